"""fp64 oracle of the iLQR controller's control step (COVO_MODE_ILQR, csrc/ilqr.hip), a plain helper module like
tests/riccati_oracle.py: a loop composed of the support modules that already exist -- the stage blocks, ladder and candidates of
tests/riccati_oracle.py, the closed-loop forward pass of tests/feedback_oracle.py and the numpy rollout cost (oracle/ref_np.py) -- for
the plants without a disturbance table (disturb kind "none": step 0 runs under the state's own force, every later one under zero).

    b_0 given (the shifted mean);  iteration j: sweep at b_j -> 17 open-loop [+ 16 closed-loop] candidates, all fp32 numbers ->
    their rollout costs -> the first cheapest is b_{j+1}

The key is not walked between iterations: every iteration judges with the same objective, so base[j + 1] == chosen[j] exactly (the
committed candidate IS the next iteration's candidate 0) and nothing moves after a choice 0.
"""
import numpy as np

from oracle import ref_np as R
from tests import feedback_oracle as FO
from tests import riccati_oracle as RO

NC = 17  # the open-loop candidates: clip(b) and the ladder's 16 step sizes


def rest_case(dpos=(0.01, 0.0, 0.0)):
    """(s, p, b): at rest 1 cm beside the hovering task's target, identity attitude, zero force, with the hover mean -- the input of the
    fixed-point checks.  The line search stalls there: the sweep succeeds on rung 0, is not flagged, and none of the 33 candidates is
    cheaper than the plan, in the fp64 loop (tests/test_ilqr_oracle.py) as on the device -- choice 0 from iteration 0.  (Exactly ON the
    target, dpos = 0, the fp64 loop also commits choice 0, but the device's sweep finds no positive definite rung there and is flagged:
    that is the path of the flagged-sweep test, not this one.)"""
    from tests.conftest import make_problem
    s, p, _ = make_problem(seed=17, time=37, task="fixed")
    s = s.replace(pos=s.pos_tar + np.asarray(dpos, dtype=np.float64), vel=np.zeros(3), quat=np.array([0.0, 0.0, 0.0, 1.0]), omega=np.zeros(3),
                  f_disturb=np.zeros(3))
    return s.astype(np.float32).astype(np.float64), p, R.hover_action(p, 32, np.float64).astype(np.float32).reshape(-1)


def plan_cost(s, p, a, reward_kind="penyaw", discount=1.0):
    """fp64 rollout cost of the action sequences a [n, 128] (or [128]) from s, under the line search's objective"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 32, 4)
    cost, _, _ = R.rollout(s.astype(np.float64), p, np.clip(a, -1.0, 1.0), discount, np.zeros(3), reward_fn=R.REWARD_FNS[reward_kind])
    return cost


def iteration(s, p, b, reward_kind="penyaw", feedback=True, discount=1.0):
    """One Riccati line search at b [128] (fp32 numbers) -> dict: b_next [128] float32, choice, costs [17 or 33], base, chosen, rung,
    mu, flagged (no rung positive definite: choice 0, b stays), alpha (0 for choice 0)"""
    b = np.asarray(b, dtype=np.float32).reshape(-1)
    b64 = b.astype(np.float64)
    forces = RO.step_forces(s, p, "none")
    blk = RO.stage_blocks(s, p, b64, reward_kind, forces)
    rung, mu, r = RO.ladder(blk)
    if r is None or not (np.isfinite(blk["g"]).all() and np.isfinite(r["d"]).all()):
        base = float(plan_cost(s, p, b64, reward_kind, discount)[0])
        return dict(b_next=np.clip(b64, -1, 1).astype(np.float32), choice=0, costs=np.asarray([base]), base=base, chosen=base, rung=rung,
                    mu=mu, flagged=True, alpha=0.0)
    cands = RO.candidates(b, r["d"])
    if feedback:
        u = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces)["u"].reshape(16, 128)
        cands = np.concatenate([cands, u.astype(np.float32).astype(np.float64)])
    costs = plan_cost(s, p, cands, reward_kind, discount)
    with np.errstate(invalid="ignore"):
        key = np.where(np.isfinite(costs), costs, np.inf)
    choice = int(np.argmin(key))  # the first cheapest: ties go to the lowest index
    alpha = 0.0 if choice == 0 else float(FO.LADDER[(choice - 1) % 16])
    return dict(b_next=cands[choice].astype(np.float32), choice=choice, costs=costs, base=float(costs[0]), chosen=float(costs[choice]),
                rung=rung, mu=mu, flagged=False, alpha=alpha)


def step(s, p, b0, k, reward_kind="penyaw", feedback=True, discount=1.0):
    """k iterations from b0 -> (means [k + 1, 128] float32: b_0 .. b_k, list of the k iteration dicts)"""
    means, its = [np.clip(np.asarray(b0, dtype=np.float32).reshape(-1), -1, 1)], []
    for _ in range(k):
        it = iteration(s, p, means[-1], reward_kind, feedback, discount)
        its.append(it)
        means.append(it["b_next"])
    return np.stack(means), its


def summary(rows, k):
    """The summary row's definition from the k Riccati rows [k, 8] (float32, as the device leaves them) -> (cost_first, cost, moved,
    fixed_at, closed, flags, grad_norm): what csrc/ilqr.hip's tally accumulates"""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float32).reshape(k, 8))
    w = rows.view(np.int32)
    choice = w[:, 2]
    zero = np.nonzero(choice == 0)[0]
    flags = 0
    for j in range(k):
        flags |= int(w[j, 7])
    return (rows[0, 0], rows[k - 1, 1], int((choice != 0).sum()), int(zero[0]) if len(zero) else k, int((choice > NC - 1).sum()),
            flags, rows[k - 1, 4])
