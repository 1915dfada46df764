import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from covo_mpc_amd.controllers._options import STEP_SWITCH_DEFAULTS
from covo_mpc_amd.envs import quadrotor as Q
name = sys.argv[1]
# python scripts/eval_seeds.py covo-online [elite=512]: the elite-set update with K elites instead of the softmax weights
# python scripts/eval_seeds.py covo-online --sigma-period 4 (or sigma_period=4): Sigma refreshed every 4th control step
# python scripts/eval_seeds.py covo-online --sigma-period 4 --sigma-adapt 0.1 (or sigma_adapt=0.1): the reuse steps blend the posterior
# covariance into the covariance they shift
# python scripts/eval_seeds.py covo-online ess_min=64 / iters=2: the ESS floor / two passes per control step
# Under ess_min, sigma_adapt and iters every seed's line also carries what the episode logs of the attachments' rows say (read_lam,
# read_sigma, read_iters): the share of steps the floor raised the temperature in, the number of reuse steps that fell back to the plain
# shift, the share of steps whose last pass found a cheaper sample than the first
# python scripts/eval_seeds.py covo-online --refine: every control step ends with the Newton line search on its committed mean (the
# refine row has no episode log: compare the errors with those of the same call without the flag)
# python scripts/eval_seeds.py mppi --riccati (or covo-offline, covo-online, with any --sigma-period): every control step ends with the
# same line search along the Riccati sweep's direction (csrc/riccati.hip); again, compare with the same call without the flag
# python scripts/eval_seeds.py mppi --riccati --riccati-feedback: the closed-loop candidates under the sweep's gains compete in that line
# search (csrc/feedback_rollout.hip); compare with the same call without the last flag
# python scripts/eval_seeds.py mppi --riccati --plan-hold 4: every 4th control step plans, the three between apply the sweep's law to the
# measured state (csrc/plan_hold.hip); every seed's line also carries the share of hold steps whose plan belonged to another trajectory
# (flag bit 2: a reset in between) and the share with a clipped component; compare the errors with --riccati alone
# python scripts/eval_seeds.py ilqr [iters=k] [--plan-hold m]: the sampling-free controller (controllers/ilqr.py), k Riccati line searches
# per control step (default 1: get_controller's); every seed's line also carries the share of plan steps that reached a fixed point
# (ilqr_fixed_at < k) and the share that committed a closed-loop candidate in some iteration, summed on the device from the info dict
# (the host loop of __call__ + episode.step: the summary row has no episode log)
# python scripts/eval_seeds.py ilqr iters=2 --riccati-box (or mppi --riccati --riccati-feedback --riccati-box): every sweep solves the
# control-limited stage problem (csrc/riccati.hip, the box form); compare with the same call without the flag.  Under ilqr every seed's
# line also carries the share of plan steps whose first sweep clamped a coordinate (the masks have no episode log)
# python scripts/eval_seeds.py dial [iters=k] [beta_pass=b] [beta_stage=b] [temp=t | temp=none]: the annealed MPPI controller
# (controllers/dial.py; defaults: get_controller's iters=1, 0.5 / 0.9 / 0.1); compare with `mppi iters=k`.  With temp every seed's line
# also carries the share of steps whose last pass fell back to the configured temperature (the temperature log's bit 31 of entry 3)
# python scripts/eval_seeds.py dial iters=k nodes=M [node_interp=cubic]: the same controller with spline-node perturbations
# python scripts/eval_seeds.py cma [gamma=g] [damping=d] [s_min=a] [s_max=b] [step_size=0] [iters=k] [elite=K] [ess_min=e]: the CMA
# controller (controllers/cma.py; defaults gamma=0.2, damping=1, s_min=0.1, s_max=4); every seed's line also carries the step size and
# the flag word the last episode ended with
# python scripts/eval_seeds.py <controller> [...] --estimator [force_std=f]: a controllers.StateEstimator attached to the controller that
# was built (csrc/state_estimator.hip): every control step plans from the filter's estimate of the noisy state; every seed's line also
# carries the mean distance the estimate moved the measured position and the share of steps that (re-)initialised; compare the errors with
# the same call without the flag
# python scripts/eval_seeds.py <controller> [...] --observer [force_walk_std=w] [disturb=periodic] [seeds=k]: a controllers.ForceObserver
# attached instead (csrc/force_observer.hip): every control step plans from a row whose disturbance force is the observer's estimate, not
# the plant's own; every seed's line also carries the RMS error of that estimate over the RMS of the true force and the share of steps
# that (re-)initialised; compare the errors with the same call without the flag.  disturb= picks the plant's disturbance model (default
# gaussian), seeds= the number of seeds (default 12), with or without a filter
rest = sys.argv[2:]
with_estimator = "--estimator" in rest
with_observer = "--observer" in rest
assert not (with_estimator and with_observer), "--estimator and --observer: two filters must not write one row"
rest = [r for r in rest if r not in ("--estimator", "--observer")]
# the boolean step switches as flags: --refine, --riccati, --riccati-feedback, --riccati-box
flags = {f"--{s.replace('_', '-')}": s for s, default in STEP_SWITCH_DEFAULTS.items() if isinstance(default, bool)}
switches = {s: flag in rest for flag, s in flags.items()}
rest = [r for r in rest if r not in flags]
for flag, key in (("--sigma-period", "sigma_period"), ("--sigma-adapt", "sigma_adapt"), ("--plan-hold", "plan_hold")):
    while flag in rest:
        i = rest.index(flag)
        rest[i:i + 2] = [f"{key}={rest[i + 1]}"]
FLOATS = ("force_std", "force_walk_std", "sigma_adapt", "ess_min", "beta_pass", "beta_stage", "temp", "gamma", "damping", "s_min", "s_max")
CMA_KEYS = ("gamma", "damping", "s_min", "s_max", "step_size")
opts = {k: (None if v.lower() == "none" else v if k in ("node_interp", "disturb") else float(v) if k in FLOATS else int(v))
        for k, v in (arg.split("=") for arg in rest)}
switches["plan_hold"] = opts.pop("plan_hold", 1)
force_std = opts.pop("force_std", None)
assert force_std is None or with_estimator, "force_std= belongs to --estimator"
force_walk_std = opts.pop("force_walk_std", None)
assert force_walk_std is None or with_observer, "force_walk_std= belongs to --observer"
disturb, n_seeds = opts.pop("disturb", "gaussian"), opts.pop("seeds", 12)
assert set(opts) <= ({"elite", "sigma_period", "sigma_adapt", "ess_min", "iters"} |
                     ({"beta_pass", "beta_stage", "temp", "nodes", "node_interp"} if name == "dial" else set()) |
                     (set(CMA_KEYS) if name == "cma" else set())), opts
cma_kw = {k: (bool(opts.pop(k)) if k == "step_size" else opts.pop(k)) for k in CMA_KEYS if k in opts}
env = Q.Quad3D(task="tracking_zigzag", obs_type="quad", lower_controller="base", enable_randomizer=False,
               disturb_type=disturb, disable_rollover_terminate=True, generate_noisy_state=True, device="cuda")
ctrl, cp = Q.get_controller(env, name, "N8192_H32_lam0.01", **switches, **opts)
if cma_kw:  # (get_controller's signature carries none of them: the controller is built again with them)
    from covo_mpc_amd import controllers
    ctrl.core.close()
    ctrl = controllers.CMAController(env, cp, ctrl.N, ctrl.H, ctrl.lam, **cma_kw, **{k: v for k, v in opts.items() if k in ("elite", "ess_min", "iters")})
if with_estimator:
    from covo_mpc_amd.controllers import StateEstimator
    StateEstimator(env, force_std=force_std).attach(ctrl)
if with_observer:
    from covo_mpc_amd.controllers import ForceObserver
    ForceObserver(env, force_walk_std=force_walk_std).attach(ctrl)
np.set_printoptions(precision=3, linewidth=200)
allerr = []
core = getattr(ctrl, "core", None)


class IlqrTally:
    """the iLQR controller behind eval_env_device's host loop (no run_episode), counting what its info dict says on the device"""
    def __init__(self, c):
        import torch
        self.c, self.core, self.init_control_params, self.alias_outputs = c, c.core, c.init_control_params, False
        # plan steps, of them at a fixed point, with a closed-loop commit, with a clamped coordinate in the first sweep
        self.acc = torch.zeros(4, dtype=torch.int64, device=c.core.device)

    def reset(self, *a):
        return self.c.reset(*a)

    def __call__(self, *a):
        self.c.alias_outputs = self.alias_outputs
        u, cp, info = self.c(*a)
        if info.get("plan_age", 0) == 0:
            self.acc[0] += 1
            self.acc[1] += info["ilqr_fixed_at"] < self.c.iters
            self.acc[2] += info["ilqr_closed"] > 0
            if "ilqr_box_count" in info:
                self.acc[3] += info["ilqr_box_count"][0] > 0
        return u, cp, info


if name == "ilqr":
    ctrl = IlqrTally(ctrl)


def rows_of(ep):
    """what the episode's row logs say, summed into `rows` ({} for a controller without them)"""
    if ep.lamlog is not None and name == "dial":
        words = np.ascontiguousarray(ep.read_lam()["evaluations"]).view(np.int32)  # (entry 3 of the row: bits(|F| | fallback << 31))
        rows["fellback"] = rows.get("fellback", 0) + int((words < 0).sum())
    elif ep.lamlog is not None:
        rows["floor"] = rows.get("floor", 0) + int((ep.read_lam()["lam_eff"] > np.float32(core.lam)).sum())
    if ep.sigmalog is not None and core.sigma_adapt_gamma > 0.0:
        rows["fallback"] = rows.get("fallback", 0) + int((ep.read_sigma()["fallback"] != 0.0).sum())
    if ep.iterlog is not None:
        it = ep.read_iters()
        rows["improved"] = rows.get("improved", 0) + int((it[:, -1] < it[:, 0]).sum())
    if ep.holdlog is not None:
        hold = ep.read_hold()
        held = hold["age"] > 0
        rows["held"] = rows.get("held", 0) + int(held.sum())
        rows["stale"] = rows.get("stale", 0) + int(((hold["flags"] & 4) != 0)[held].sum())
        rows["clipped"] = rows.get("clipped", 0) + int((hold["clipped"] > 0)[held].sum())
    if ep.estlog is not None:
        e = ep.read_estimate()
        rows["est_init"] = rows.get("est_init", 0) + int((e["flags"] != 0).sum())
        rows["est_moved"] = rows.get("est_moved", 0.0) + float(e["moved_pos"].sum())
    if ep.obslog is not None:
        e = ep.read_force()
        rows["obs_init"] = rows.get("obs_init", 0) + int((np.ascontiguousarray(e["rows"][:, 0]).view(np.int32) != 0).sum())
        rows["obs_err2"] = rows.get("obs_err2", 0.0) + float(((e["force_est"] - e["force_true"]).astype(np.float64) ** 2).sum())
        rows["obs_true2"] = rows.get("obs_true2", 0.0) + float((e["force_true"].astype(np.float64) ** 2).sum())
    if name == "cma":
        row = core.cma_rows[0].cpu().numpy()
        rows["cma_s"], rows["cma_flags"] = float(row[0]), float(row[7])
    rows["steps"] = rows.get("steps", 0) + ep.n_steps


for seed in range(1, 1 + n_seeds):
    rows = {}
    errs = Q.eval_env_device(env, controller=ctrl, total_steps=300*4*10, seed=seed, verbose=False, on_episode=rows_of if core else None)
    allerr.append(errs)
    if name == "ilqr":
        acc = ctrl.acc.cpu().numpy()
        ctrl.acc.zero_()
        rows["fixed"], rows["closed"], rows["plans"] = int(acc[1]), int(acc[2]), int(acc[0])
        if switches["riccati_box"]:
            rows["boxed"] = int(acc[3])
    n = max(rows.get("steps", 0), 1)
    if "obs_err2" in rows:
        rows["obs_ratio"] = (rows["obs_err2"] / max(rows["obs_true2"], 1e-300)) ** 0.5
    npl = max(rows.get("plans", 0), 1)
    nh = max(rows.get("held", 0), 1)
    extra = "".join(text % (rows[k] / d) for k, text, d in (("floor", "  lam_eff>lam: %.3f", n), ("fallback", "  adapt fallbacks: %d", 1),
                                                           ("fellback", "  last pass at the configured lam: %.3f", n),
                                                           ("improved", "  last pass beat first: %.3f", n),
                                                           ("fixed", "  plan steps at a fixed point: %.3f", npl),
                                                           ("closed", "  plan steps with a closed-loop commit: %.3f", npl),
                                                           ("boxed", "  plan steps with a live box: %.3f", npl),
                                                           ("stale", "  hold steps on another trajectory's plan: %.3f", nh),
                                                           ("clipped", "  hold steps with a clipped component: %.3f", nh),
                                                           ("est_moved", "  estimate moved the position by: %.4f", n),
                                                           ("est_init", "  steps that (re-)initialised the filter: %.4f", n),
                                                           ("obs_ratio", "  rms force error / rms force: %.3f", 1),
                                                           ("obs_init", "  steps that (re-)initialised the observer: %.4f", n),
                                                           ("cma_s", "  last step size: %.3f", 1), ("cma_flags", "  last flags: %d", 1)) if k in rows)
    print(name, "seed", seed, "mean %.3f med %.3f max %.3f  n>0.1: %d" % (errs.mean(), np.median(errs), errs.max(), (errs > 0.1).sum()) + extra,
          flush=True)
allerr = np.concatenate(allerr)
print(name, "TOTAL n", len(allerr), "crashes(>0.3)", (allerr > 0.3).sum(), "outliers(>0.06)", (allerr > 0.06).sum(), "median %.4f" % np.median(allerr), "mean-noncrash %.4f" % allerr[allerr<0.3].mean())
