"""What the plan hold saves: microseconds per control step under riccati=True alone and under plan_hold=m on top of it, on the same
build and in one process, at scripts/riccati_cost.py's shapes -- covo-online (or --controller) at N = 4 096 and 65 536, the env-batched
covo-online step at 32 x 4 096.
  per-step mean   five alternating windows of 200 steps after warm-up (riccati_cost.py's protocol), the arms riccati alone and
                  m = 2, 4, 8: min / median / max of the windows
  a plan step, a hold step   under m = 8, every step synchronised on its own and timed by the host clock, by age: the latency of
                  one step of either kind, launch and synchronisation included (median of 25 plan steps / 175 hold steps)
  --ab TREE       plan_hold=1 against another checkout (the parent commit, built): `bench.py --gpus 1` in both trees, three
                  alternating runs, one process each; nothing is enqueued with the switch off, so the two should agree within the
                  process-to-process spread
    python scripts/plan_hold_cost.py [--N 4096 65536] [--E 32 --NE 4096] [--controller covo-online] [--ab TREE [--steps 200]]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PERIODS = (2, 4, 8)


def report_arms(name, steps):
    from riccati_cost import window
    for s in steps.values():
        for _ in range(48):  # (a multiple of every period: each arm's timed windows start on a plan step)
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s))
    base = np.median(us["riccati"])
    for k, v in us.items():
        print(f"{name:38s} per-step mean {k:8s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us"
              f"  ({np.median(v) - base:+8.2f} us against riccati alone)", flush=True)


def by_age(name, step, age_of, m, n=200):
    """every step synchronised on its own: host-clock latency of a plan step and of a hold step"""
    import torch
    for _ in range(2 * m):
        step()
    t = {0: [], 1: []}
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        t[1 if age_of() else 0].append((time.perf_counter() - t0) * 1e6)
    for kind, v in (("plan", t[0]), ("hold", t[1])):
        print(f"{name:38s} a {kind} step alone (m = {m}, synchronised): median {np.median(v):8.2f}  min {min(v):8.2f} us over {len(v)}",
              flush=True)


def single(name, N, dev):
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps, last = {}, None
    for arm, m in (("riccati", 1),) + tuple((f"m={m}", m) for m in PERIODS):
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, riccati=True, plan_hold=m)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)
        if name == "covo-offline":
            st["cp"] = c.reset(state, params, st["cp"], cr.PRNGKey(2))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
        last = c
    report_arms(f"{name} N={N}", steps)
    by_age(f"{name} N={N}", steps[f"m={PERIODS[-1]}"], lambda: last.core._plan_ages()[1], PERIODS[-1])


def batched(E, N, dev):
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps, last = {}, None
    for arm, m in (("riccati", 1),) + tuple((f"m={m}", m) for m in PERIODS):
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, riccati=True, plan_hold=m)
        b.set_instances([s[2] for s in states], params)
        b([s[1]["noisy_state"] for s in states], keys)
        b.reset(None, None, None)  # (the timed windows start on a plan step)
        steps[arm] = lambda b=b: b(None, keys)
        last = b
    report_arms(f"batched covo-online E={E} N={N}", steps)
    by_age(f"batched covo-online E={E} N={N}", steps[f"m={PERIODS[-1]}"], lambda: last.plan_age, PERIODS[-1])


def ab(tree, steps, warmup):
    """bench.py's headline in this tree (plan_hold off: its default) and in `tree`, three alternating runs"""
    vals = {"this": [], "other": []}
    for r in range(3):
        for arm, cwd in (("other", tree), ("this", ROOT)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=cwd,
                                 capture_output=True, text=True, timeout=420, check=True).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            vals[arm].append(float(json.loads(line)["value"]))
            print(f"A/B run {r} {arm:5s}: {vals[arm][-1]:9.1f} control-steps/s", flush=True)
    for arm, v in vals.items():
        print(f"A/B {arm:5s}: min {min(v):9.1f}  median {np.median(v):9.1f}  max {max(v):9.1f} control-steps/s")
    print(f"A/B this / other (medians): {np.median(vals['this']) / np.median(vals['other']):.4f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="*", default=[4096, 65536])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--controller", default="covo-online")
    ap.add_argument("--ab", metavar="TREE", default=None, help="only the A/B of bench.py against the checkout at TREE")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.ab:
        ab(os.path.abspath(a.ab), a.steps, a.warmup)
        sys.exit(0)
    for N in a.N:
        single(a.controller, N, "cuda:0")
    if a.E > 0:
        batched(a.E, a.NE, "cuda:0")
