"""What the spline-node sampler costs.
1. The sampler alone (covo_noise_nodes_philox) against the block-diagonal kernel alone (covo_noise_blockdiag_philox) at each N, for
   M in --Ms and every stage split S in --splits: 200 launches captured into one graph, device events around ten replays, five times,
   min / median / max microseconds per launch.  S is read once per process (COVO_NODES_SPLIT), so every S runs in a child process of its
   own.  The stand-alone entry has no instance dimension: 32 x 4 096 is measured as one launch of N = 131 072 -- the same workgroups and
   bytes, the instance on the sample axis instead of blockIdx.z.
2. dial(nodes=8) against dial() at k = 4 passes: microseconds per control step, five alternating windows of 200 steps after warm-up
   (scripts/anneal_cost.py's protocol), at N = 4 096 and 65 536, and for 32 x 4 096 env-batched instances.
   nodes=32 linear is dial() value for value, so that arm differs from dial() in the sampler's launch alone; the nodes=8 arms also see
   other samples, and the update's cost depends on how many of them keep a weight.
    python scripts/nodes_cost.py [--Ns 4096 65536 131072] [--Ms 4 8 16 32] [--splits 1 2 4 8] [--E 32 --NE 4096] [--k 4]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._options import node_schedule  # noqa: E402
from scripts.anneal_cost import report  # noqa: E402

DEV = "cuda:0"


def graph_us(call, stream, R=200, replays=10):
    """R launches in one captured graph -> (min, median, max) microseconds per launch over five timings of `replays` replays; `stream`
    is asked for the current stream at every launch (under capture: the capturing one)"""
    _lib.check(call(stream()), "launch")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(R):
            _lib.check(call(stream()), "launch")
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / (R * replays))
    return min(us), float(np.median(us)), max(us)


def sampler_alone(Ns, Ms, with_block):
    split = os.environ.get("COVO_NODES_SPLIT", "default")
    for N in Ns:
        core = cm.controllers._core.SamplingCore(N, 32, 0.01, 1.0, device=DEV, compute_info=False)
        lib, h = core.lib, core.h
        mu = torch.zeros(128, dtype=torch.float32, device=DEV)
        if with_block:
            Ls = (0.5 * torch.eye(4, device=DEV)).repeat(32, 1, 1).contiguous()
            lo, med, hi = graph_us(lambda s: lib.covo_noise_blockdiag_philox(h, _lib.ptr(Ls), _lib.ptr(mu), 3, 4, 0, N, _lib.ptr(core.a), s),
                                   core.stream)
            print(f"sampler alone N={N:6d} noise_blockdiag        : min {lo:6.2f}  median {med:6.2f}  max {hi:6.2f} us/launch", flush=True)
        for M in Ms:
            B = torch.from_numpy(node_schedule(0.5, 1, 0.5, 0.9, M, "cubic")[1][0]).to(DEV).contiguous()
            lo, med, hi = graph_us(lambda s: lib.covo_noise_nodes_philox(h, _lib.ptr(B), M, _lib.ptr(mu), 3, 4, 0, N, _lib.ptr(core.a), s),
                                   core.stream)
            print(f"sampler alone N={N:6d} noise_nodes M={M:2d} S={split:7s}: min {lo:6.2f}  median {med:6.2f}  max {hi:6.2f} us/launch",
                  flush=True)
        core.close()


def single(N, k):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    # nodes=32 linear is dial() value for value: the arm that differs from it in the sampler's launch alone
    arms = {"dial": dict(iters=k), "dial-nodes32": dict(iters=k, nodes=32), "dial-nodes8": dict(iters=k, nodes=8),
            "dial-nodes8c": dict(iters=k, nodes=8, node_interp="cubic")}
    steps = {}
    for arm, kw in arms.items():
        c, _ = cm.envs.get_controller(env, "dial", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, **kw)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.reset(state, params, c.init_control_params, cr.PRNGKey(2)))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
    m = report(f"single N={N} k={k}", steps)
    print(f"{'':28s} dial-nodes8 - dial {m['dial-nodes8'] - m['dial']:+.2f} us/step ({(m['dial-nodes8'] - m['dial']) / k:+.2f} per pass)",
          flush=True)


def batched(E, N, k):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps = {}
    for arm, kw in (("dial", {}), ("dial-nodes32", dict(nodes=32)), ("dial-nodes8", dict(nodes=8))):
        b = cm.controllers.BatchedDialController(env, E, N, 32, 0.01, iters=k, a_mean_init=cp0.a_mean, device=DEV, **kw)
        b.set_instances([s[2] for s in states], params)
        b([s[1]["noisy_state"] for s in states], keys)
        steps[arm] = lambda b=b: b(None, keys)
    m = report(f"batched E={E} N={N} k={k}", steps)
    print(f"{'':28s} dial-nodes8 - dial {m['dial-nodes8'] - m['dial']:+.2f} us/step", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--Ns", type=int, nargs="+", default=[4096, 65536, 131072])
    ap.add_argument("--Ms", type=int, nargs="+", default=[4, 8, 16, 32])
    ap.add_argument("--splits", type=int, nargs="*", default=[1, 2, 4, 8], help="(none: skip the sampler alone)")
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--sampler-child", action="store_true", help="(internal) the sampler's timings for this process's COVO_NODES_SPLIT")
    ap.add_argument("--with-block", action="store_true", help="(internal) also time the block-diagonal kernel")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nodes_cost.py measures on the GPU; there is none")
    if a.sampler_child:
        sampler_alone(a.Ns, a.Ms, a.with_block)
        raise SystemExit(0)
    for i, S in enumerate(a.splits):  # a fresh child per S: the library reads the split once
        cmd = [sys.executable, os.path.abspath(__file__), "--sampler-child", "--Ns", *map(str, a.Ns), "--Ms", *map(str, a.Ms)]
        rc = subprocess.run(cmd + (["--with-block"] if i == 0 else []), env=dict(os.environ, COVO_NODES_SPLIT=str(S)), timeout=240).returncode
        if rc != 0:
            raise SystemExit(f"the sampler's child for S={S} ended with {rc}")
    for N in a.Ns[:2]:
        single(N, a.k)
    batched(a.E, a.NE, a.k)
