"""What covo-online in spline-node space costs.
1. The two kernels alone at each M in --Ms: covo_sigma_nodes on one real Hessian and on a batch of --E copies of it, next to the Sigma
   chain (covo_sigma) on the same input, and covo_noise_factor_philox at each N in --Ns next to the noise GEMM with the in-kernel draw
   (covo_noise_gemm_philox): 200 launches captured into one graph, device events around ten replays, five times, min / median / max
   microseconds per launch (scripts/nodes_cost.py's protocol).  The stand-alone sampler has no instance dimension: E x NE is measured as
   one launch of N = E NE -- the same workgroups and bytes, the instance on the sample axis instead of blockIdx.z.
2. CoVOController(mode="online", sigma_nodes=M) against the same controller without the keyword -- the step as it was: with the keyword
   at None nothing is attached and no launch changes --, microseconds per control step, five alternating windows of 200 steps after
   warm-up (scripts/anneal_cost.py's protocol), at each N in --Ns, and BatchedCoVOController for --E x --NE instances.  The arms with
   the keyword also see other samples, and the update's cost depends on how many of them keep a weight.
    python scripts/sigma_nodes_cost.py [--Ns 4096 65536] [--Ms 4 8 16] [--E 32 --NE 4096]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._options import node_basis  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from scripts.anneal_cost import report  # noqa: E402
from scripts.nodes_cost import graph_us  # noqa: E402

DEV = "cuda:0"


def _env(batched=False):
    if batched:
        return cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                              disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    return cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                          generate_noisy_state=True, device=DEV)


def _online(env, N, cp=None, **kw):
    if cp is None:
        c0, cp = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
        c0.core.close()
    return cm.controllers.CoVOController(env, cp, N, 32, 0.01, "online", device=DEV, compute_info=False, **kw), cp


def kernels_alone(Ns, Ms, E, NE):
    env = _env()
    core = cm.controllers._core.SamplingCore(max(max(Ns), E * NE), 32, 0.01, 1.0, device=DEV, compute_info=False)
    lib, h = core.lib, core.h
    c, _ = _online(env, 256)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    ds = as_device_state(info["noisy_state"], DEV)
    mu = torch.zeros(128, dtype=torch.float32, device=DEV)
    mu[0::4] = -0.6
    R1 = core.hessian(ds.packed, ds, c._params_c(params), mu)
    c.core.close()
    f32 = dict(dtype=torch.float32, device=DEV)
    for batch in (1, E):
        R = R1.repeat(batch, 1, 1).contiguous()
        Sig, L = torch.empty((batch, 128, 128), **f32), torch.empty((batch, 128, 128), **f32)
        lo, med, hi = graph_us(lambda s: lib.covo_sigma(h, _lib.ptr(R), batch, 0.5, _lib.ptr(Sig), _lib.ptr(L), s), core.stream)
        print(f"kernel alone batch={batch:2d} Sigma chain (covo_sigma): min {lo:7.2f}  median {med:7.2f}  max {hi:7.2f} us/launch", flush=True)
        for M in Ms:
            d = 4 * M
            W = torch.from_numpy(node_basis(M, "linear")).to(DEV).contiguous()
            SM = torch.empty((batch, d, d), dtype=torch.float64, device=DEV)
            G = torch.empty((batch, 128, d), **f32)
            rows = torch.empty((batch, 8), **f32)
            lo, med, hi = graph_us(lambda s: lib.covo_sigma_nodes(h, _lib.ptr(R), batch, _lib.ptr(W), M, 0.5, _lib.ptr(SM), _lib.ptr(G),
                                                                  _lib.ptr(Sig), _lib.ptr(rows), s), core.stream)
            torch.cuda.synchronize()
            print(f"kernel alone batch={batch:2d} sigma_nodes M={M:2d} (sweeps {int(rows[0, 5])}, flags {int(rows[0, 6])}): "
                  f"min {lo:7.2f}  median {med:7.2f}  max {hi:7.2f} us/launch", flush=True)
    L1 = L[0].contiguous()
    for N in list(Ns) + [E * NE]:
        lo, med, hi = graph_us(lambda s: lib.covo_noise_gemm_philox(h, _lib.ptr(L1), _lib.ptr(mu), 3, 4, 0, N, _lib.ptr(core.a), s),
                               core.stream)
        print(f"kernel alone N={N:6d} noise GEMM (in-kernel draw): min {lo:7.2f}  median {med:7.2f}  max {hi:7.2f} us/launch", flush=True)
        for M in Ms:
            G1 = (0.1 * torch.randn((128, 4 * M), generator=torch.Generator().manual_seed(M))).to(DEV).contiguous()
            lo, med, hi = graph_us(lambda s: lib.covo_noise_factor_philox(h, _lib.ptr(G1), 4 * M, _lib.ptr(mu), 3, 4, 0, N,
                                                                          _lib.ptr(core.a), s), core.stream)
            print(f"kernel alone N={N:6d} noise_factor d={4 * M:2d}          : min {lo:7.2f}  median {med:7.2f}  max {hi:7.2f} us/launch",
                  flush=True)
    core.close()


def single(N, Ms):
    env = _env()
    arms = {"covo-online": {}}
    arms.update({f"nodes{M}": dict(sigma_nodes=M) for M in Ms})
    steps, cp0 = {}, None
    for arm, kw in arms.items():
        c, cp0 = _online(env, N, cp0, **kw)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.reset(state, params, cp0, cr.PRNGKey(2)))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
    m = report(f"single N={N}", steps)
    for M in Ms:
        print(f"{'':28s} nodes{M} - covo-online {m[f'nodes{M}'] - m['covo-online']:+.2f} us/step", flush=True)


def batched(E, N, Ms):
    env = _env(batched=True)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    c0.core.close()
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps = {}
    for arm, kw in [("covo-online", {})] + [(f"nodes{M}", dict(sigma_nodes=M)) for M in Ms]:
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=DEV, **kw)
        b.set_instances([s[2] for s in states], params)
        b([s[1]["noisy_state"] for s in states], keys)
        steps[arm] = lambda b=b: b(None, keys)
    m = report(f"batched E={E} N={N}", steps)
    for M in Ms:
        print(f"{'':28s} nodes{M} - covo-online {m[f'nodes{M}'] - m['covo-online']:+.2f} us/step", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--Ns", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--Ms", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sigma_nodes_cost.py measures on the GPU; there is none")
    kernels_alone(a.Ns, a.Ms, a.E, a.NE)
    for N in a.Ns:
        single(N, a.Ms)
    batched(a.E, a.NE, a.Ms)
