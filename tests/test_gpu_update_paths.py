"""GPU tests (-m gpu): the new mean (and MPPI's adapted covariance) of REAL control steps on every update path, against numpy fp64 on
the step's own fp32 costs and actions (tests/update_oracle.py::check_update) -- the cost error of an fp64 rollout is out of the
picture, so there is no escape hatch, and the bar is the project's 1e-5 absolute.

Paths, each at the smallest sizes that reach it (eager and as a captured graph where the path has both):
  record-leaving rollout (covo-online; csrc/rollout_common.hpp: rollout_record)  1 group per workgroup N = 65, 4 096; 2 groups
      N = 16 448 (257 groups); 4 groups N = 32 832 (513 groups), 65 536
  stand-alone stage 1 inside a step (more rollout workgroups than records)       covo-online N = 65 600
  one-launch small step (csrc/step_small.hip), covo-offline and MPPI              N = 40, 1 000 (gamma_mean 0.7), 16 384
  the same staged (covo_debug_set_fuse_small(0))                                  N = 1 000
  MPPI with gamma_sigma = 0.3 (second-moment stage 1 + merge_cov_body)            N = 257, 4 096: mean and covariance
  env-batched fused covo-online / MPPI / covo-offline, env-batched staged MPPI / covo-offline   3 instances x N = 1 024, every instance
  sample-sharded rank records + covo_merge_ranks on one GPU                       2 x 1 024
Every path runs at lambda = 0.01, 0.1, 1, 1e4 (one controller per lambda: it is the handle's).  Coverage, asserted per path over its
lambda loop: at least one step each with n_live <= 8, with 8 < n_live < N and with n_live == N (n_live: the samples whose fp32 weight
is > 0).  Where the four temperatures miss a regime, a further temperature is computed from the first step's costs (they do not
depend on lambda): the k-th smallest cost 105 lambda above the minimum.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests import update_oracle as U  # noqa: E402
from tests.gpu_support import DEV, instances, quad_env, single_controller  # noqa: E402

LAMS = (0.01, 0.1, 1.0, 1e4)
REGIMES = ("few", "some", "all")


class Coverage:
    """The regimes a path's steps ran in and its worst errors; run(lam) -> the first step's costs."""

    def __init__(self, path, N):
        self.path, self.N, self.seen, self.err, self.err_cov = path, N, set(), 0.0, 0.0

    def add(self, out):
        self.seen.add(U.regime(out["n_live"], out["N"]))
        self.err = max(self.err, out["err"])
        self.err_cov = max(self.err_cov, out["err_cov"] or 0.0)

    def finish(self, run, cost0):
        """The temperatures for the regimes the four fixed ones missed, then the conditions."""
        targets = {"few": 4, "some": max(self.N // 16, 12), "all": None}
        for r in REGIMES:
            if r not in self.seen:
                c = np.sort(np.asarray(cost0, dtype=np.float64))
                lam = float((c[-1] - c[0]) / 50.0) if r == "all" else U.lam_for_live(cost0, targets[r])
                print(f"  {self.path}: regime '{r}' not met at lambda = {LAMS}: a further temperature {lam:.6g}")
                run(lam)
        print(f"  {self.path} N {self.N}: regimes {sorted(self.seen)}, worst mean err {self.err:.2e}, worst cov err {self.err_cov:.2e}")
        assert self.seen == set(REGIMES), (self.path, self.N, self.seen)


def _single_path(path, name, N, graph, monkeypatch, gamma_mean=1.0, gamma_sigma=0.0, fuse_small=None):
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    cov_check = gamma_sigma != 0.0
    cover = Coverage(f"{path} {name} {graph}", N)
    first = {}

    def run(lam):
        c, cp, obs, info, state, params = single_controller(env, name, N, lam=repr(lam))
        assert c.core.uses_graph == (graph == "graph")
        if fuse_small is not None:
            _lib.check(c.core.lib.covo_debug_set_fuse_small(c.core.h, fuse_small), "fuse_small")
        cp = cp.replace(gamma_mean=gamma_mean)
        if cov_check:
            cp = cp.replace(gamma_sigma=gamma_sigma)
        key = cr.PRNGKey(3)
        for step in range(3 if graph == "graph" else 2):  # graph: eager first call, capture, replay
            key, k_act, k_step = cr.split(key, 3)
            before = cp
            u, cp, _ = c(obs, state, params, k_act, cp, info)
            torch.cuda.synchronize()
            out = U.check_update(c.core, before.a_mean, gamma_mean, lam, cp.a_mean, before.a_cov if cov_check else None,
                                 gamma_sigma if cov_check else None, cp.a_cov if cov_check else None,
                                 where=f"{path} {name} {graph} step {step}")
            cover.add(out)
            if step == 0:
                first.setdefault("cost", c.core.cost.cpu().numpy().copy())
            obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
        assert c.core.device_status() == 0
        c.core.close()

    for lam in LAMS:
        run(lam)
    cover.finish(run, first["cost"])


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("N", [65, 4096, 16448, 32832, 65536])
def test_record_leaving_rollout(N, graph, monkeypatch):
    """covo-online: the rollout's workgroups leave the softmax records, the launch's last workgroup merges them -- 1, 2 and 4
    64-sample groups per workgroup; N = 65: the second workgroup holds one sample; 16 448 / 32 832: the last workgroup half empty /
    with one group of four."""
    _single_path("record-leaving rollout", "covo-online", N, graph, monkeypatch)


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_standalone_stage1_inside_a_step(graph, monkeypatch):
    """N = 65 600: 257 rollout workgroups, more than the merge takes records -- the stand-alone stage 1 forms them, its grid capped,
    its waves striding."""
    _single_path("stand-alone stage 1", "covo-online", 65600, graph, monkeypatch)


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("N", [40, 1000, 16384])
@pytest.mark.parametrize("name", ["covo-offline", "mppi"])
def test_one_launch_small_step(name, N, graph, monkeypatch):
    _single_path("one-launch small step", name, N, graph, monkeypatch, gamma_mean=0.7 if N == 1000 else 1.0)


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name", ["covo-offline", "mppi"])
def test_small_step_staged(name, graph, monkeypatch):
    _single_path("staged small step", name, 1000, graph, monkeypatch, gamma_mean=0.7, fuse_small=0)


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("N", [257, 4096])
def test_mppi_covariance_adaptation(N, graph, monkeypatch):
    """gamma_sigma = 0.3: stage 1 with second moments and merge_cov_body -- the mean and the adapted covariance."""
    _single_path("MPPI gamma_sigma", "mppi", N, graph, monkeypatch, gamma_sigma=0.3)


_TABLES = {}


# ------------------------------------------------------------------------------------------ env-batched steps
def _batched_path(path, name, staged, N=1024, E=3):
    import covo_mpc_amd as cm
    env = quad_env(task="tracking", randomizer=True)
    cover = Coverage(f"{path} {name}", N)
    first = {}

    def run(lam):
        inst = instances(env, None, None, None, E, controllers=False)
        hover = env.default_params.m * env.default_params.g / env.default_params.max_thrust * 2.0 - 1.0
        a0 = torch.tensor([hover, 0.0, 0.0, 0.0], dtype=torch.float32).repeat(32, 1)
        kw = dict(staged=True) if staged else {}
        if name == "mppi":
            b = cm.controllers.BatchedMPPIController(env, E, N, 32, float(lam), a_mean_init=a0, device=DEV, **kw)
        else:
            b = cm.controllers.BatchedCoVOController(env, E, N, 32, float(lam), a_mean_init=a0, device=DEV,
                                                     mode="offline" if name == "covo-offline" else "online", **kw)
        b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
        if name == "covo-offline":
            if "t" not in _TABLES:
                _TABLES["t"] = b.reset([i["state"] for i in inst], [i["params"] for i in inst], [i["reset_key"] for i in inst])
            b.set_tables(*_TABLES["t"])
        for step in range(3):  # (the batched controllers replay a graph: eager first call, capture, replay)
            k_acts = []
            for i in inst:
                i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
                k_acts.append(np.asarray(k_act))
            before = b.a_mean.clone()
            u = b([i["info"]["noisy_state"] for i in inst], np.stack(k_acts)).clone()
            torch.cuda.synchronize()
            for e, i in enumerate(inst):  # every instance with its own rows
                cover.add(U.check_update((b._cost[e], b._a[e]), before[e], 1.0, lam, b.a_mean[e],
                                         where=f"{path} {name} step {step} instance {e}"))
                if step == 0 and e == 0:
                    first.setdefault("cost", b._cost[0].cpu().numpy().copy())
                i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u[e].cpu().numpy(), i["params"])
        assert b.core.device_status() == 0
        b.core.close()

    for lam in LAMS:
        run(lam)
    cover.finish(run, first["cost"])


@pytest.mark.parametrize("name", ["covo-online", "mppi", "covo-offline"])
def test_env_batched_fused_step(name):
    _batched_path("env-batched fused", name, staged=False)


@pytest.mark.parametrize("name", ["mppi", "covo-offline"])
def test_env_batched_staged_step(name):
    _batched_path("env-batched staged", name, staged=True)


# ------------------------------------------------------------------------------------------ sample-sharded ranks on one GPU
def test_sharded_rank_records_merged_on_one_gpu():
    """Two 1 024-sample shards of one covo-offline step (the set-up of test_gpu_parity.py::
    test_small_fused_step_on_a_sharded_rank_leaves_the_merged_record): each leaves its rank record {m, s, v} through partial_out,
    covo_merge_ranks merges the two -- against mean64 on the 2 048 costs and actions of both shards."""
    from covo_mpc_amd.dynamics.dataclass import as_device_state
    n, G = 1024, 2
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(3), params)
    dstate = as_device_state(info["noisy_state"], DEV)
    pc = params.to_c()
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 128, 128, generator=g, dtype=torch.float64)
    L = torch.linalg.cholesky(0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64)).float().to(DEV).contiguous()
    hover = params.m * params.g / params.max_thrust * 2.0 - 1.0
    a_mean0 = (torch.tensor([hover, 0.0, 0.0, 0.0]).repeat(32) + 0.05 * torch.randn(128, generator=g)).to(DEV)
    cover = Coverage("sharded rank records", G * n)
    first = {}

    def run(lam):
        core = SamplingCore(n, 32, lam, 1.0, device=DEV, use_graph=False)
        for gamma in (1.0, 0.7):
            records = torch.zeros((G, _lib.COVO_RANK_RECORD_FLOATS), device=DEV)
            costs, acts = [], []
            for r in range(G):
                args, am, am_shift, _ = core._prepare_step(_lib.MODE_COVO_OFFLINE, dstate, a_mean0, L_table=L, derive_keys=True,
                                                           gamma_mean=gamma)
                args.partial_out = records[r].data_ptr()
                args.a_mean_shift = am_shift.data_ptr()
                args.sample_offset = r * n
                _lib.check(core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 7, 9, None, core.stream()), "covo_mpc_step")
                torch.cuda.synchronize()
                costs.append(core.cost.clone())
                acts.append(core.a.clone())
            assert not torch.equal(costs[0], costs[1])  # the shards drew their own samples
            out = torch.empty(128, device=DEV)
            _lib.check(core.lib.covo_merge_ranks(core.h, _lib.ptr(records), G, _lib.ptr(am_shift), gamma, _lib.ptr(out), None,
                                                 core.stream()), "covo_merge_ranks")
            torch.cuda.synchronize()
            assert torch.equal(am_shift.view(32, 4)[:-1], a_mean0.view(32, 4)[1:])
            cover.add(U.check_update((torch.cat(costs), torch.cat(acts, dim=1)), a_mean0, gamma, lam, out,
                                     where=f"sharded rank records gamma {gamma}"))
            first.setdefault("cost", torch.cat(costs).cpu().numpy().copy())
        assert core.device_status() == 0
        core.close()

    for lam in LAMS:
        run(lam)
    cover.finish(run, first["cost"])
