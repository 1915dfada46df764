"""GPU parity tests (-m gpu): every HIP kernel, called through the C ABI, against the CPU oracle on
the same seeded inputs.  Tolerances (north_star: 1e-5 relative fp32):
  noise GEMM / block-diag   bit-exact vs the oracle's ascending-k fmaf chain
  rollout cost              <= 1e-5 relative (vs fp64 oracle; measured ~2e-6)
  softmax update            <= 1e-5 absolute on a_mean in [-1,1]
  Hessian                   <= 1e-9 absolute vs the fp64 AD oracle
  Sigma / chol(Sigma)       <= 1e-6 relative Frobenius vs fp64 LAPACK
Start states come from two sources: tests/conftest.py::make_problem (level, yaw 0.04 rad, within 5 cm of the target: every test
of this file) and tests/state_atlas.py (yaw octants, near-singular, inverted, tumbling, far / fast, non-unit and negated quaternions:
tests/test_gpu_state_atlas.py runs the same kernels from those).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import EnvParams3D  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from oracle import rng_np  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_cases import _batched_step_equals_replicas, _oracle_check_of_a_fused_step, _run_rollout  # noqa: E402
from tests.gpu_support import DEV, dev_state, sample_actions, to_stripes  # noqa: E402
from tests.oracle_support import oracle_state, rel_err  # noqa: E402
from tests.update_oracle import check_update  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------ RNG
def test_randn_matches_philox_oracle_and_is_shard_invariant():
    core = SamplingCore(4096, 32, 0.01, 1.0, device=DEV)
    z = core.randn((123, 456)).cpu().numpy()
    ref = rng_np.randn(123, 456, 0, 4096, 128)
    assert np.abs(z - ref).max() < 2e-5          # integer stream identical; hardware sin/cos/log vs libm
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    core.offset = 1 << 33                          # ids beyond 32 bits exercise the high counter word
    z2 = core.randn((123, 456)).cpu().numpy()[:64]
    assert np.abs(z2 - rng_np.randn(123, 456, 1 << 33, 64, 128)).max() < 2e-5


def test_randn_jax_equals_the_oracle_twin_and_is_shard_invariant():
    """covo_randn_jax (csrc/rng_jax.hip) against oracle/jax_rng_np.py -- the checker, an independent restatement pinned to jax's
    published outputs (tests/test_oracle.py), not the product's own host twin: the threefry integers are exact, the normals
    agree to the last ulp of log1p / sqrt."""
    from oracle import jax_rng_np as J

    class rj:  # the oracle under the names the body below uses
        controller_epsilon = staticmethod(lambda key, N, sample_offset=0, n_samples=None: J.controller_epsilon(
            key, N, offset=sample_offset, count=n_samples))
        controller_epsilon_mppi = staticmethod(lambda key, N, n_samples=None: J.controller_epsilon_mppi(key, N, count=n_samples))
    N = 1000
    key = J.split(J.prng_key(1))[1]
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV)
    z = core.randn_jax(key).cpu().numpy().copy()
    ref = rj.controller_epsilon(key, N)
    assert np.abs(z - ref).max() < 2e-6 and np.mean(z == ref) > 0.9  # bit-equal except where log1p rounds the other way
    assert abs(z.mean()) < 1e-2 and abs(z.std() - 1) < 1e-2
    zm = core.randn_jax(key, mppi=True).cpu().numpy().copy()
    refm = rj.controller_epsilon_mppi(key, N, n_samples=64)
    assert np.abs(zm[:64] - refm).max() < 2e-6
    assert np.abs(zm - z).max() > 0.1  # the two key trees differ
    # a shard draws exactly its rows of the global matrix (split(act_key, N_global) indexed by global id)
    core.N, core.offset, core.n_local = 4 * N, 3 * N, N
    zs = core.randn_jax(key).cpu().numpy()
    refs = rj.controller_epsilon(key, 4 * N, sample_offset=3 * N, n_samples=32)
    assert np.abs(zs[:32] - refs).max() < 2e-6


# ------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("N", [32, 1000, 8192])
def test_noise_gemm_bit_exact(N):
    rng = np.random.default_rng(N)
    A = rng.normal(size=(128, 128))
    L = np.linalg.cholesky(A @ A.T / 128 + 0.05 * np.eye(128)).astype(np.float32)
    Lfull = L + np.triu(rng.normal(size=(128, 128)).astype(np.float32), 1)  # garbage above the diagonal is ignored
    mu = (0.3 * rng.normal(size=128)).astype(np.float32)
    eps = rng.normal(size=(N, 128)).astype(np.float32)
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV)
    a = core.noise_gemm(torch.from_numpy(Lfull).to(DEV), torch.from_numpy(mu).to(DEV), torch.from_numpy(eps).to(DEV))
    got = a.permute(1, 0, 2).reshape(N, 128).cpu().numpy()
    ref = CO.noise_gemm(L, mu, eps)
    assert np.array_equal(got, ref), f"max diff {np.abs(got - ref).max()}"
    assert (np.abs(got) == 1.0).mean() > 0.001  # the clip is exercised


def test_nan_propagation_flag_in_the_action_clips():
    """COVO_FLAG_PROPAGATE_NAN (SamplingCore(propagate_nan=True)): the clips of covo.py:224 / mppi.py:66 / quadrotor.py:223,258 keep
    a NaN like jnp.clip = minimum(maximum(x, lo), hi); without the flag (the kernels' maxNum / minNum clip) a NaN
    sample becomes -1.  Everything that is not NaN is bit-identical under both settings."""
    rng = np.random.default_rng(4)
    N = 1000
    A = rng.normal(size=(128, 128))
    L = np.linalg.cholesky(A @ A.T / 128 + 0.05 * np.eye(128)).astype(np.float32)
    mu = (0.3 * rng.normal(size=128)).astype(np.float32)
    eps = rng.normal(size=(N, 128)).astype(np.float32)
    L[50, 20] = np.nan                                    # a NaN factor entry (a NaN Sigma row): action 50 of every sample
    mun = mu.copy()
    mun[13] = np.nan                                      # a NaN mean entry: action 13 of EVERY sample
    out = {}
    for flag in (False, True):
        core = SamplingCore(N, 32, 0.01, 1.0, device=DEV, propagate_nan=flag)
        assert core.propagate_nan == flag
        Ld, ed = torch.from_numpy(L).to(DEV), torch.from_numpy(eps).to(DEV)
        a1 = core.noise_gemm(Ld, torch.from_numpy(mu).to(DEV), ed).permute(1, 0, 2).reshape(N, 128).cpu().numpy().copy()
        a2 = core.noise_gemm(Ld, torch.from_numpy(mun).to(DEV), ed).permute(1, 0, 2).reshape(N, 128).cpu().numpy().copy()
        Ls = torch.eye(4, device=DEV).repeat(32, 1, 1) * 0.5
        a3 = core.noise_blockdiag(Ls, torch.from_numpy(mun).to(DEV), ed).permute(1, 0, 2).reshape(N, 128).cpu().numpy().copy()
        out[flag] = (a1, a2, a3)
        # the rollout's own re-clip of stripes it cannot trust (covo_rollout_cost on a handle without COVO_FLAG_ACTIONS_CLIPPED)
        s, p, _ = make_problem(seed=3, time=10)
        acts = sample_actions(p, rng, N)
        acts[5, 3, 2] = np.nan
        cost = _run_rollout(core, s, p, acts, np.zeros(3))
        assert np.isnan(cost[5]) == flag and np.isfinite(np.delete(cost, 5)).all()
    a1f, a2f, a3f = out[False]
    a1t, a2t, a3t = out[True]
    assert np.isfinite(a1f).all() and np.all(a1f[:, 50] == -1.0)            # default: NaN loses against the clip bounds
    assert np.isnan(a1t[:, 50]).all() and np.isfinite(np.delete(a1t, 50, axis=1)).all()   # flag: NaN stays
    assert np.array_equal(np.delete(a1f, 50, axis=1), np.delete(a1t, 50, axis=1))
    assert np.all(a2f[:, 13] == -1.0) and np.isnan(a2t[:, 13]).all() and np.all(a3f[:, 13] == -1.0) and np.isnan(a3t[:, 13]).all()


def test_covo_offline_hovering_nan_row_follows_the_flag():
    """The one place quadjax makes a NaN by itself on this path: covo-offline on `hovering` -- at reset position and
    velocity sit exactly on their targets, JAX's JVP of the norm at 0 is NaN, row 0 of a_cov_offline is NaN (the Hessian
    kernels mirror the convention) and under jnp.clip (covo.py:224) every sample of step 0, hence every later mean, is NaN.
    With propagate_nan=True this library does the same; by default the NaN samples of that one step become -1 and the episode
    carries on."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="hovering", enable_randomizer=False, disturb_type="none", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    params = env.default_params
    res = {}
    for flag in (False, True):
        _, cp0 = cm.envs.get_controller(env, "covo-offline", "N1024_H32_lam0.01", device=DEV)
        c = cm.controllers.CoVOController(env=env, control_params=cp0, N=1024, H=32, lam=0.01, mode="offline", device=DEV,
                                          compute_info=False, propagate_nan=flag)
        obs, info, state = env.reset(cr.PRNGKey(2), params)
        cp = c.reset(state, params, cp0, cr.PRNGKey(3))
        assert torch.isnan(cp.a_cov_offline[0]).any() and torch.isfinite(cp.a_cov_offline[1:]).all()
        key = cr.PRNGKey(4)
        for _ in range(3):
            key, k_act, k_step = cr.split(key, 3)
            u, cp, _ = c(obs, state, params, k_act, cp, info)
            obs, state, reward, done, info = env.step(k_step, state, np.nan_to_num(u.cpu().numpy()), params)
        res[flag] = cp.a_mean.cpu().numpy()
    assert np.isfinite(res[False]).all()
    assert np.isnan(res[True]).all()


def test_device_bus_id_is_a_physical_identity():
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    bus = core.device_bus_id()
    assert len(bus) >= 7 and bus.count(":") >= 1 and bus == SamplingCore(256, 32, 0.01, 1.0, device=DEV).device_bus_id()


def test_in_kernel_philox_equals_randn_then_gemm():
    """The production path draws epsilon inside the noise kernels; it must equal covo_randn -> covo_noise_*
    bit for bit, for any shard offset."""
    rng = np.random.default_rng(9)
    N = 4096 + 17
    A = rng.normal(size=(128, 128))
    L = torch.from_numpy(np.linalg.cholesky(A @ A.T / 128 + 0.05 * np.eye(128)).astype(np.float32)).to(DEV)
    mu = torch.from_numpy((0.3 * rng.normal(size=128)).astype(np.float32)).to(DEV)
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV)
    for off in (0, 12345, 1 << 33):
        core.offset = off
        core.randn((77, 88))
        ref = core.noise_gemm(L, mu).clone()
        got = core.noise_gemm_philox(L, mu, (77, 88))
        assert torch.equal(ref, got), off
        Ls = torch.eye(4, device=DEV).repeat(32, 1, 1) * 0.5
        ref = core.noise_blockdiag(Ls, mu).clone()
        got = core.noise_blockdiag_philox(Ls, mu, (77, 88))
        assert torch.equal(ref, got), off


def test_noise_blockdiag_bit_exact_and_cholesky4():
    rng = np.random.default_rng(5)
    N, H = 777, 32
    cov = np.stack([(lambda B: B @ B.T + 0.1 * np.eye(4))(rng.normal(size=(4, 4))) for _ in range(H)]).astype(np.float32)
    core = SamplingCore(N, H, 0.01, 1.0, device=DEV)
    Ls = core.cholesky(torch.from_numpy(cov).to(DEV), 4, H)
    Ls_ref = np.stack([np.linalg.cholesky(c.astype(np.float64)) for c in cov])
    assert np.abs(Ls.cpu().numpy() - Ls_ref).max() < 1e-6
    mu = (0.3 * rng.normal(size=(H, 4))).astype(np.float32)
    eps = rng.normal(size=(N, H, 4)).astype(np.float32)
    a = core.noise_blockdiag(Ls, torch.from_numpy(mu).to(DEV), torch.from_numpy(eps).to(DEV))
    ref = CO.noise_blockdiag(Ls.cpu().numpy(), mu, eps)
    assert np.array_equal(a.permute(1, 0, 2).cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------ rollout
def test_rollout_golden_fixtures():
    g = np.load(os.path.join(HERE, "golden", "rollout_small.npz"))
    for name in ("mid", "late", "start"):
        st = g[f"{name}_state"]
        s = R.State(pos=st[0:3], vel=st[3:6], quat=st[6:10], omega=st[10:13], f_disturb=st[13:16], pos_tar=st[16:19],
                    vel_tar=st[19:22], acc_tar=np.zeros(3), time=int(g[f"{name}_time"]), pos_traj=g[f"{name}_pos_traj"],
                    vel_traj=g[f"{name}_vel_traj"], acc_traj=np.zeros_like(g[f"{name}_pos_traj"]))
        core = SamplingCore(64, 32, 0.01, float(g[f"{name}_discount"]), device=DEV)
        cost = _run_rollout(core, s, R.Params().fp32(), g[f"{name}_a"], g[f"{name}_f_shared"])
        assert rel_err(cost, g[f"{name}_cost"]).max() < 1e-5, name


@pytest.mark.parametrize("time,seed,N", [(37, 0, 4096), (285, 1, 1000), (0, 2, 300), (330, 3, 257),
                                         (300, 712, 1)])  # one sample: pos_std is exactly 0 at every step
def test_rollout_vs_fp64_oracle(time, seed, N):
    s, p, rng = make_problem(seed=seed, time=time)
    a = sample_actions(p, rng, N)
    fs = np.array([0.01, -0.02, 0.03], dtype=np.float32)
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV)
    cost = _run_rollout(core, s, p, a, fs, want_stats=True)
    ref, rew, poses = CO.rollout(s, p, a.astype(np.float64), 1.0, fs.astype(np.float64), dtype=np.float64,
                                 want_rewards=True, want_poses=True)
    assert rel_err(cost, ref).max() < 1e-5
    # block minima and position statistics (covo.py:281)
    bm = core.blockmin.cpu().numpy()
    assert np.array_equal(bm, np.array([cost[i:i + 64].min() for i in range(0, N, 64)], dtype=np.float32))
    info = core.info(dev_state(s))
    pm, ps = R.pos_stats(poses)
    assert np.abs(info["pos_mean"].cpu().numpy() - pm).max() < 2e-5
    assert np.abs(info["pos_std"].cpu().numpy() - ps).max() < 2e-5


def test_rollout_freeze_and_box_exit():
    s, p, rng = make_problem(seed=7, time=10)
    s = s.replace(pos=s.pos + np.array([2.9, 0, 0]), vel=s.vel + np.array([3.0, 0, 0]))
    a = sample_actions(p, rng, 512)
    core = SamplingCore(512, 32, 0.01, 0.95, device=DEV)
    cost = _run_rollout(core, s, p, a, np.zeros(3))
    ref, rew = CO.rollout(s, p, a.astype(np.float64), 0.95, np.zeros(3), dtype=np.float64, want_rewards=True)
    assert np.any(rew[:, -1] == rew[:, -2])  # frozen rewards present
    assert rel_err(cost, ref).max() < 1e-5


@pytest.mark.parametrize("want_stats", [False, True])
def test_rollout_rollover_termination(want_stats):
    """Quad3D(disable_rollover_terminate=False), the constructor's default: is_terminal also fires on quat[3] < cos(pi/4)
    or |omega| > 100 (quadrotor.py:486-490).  Large body-rate commands tip a good share of the samples over within the
    horizon; the pipelined kernel without and with the position statistics (its STATS variant) against the oracle."""
    s, p, rng = make_problem(seed=31, time=60)
    N = 3000
    a = np.clip(R.hover_action(p, 32, np.float64)[None] + np.array([0.3, 1.5, 1.5, 0.5]) * rng.normal(size=(N, 32, 4)), -1, 1)
    a = a.astype(np.float32)
    core = SamplingCore(N, 32, 0.01, 0.97, device=DEV)
    cost = _run_rollout(core, s, p, a, np.zeros(3), want_stats=want_stats, rollover=True)
    ref, rew = CO.rollout(s, p, a.astype(np.float64), 0.97, np.zeros(3), dtype=np.float64, want_rewards=True, rollover=True)
    ref_off = CO.rollout(s, p, a.astype(np.float64), 0.97, np.zeros(3), dtype=np.float64)
    tipped = np.abs(ref - ref_off) > 1e-3
    assert 0.1 < tipped.mean() < 0.999, tipped.mean()  # the flag matters for many samples, not for all
    # a sample whose quat[3] passes within rounding of cos(pi/4) may freeze one step apart in fp32 and fp64: those few are
    # compared against the neighbouring decisions instead (the oracle run in fp32 takes the fp32 side of the coin)
    ref32 = CO.rollout(s.astype(np.float32), p, a, 0.97, np.zeros(3, np.float32), dtype=np.float32, rollover=True)
    err = np.minimum(rel_err(cost, ref), rel_err(cost, ref32.astype(np.float64)))
    assert (err < 1e-5).mean() > 0.995 and np.median(err) < 2e-6
    off = _run_rollout(core, s, p, a, np.zeros(3), want_stats=want_stats, rollover=False)
    assert rel_err(off, ref_off).max() < 1e-5


def test_rollout_full_size_properties():
    """N = 65536 (BASELINE full size): duplicate / permutation invariance and a sub-sampled oracle check."""
    N = 65536
    s, p, rng = make_problem(seed=11, time=120)
    base = sample_actions(p, rng, N // 2)
    a = np.concatenate([base, base[::-1]], axis=0)  # second half = mirrored copy of the first
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV)
    cost = _run_rollout(core, s, p, a, np.zeros(3))
    assert np.array_equal(cost[:N // 2], cost[N // 2:][::-1])  # same sample -> same bits wherever it sits
    idx = rng.choice(N, 2048, replace=False)
    ref = CO.rollout(s, p, a[idx].astype(np.float64), 1.0, np.zeros(3), dtype=np.float64)
    assert rel_err(cost[idx], ref).max() < 1e-5


@pytest.mark.parametrize("N", [16448, 20000, 40001, 70016, 600000])
def test_rollout_workgroup_shapes(N):
    """The pipelined kernel runs 1, 2 or 4 sample groups per workgroup (rollout.hip: pipe_groups): <= 256 groups -> 1,
    <= 512 -> 2, beyond -> 4 (XCD-affine chunks at N = 65 536: test_rollout_full_size_properties); ragged tails in each."""
    s, p, rng = make_problem(seed=21, time=200)
    a = sample_actions(p, rng, N)
    core = SamplingCore(N, 32, 0.01, 0.99, device=DEV)
    cost = _run_rollout(core, s, p, a, np.array([0.0, 0.01, -0.01]))
    idx = rng.choice(N, 4096, replace=False)
    ref = CO.rollout(s, p, a[idx].astype(np.float64), 0.99, np.array([0.0, 0.01, -0.01]), dtype=np.float64)
    assert rel_err(cost[idx], ref).max() < 1e-5
    gm = core.blockmin.cpu().numpy()
    assert np.array_equal(gm, np.array([cost[i:i + 64].min() for i in range(0, N, 64)], dtype=np.float32))


@pytest.mark.parametrize("N", [1, 33, 63, 65, 129])
def test_tiny_and_ragged_sample_counts(N):
    """Edge sizes: a single sample, partial waves / MFMA tiles / reduce groups.  Whole sampling path (in-kernel Philox
    noise GEMM -> rollout -> softmax update) against the oracle on the materialised epsilon."""
    s, p, rng = make_problem(seed=N, time=150)
    A = rng.normal(size=(128, 128))
    L = np.linalg.cholesky(A @ A.T / 128 + 0.05 * np.eye(128)).astype(np.float32)
    am = (R.hover_action(p, 32, np.float64) + 0.05 * rng.normal(size=(32, 4))).astype(np.float32)
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV)
    core.randn((5, N))
    eps = core.eps.cpu().numpy()
    assert eps.shape == (N, 128) and np.all(np.isfinite(eps))
    core.noise_gemm_philox(torch.from_numpy(L).to(DEV), torch.from_numpy(am.reshape(-1)).to(DEV), (5, N))
    a_dev = core.a.permute(1, 0, 2).contiguous().cpu().numpy()
    a_ref = CO.noise_gemm(L, am.reshape(-1), eps).reshape(N, 32, 4)
    assert np.array_equal(a_dev, a_ref)
    cost = core.rollout(dev_state(s), EnvParams3D().to_c(), (0.0, 0.0, 0.0), False).cpu().numpy()
    ref = CO.rollout(s, p, a_dev.astype(np.float64), 1.0, np.zeros(3), dtype=np.float64)
    assert cost.shape == (N,) and rel_err(cost, ref).max() < 1e-5
    out = core.update(torch.from_numpy(am.reshape(-1)).to(DEV), 1.0).cpu().numpy().reshape(32, 4)
    upd, w = R.softmax_update(ref, a_dev.astype(np.float64), 0.01, 1.0, am.astype(np.float64))
    gap = np.diff(np.sort(ref)[:2])[0] if N > 1 else 1.0
    err = np.abs(out - upd).max()
    print(f"  tiny N={N}: mean vs oracle costs: err {err:.3e}, gap {gap:.3e}, passed by {'err' if err < 1e-4 else 'gap'}")
    assert np.abs(out - upd).max() < 1e-4 or gap < 1e-3
    check_update(core, am, 1.0, 0.01, out, where=f"tiny N={N}", shifted=True)  # the same mean on the device's own costs: no hatch


# ------------------------------------------------------------------------------------------ reduce
@pytest.mark.parametrize("lam,N", [(0.01, 8192), (1.0, 3000), (100.0, 512)])
def test_softmax_update_vs_oracle(lam, N):
    rng = np.random.default_rng(int(lam * 100) + N)
    a = np.clip(0.6 * rng.normal(size=(N, 32, 4)), -1, 1).astype(np.float32)
    cost = (5.0 + rng.normal(size=N) * (3.0 if lam < 1 else 1.0)).astype(np.float32)
    cost[rng.integers(N)] = cost.min() - 0.003  # a clear winner plus close runners-up
    a_mean_old = (0.1 * rng.normal(size=(32, 4))).astype(np.float32)
    core = SamplingCore(N, 32, lam, 1.0, device=DEV)
    core.a.copy_(to_stripes(a))
    core.cost.copy_(torch.from_numpy(cost))
    core.blockmin.copy_(torch.from_numpy(np.array([cost[i:i + 64].min() for i in range(0, N, 64)], dtype=np.float32)))
    for gamma in (1.0, 0.7):
        out = core.update(torch.from_numpy(a_mean_old.reshape(-1)).to(DEV), gamma).cpu().numpy().reshape(32, 4)
        ref, w = R.softmax_update(cost.astype(np.float64), a.astype(np.float64), lam, gamma, a_mean_old.astype(np.float64))
        assert np.abs(out - ref).max() < 1e-5, (lam, gamma, np.abs(out - ref).max())
    # record path + blockmin recomputed internally (blockmin = NULL) + merge of G shard records
    lib = core.lib
    rec = torch.zeros(132, device=DEV)
    _lib.check(lib.covo_softmax_reduce(core.h, _lib.ptr(core.cost), _lib.ptr(core.a), N, None, _lib.ptr(rec), core.stream()))
    m, s_, v = R.softmax_partial(cost.astype(np.float64), a.reshape(N, 128).astype(np.float64), lam)
    r = rec.cpu().numpy()
    assert r[0] == np.float32(m) and abs(r[1] - s_) < 1e-5 * s_ and np.abs(r[2:130] - v).max() < 1e-5 * max(1.0, s_)


def test_merge_shard_invariance_on_device():
    """G in {1,2,4,8} logical shards reduced separately then merged == unsharded."""
    N, lam = 8192, 0.05
    rng = np.random.default_rng(3)
    a = np.clip(0.6 * rng.normal(size=(N, 32, 4)), -1, 1).astype(np.float32)
    cost = (5.0 + 0.2 * rng.normal(size=N)).astype(np.float32)
    am = (0.1 * rng.normal(size=128)).astype(np.float32)
    ref, _ = R.softmax_update(cost.astype(np.float64), a.astype(np.float64), lam, 1.0, am.reshape(32, 4).astype(np.float64))
    outs = []
    for G in (1, 2, 4, 8):
        n = N // G
        core = SamplingCore(n, 32, lam, 1.0, device=DEV)
        recs = torch.zeros((G, 132), device=DEV)
        for g in range(G):
            core.a.copy_(to_stripes(a[g * n:(g + 1) * n]))
            core.cost.copy_(torch.from_numpy(cost[g * n:(g + 1) * n]))
            _lib.check(core.lib.covo_softmax_reduce(core.h, _lib.ptr(core.cost), _lib.ptr(core.a), n, None,
                                                    _lib.ptr(recs[g]), core.stream()))
        out = torch.empty(128, device=DEV)
        _lib.check(core.lib.covo_merge(core.h, _lib.ptr(recs), G, _lib.ptr(torch.from_numpy(am).to(DEV)), 1.0,
                                       _lib.ptr(out), core.stream()))
        outs.append(out.cpu().numpy())
        assert np.abs(outs[-1].reshape(32, 4) - ref).max() < 1e-5, G
    assert max(np.abs(o - outs[0]).max() for o in outs) < 2e-6


def test_shift_mean():
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    x = torch.arange(128, dtype=torch.float32, device=DEV)
    y = core.shift_mean(x).cpu().numpy().reshape(32, 4)
    assert np.array_equal(y, R.shift_mean(np.arange(128, dtype=np.float32).reshape(32, 4)))


# ------------------------------------------------------------------------------------------ Sigma path
@pytest.mark.parametrize("method", ["adjoint", "pairs"])
def test_hessian_vs_ad_oracle(method):
    from oracle import ref_torch as RT
    s, p, rng = make_problem(seed=0, time=37)
    a = (R.hover_action(p, 32, np.float64) + 0.1 * rng.normal(size=(32, 4))).astype(np.float32)
    a[3, 1] = 1.0    # exact clip tie: jnp.clip's JVP passes 0.5 per clip, two clips on the path
    a[5, 2] = -1.0
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    ds = dev_state(s)
    Rm = core.hessian(ds.packed, ds, EnvParams3D().to_c(), torch.from_numpy(a.reshape(-1)).to(DEV),
                      method=method)[0].cpu().numpy()
    ref = RT.hessian(s, p, a.reshape(-1).astype(np.float64), 32)
    assert np.abs(Rm - Rm.T).max() == 0.0 and np.abs(Rm[124:]).max() == 0.0  # KAT 8
    assert np.abs(Rm - ref).max() < 1e-9 * max(1.0, np.abs(ref).max()), np.abs(Rm - ref).max()
    assert np.abs(ref[13]).max() > 0 and np.abs(Rm[13] - ref[13]).max() < 1e-9  # the tie rows are live


@pytest.mark.parametrize("method", ["ns", "jacobi"])
def test_sigma_and_cholesky_vs_lapack(method):
    s, p, rng = make_problem(seed=0, time=37)
    mats = []
    A = rng.normal(size=(128, 128))
    mats.append(0.05 * (A + A.T))                     # generic indefinite
    B = 0.05 * (A + A.T)
    B[124:, :] = 0
    B[:, 124:] = 0
    mats.append(B)                                    # exact 4-dim null space like a real CoVO Hessian
    mats.append(np.eye(128) * 3.0)                    # KAT 7: R = c I -> Sigma = sigma^2 I
    C = 0.05 * (A + A.T)
    w, U = np.linalg.eigh(C)
    w[1] = w[0] + 1e-7                                # near-degenerate bottom pair: lambda_min must stay exact
    w[-1] = w[0] + 40.0                               # wide spectrum: cond(R + delta I) = 4000
    mats.append((U * w) @ U.T)
    Rb = np.stack(mats)
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    Sigma, L = core.sigma(torch.from_numpy(Rb).to(DEV), 0.5, batch=len(mats), method=method)
    Sigma, L = Sigma.cpu().numpy(), L.cpu().numpy()
    for i, Rm in enumerate(mats):
        ref = R.optimize_sigma(Rm, 0.5, 32, 4)
        assert np.linalg.norm(Sigma[i] - ref) / np.linalg.norm(ref) < 1e-6, i
        assert np.array_equal(Sigma[i], Sigma[i].T)
        # L factors the fp64 Sigma (the ns path: L = sqrt(c) chol(Z)) or its fp32 rounding (jacobi path); the two
        # differ by <= cond(Sigma) 2^-24, so: (a) L L^T reproduces a_cov to fp32 rounding, (b) L is close to the
        # exact factor of the rounded matrix
        S64, L64 = Sigma[i].astype(np.float64), L[i].astype(np.float64)
        assert np.linalg.norm(L64 @ L64.T - S64) / np.linalg.norm(S64) < 2e-7, i
        Lref = np.linalg.cholesky(S64)
        assert np.linalg.norm(L[i] - Lref) / np.linalg.norm(Lref) < 3e-6 and np.all(np.triu(L[i], 1) == 0)
    assert np.abs(Sigma[2] - 0.25 * np.eye(128)).max() < 1e-7
    # standalone batched Cholesky at n = 128
    L2 = core.cholesky(torch.from_numpy(Sigma).to(DEV), 128, len(mats)).cpu().numpy()
    assert np.abs(L2 - L).max() < 1e-6


# ------------------------------------------------------------------------------------------ controllers
@pytest.mark.parametrize("name,task,N", [("mppi", "hovering", 1024), ("covo-online", "tracking_zigzag", 2048),
                                         ("covo-offline", "tracking_zigzag", 2048)])
def test_controller_step_teacher_forced(name, task, N):
    """BASELINE configs 1-3 (reduced N): per control step, same epsilon -> cost, Sigma and a_mean parity."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task=task, enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    controller, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    cp = controller.reset(state, params, controller.init_control_params, cr.PRNGKey(2))
    key = cr.PRNGKey(3)
    core = controller.core
    controller.materialize_eps = True  # epsilon is an explicit input of the parity interface
    for step in range(4):
        key, k_act, k_step = cr.split(key, 3)
        ns = info["noisy_state"]
        a_mean_shift = R.shift_mean(cp.a_mean.cpu().numpy().astype(np.float64))
        u, cp_new, cinfo = controller(obs, state, params, k_act, cp, info)
        so = oracle_state(ns)
        eps = core.eps.cpu().numpy()
        a_dev = core.a.permute(1, 0, 2).contiguous().cpu().numpy()
        if name == "mppi":
            a_ref, _ = R.sample_actions_blockdiag(a_mean_shift.astype(np.float32), np.tile(np.eye(4, dtype=np.float32) * 0.25, (32, 1, 1)),
                                                  eps.reshape(N, 32, 4))
            _, k2 = cr.split(k_act)
            _, step_key = cr.split(cr.split(k_act)[0])
            fs = env.rollout_disturbance(step_key, params, deterministic=False)
            assert np.abs(fs).max() > 0
        else:
            Sigma = cp_new.a_cov.cpu().numpy().astype(np.float64)
            if name == "covo-online":
                from oracle import ref_torch as RT
                if step == 3:  # one AD Hessian (9 s on the host) is enough
                    Rm = RT.hessian(so, R.Params().fp32(), a_mean_shift.reshape(-1), 32)
                    Sref = R.optimize_sigma(Rm, 0.5, 32, 4)
                    assert np.linalg.norm(Sigma - Sref) / np.linalg.norm(Sref) < 2e-5
            a_ref, _ = R.sample_actions_full(a_mean_shift.astype(np.float32), Sigma.astype(np.float32), eps)
            fs = np.zeros(3, dtype=np.float32)
        assert np.abs(a_dev - a_ref).max() < 2e-6
        cost_ref = CO.rollout(so, R.Params().fp32(), a_dev.astype(np.float64), 1.0, fs.astype(np.float64), dtype=np.float64)
        assert rel_err(core.cost.cpu().numpy(), cost_ref).max() < 1e-5
        a_new_ref, w = R.softmax_update(cost_ref, a_dev.astype(np.float64), 0.01, 1.0, a_mean_shift)
        gap = np.diff(np.sort(cost_ref)[:2])[0]
        err = np.abs(cp_new.a_mean.cpu().numpy() - a_new_ref).max()
        print(f"  teacher-forced {name} step {step}: mean vs oracle costs: err {err:.3e}, gap {gap:.3e}, passed by {'err' if err < 1e-4 else 'gap'}")
        assert err < 1e-4 or gap < 1e-3, (step, err, gap)
        check_update(core, cp.a_mean, 1.0, 0.01, cp_new.a_mean, where=f"teacher-forced {name} step {step}")
        assert np.array_equal(u.cpu().numpy(), cp_new.a_mean[0].cpu().numpy())
        assert cinfo["pos_mean"].shape == (32, 3) and cinfo["pos_std"].shape == (32, 3)
        cp = cp_new
        obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name,task", [("mppi", "hovering"), ("covo-online", "tracking_zigzag"),
                                       ("covo-offline", "tracking_zigzag")])
def test_fused_step_equals_kernel_by_kernel(name, task, graph, monkeypatch):
    """covo_mpc_step (one C call; eager, or eager once, captured, then replayed as a hipGraph) against the kernel-by-kernel path that
    materialises epsilon, step after step: bit-identical actions, costs, Sigma and info; the means agree to fp32
    rounding (the fused step forms the softmax from per-workgroup records shifted by their LOCAL cost minimum and
    rescaled in the merge, the stand-alone covo_softmax_reduce shifts by the global minimum like covo.py:266)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task=task, enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    N = 4096
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    ca, cpa = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV)
    assert ca.core.uses_graph == (graph == "graph")
    cb, cpb = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV)
    cb.materialize_eps = True
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(4), params)
    cpa = ca.reset(state, params, ca.init_control_params, cr.PRNGKey(5))
    cpb = cb.reset(state, params, cb.init_control_params, cr.PRNGKey(5))
    key = cr.PRNGKey(6)
    for step in range(6):  # call 1 eager, call 2 captures, calls 3+ replay the graph
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        assert (cpa.a_mean - cpb.a_mean).abs().max() <= 2e-6, (name, step, (cpa.a_mean - cpb.a_mean).abs().max())
        assert torch.equal(ca.core.a, cb.core.a)
        assert torch.equal(ca.core.cost, cb.core.cost)
        cpb = cpb.replace(a_mean=cpa.a_mean.clone())  # keep the two runs on the same trajectory bit for bit
        assert torch.allclose(cpa.a_cov, cpb.a_cov, rtol=0, atol=0)
        assert torch.equal(ia["pos_mean"], ib["pos_mean"]) and torch.equal(ia["pos_std"], ib["pos_std"])
        obs, state, reward, done, info = env.step(k_step, state, ua.cpu().numpy(), params)


@pytest.mark.parametrize("name,N,lam", [("covo-online", 1000, "0.01"), ("covo-online", 4096, "1.0"), ("mppi", 100, "0.1"),
                                        ("covo-online", 65, "0.01"),
                                        ("covo-online", 131072, "0.01")])  # > 256 rollout workgroups: stand-alone softmax stage 1
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_fused_step_ragged_sizes_and_warm_lambda(name, N, lam, graph, monkeypatch):
    """The fused step's own kernels at the edges the stand-alone ones are tested on: sample counts that are not a
    multiple of the 32-sample MFMA tile / the 64-lane wave / the 256-sample workgroup (epsilon drawn ahead in tile
    order, softmax records from partial workgroups) and temperatures at which EVERY sample carries weight (the record's
    live-sample loop runs over whole waves).  Against the kernel-by-kernel path: same actions and costs bit for bit,
    means to fp32 rounding."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    ca, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
    cb, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
    cb.materialize_eps = True
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(14), params)
    cpa = ca.reset(state, params, ca.init_control_params, cr.PRNGKey(5))
    cpb = cb.reset(state, params, cb.init_control_params, cr.PRNGKey(5))
    key = cr.PRNGKey(16)
    for step in range(4):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, _ = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, _ = cb(obs, state, params, k_act, cpb, info)
        assert torch.equal(ca.core.a, cb.core.a), (name, N, step)
        assert torch.equal(ca.core.cost, cb.core.cost), (name, N, step)
        assert (cpa.a_mean - cpb.a_mean).abs().max() <= 5e-6, (name, N, step, (cpa.a_mean - cpb.a_mean).abs().max())
        if name == "covo-online":
            # the fused step leaves a_cov to the noise GEMM's first workgroups (64 of them from N = 16 384 on, striding ones
            # below), the kernel-by-kernel path to the chain's finalize launch: same expression, same bits
            assert torch.equal(cpa.a_cov, cpb.a_cov), (name, N, step)
        cpb = cpb.replace(a_mean=cpa.a_mean.clone())
        obs, state, reward, done, info = env.step(k_step, state, ua.cpu().numpy(), params)


def test_env_instances_with_domain_randomisation():
    """BASELINE configs[4] (reduced: 4 of the 256 instances, N = 4096): independent env instances of the lissajous
    `tracking` task, each with its own domain-randomised parameters (quadrotor.py:135-160), each its own complete
    covo-online MPC problem ("replicas only").  Per instance: cost trajectories against the fp64
    oracle run with THAT instance's parameters, and the instances really differ."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    N, E = 4096, 4
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    masses, means = [], []
    for e in range(E):
        params = env.sample_params(cr.PRNGKey(100 + e))
        masses.append(float(params.m))
        controller, cp = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV)
        controller.materialize_eps = True
        obs, info, state = env.reset(cr.PRNGKey(200 + e), params)
        cp = controller.reset(state, params, controller.init_control_params, cr.PRNGKey(2))
        key = cr.PRNGKey(300 + e)
        po = R.Params(m=float(params.m), action_scale=float(params.action_scale),
                      alpha_bodyrate=float(params.alpha_bodyrate)).fp32()
        for step in range(3):
            key, k_act, k_step = cr.split(key, 3)
            so = oracle_state(info["noisy_state"])
            u, cp, _ = controller(obs, state, params, k_act, cp, info)
            a_dev = controller.core.a.permute(1, 0, 2).contiguous().cpu().numpy()
            cost_ref = CO.rollout(so, po, a_dev.astype(np.float64), 1.0, np.zeros(3), dtype=np.float64)
            assert rel_err(controller.core.cost.cpu().numpy(), cost_ref).max() < 1e-5, (e, step)
            obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
        means.append(cp.a_mean.cpu().numpy())
    assert np.ptp(masses) > 1e-4                       # the instances are different plants ...
    assert np.abs(means[0] - means[1]).max() > 1e-4    # ... and get different plans


def test_batched_step_equals_replicas():
    """BASELINE configs[4] reduced to 3 instances, N = 4096, five steps."""
    _batched_step_equals_replicas(4096, 3, 5)


def core_scalars(core, batch, count=24):
    """the first `count` scalars of matrix 0 of the Sigma chain's workspace after a covo_sigma call on `batch` matrices"""
    from covo_mpc_amd import _lib
    out = torch.zeros(count, dtype=torch.float64, device=DEV)
    _lib.check(core.lib.covo_debug_sigma_workspace(core.h, _lib.ptr(out), 11 * batch * 128 * 128, count, core.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_sigma_persistent_plans_equal_phased_plan():
    """The Sigma chain's squarings and Newton-Schulz iterations run inside persistent launches whose phases are separated by
    barriers inside the launch (sigma_ns.hip: ns_square_tail_pair_kernel, ns_iter_tail_pair_kernel; all workgroups of a matrix on one
    XCD, sc1 loads, plain stores once the placement is verified).  The phased plan -- every phase its own launch, what a
    COVO_FLAG_SHARED_DEVICE handle runs -- must give the same Sigma and L bit for bit, for one matrix and for a batch (every matrix
    of a batched launch runs its tail at its own pace; 11 matrices: XCDs with one and with two of them)."""
    from covo_mpc_amd import _lib
    lib = _lib.load_library()
    rng = np.random.default_rng(5)
    n = 128
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    mats = []
    G = rng.standard_normal((n, n)); mats.append(0.05 * (G + G.T))                                   # ~8 iterations
    w = np.concatenate([np.abs(rng.standard_normal(20)) * 50, rng.standard_normal(108) * 0.05]); mats.append((Q * w) @ Q.T)
    w = np.concatenate([[-2.0, -1.1, -0.7], np.geomspace(0.01, 900.0, n - 3)]); mats.append((Q * w) @ Q.T)  # closed-loop-like
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    phased = SamplingCore(256, 32, 0.01, 1.0, device=DEV, shared_device=True)
    try:
        for Rm in mats:
            R_d = torch.from_numpy(np.ascontiguousarray(Rm)).to(DEV)
            outs = []
            for c in (phased, core):
                Sig, L = c.sigma(R_d[None], 0.5)
                outs.append((Sig.clone(), L.clone()))
            assert torch.isfinite(outs[0][0]).all()
            for Sig, L in outs[1:]:
                assert torch.equal(Sig, outs[0][0]) and torch.equal(L, outs[0][1])
        # a batch: the three matrices and scaled / shifted copies, 11 in all
        batch = [mats[i % 3] * (1.0 + 0.25 * (i // 3)) + 0.1 * (i // 3) * np.eye(n) for i in range(11)]
        R_b = torch.from_numpy(np.ascontiguousarray(np.stack(batch))).to(DEV)
        outs = []
        for c in (phased, core):
            Sig, L = c.sigma(R_b, 0.5, batch=11)
            outs.append((Sig.clone(), L.clone()))
        assert torch.isfinite(outs[0][0]).all()
        for Sig, L in outs[1:]:
            assert torch.equal(Sig, outs[0][0]) and torch.equal(L, outs[0][1])
        for i in range(3):  # and a matrix of a batch equals the same matrix alone
            Sig1, L1 = core.sigma(R_b[i:i + 1].contiguous(), 0.5)
            assert torch.equal(Sig1[0], outs[0][0][i]) and torch.equal(L1[0], outs[0][1][i])
        # the placement check's fallback (workgroups of a launch NOT on one XCD: every access stays an agent-scope atomic), which no
        # MI355X box takes by itself: forced, one matrix and the batch
        tail_modes = lambda b: core_scalars(core, b)[21:23]
        Sig_x, L_x = core.sigma(R_b[:1].contiguous(), 0.5)
        assert list(tail_modes(1)) == [2.0, 2.0], tail_modes(1)  # both persistent launches found themselves on one XCD
        _lib.check(lib.covo_debug_set_ns_coherence(core.h, 1))
        Sig_a, L_a = core.sigma(R_b[:1].contiguous(), 0.5)
        assert list(tail_modes(1)) == [1.0, 1.0], tail_modes(1)
        assert torch.equal(Sig_a, Sig_x) and torch.equal(L_a, L_x)
        Sig_a, L_a = core.sigma(R_b, 0.5, batch=11)
        assert torch.equal(Sig_a, outs[0][0]) and torch.equal(L_a, outs[0][1])
    finally:
        _lib.check(lib.covo_debug_set_ns_coherence(core.h, 0))


def test_batched_step_single_instance_and_errors():
    """covo_mpc_step_batched at its edges: one instance (no batching to hide behind) equals the plain controller bit for
    bit; more instances than COVO_MAX_ENVS, and a call before the instances are bound, fail loudly."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    N = 2048
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    params = env.sample_params(cr.PRNGKey(7))
    controller, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    obs, info, state = env.reset(cr.PRNGKey(8), params)
    cp = controller.reset(state, params, controller.init_control_params, cr.PRNGKey(2))
    b = cm.controllers.BatchedCoVOController(env, 1, N, 32, 0.01, discount=cp.discount, gamma_mean=cp.gamma_mean,
                                             sample_sigma=cp.sample_sigma, a_mean_init=cp.a_mean, device=DEV)
    with pytest.raises(RuntimeError):
        b([info["noisy_state"]], np.zeros((1, 2), dtype=np.uint32))
    b.set_instances([state], [params])
    key = cr.PRNGKey(9)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        u_b = b([info["noisy_state"]], np.asarray(k_act)[None]).clone()
        u, cp, _ = controller(obs, state, params, k_act, cp, info)
        assert torch.equal(u_b[0], u) and torch.equal(b.a_mean[0].view(32, 4), cp.a_mean) and torch.equal(b.a_cov[0], cp.a_cov)
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    with pytest.raises(ValueError):
        cm.controllers.BatchedCoVOController(env, 65, N, 32, 0.01, device=DEV)


def test_closed_loop_tracking_sanity():
    """Free-running covo-offline on tracking_zigzag: tracking error stays at the few-cm level after the
    start-up transient."""
    import covo_mpc_amd as cm
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    controller, _ = cm.envs.get_controller(env, "mppi", "N4096_H32_lam0.01", device=DEV, compute_info=False)
    err = cm.envs.eval_env(env, controller, total_steps=300, num_trajs=1, save=False, verbose=False)
    assert err[0] < 0.15, err


def test_offline_nominal_trajectory_device_vs_host():
    """covo-offline reset (covo.py:58-99): the device kernels (covo_pid_nominal: PID law pid.py:38-84 + env steps, keys
    split on the device) against the Python env + PID loop: the 300 start states and their 32-step nominal means."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    controller, cp = cm.envs.get_controller(env, "covo-offline", "N1024_H32_lam0.01", device=DEV)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(31), params)
    ph, ah = controller._nominal_host(state, params, cr.PRNGKey(32))
    pd, ad, _ = controller._nominal_device(state, params, cr.PRNGKey(32))
    pd, ad = pd.cpu().numpy(), ad.cpu().numpy()
    assert np.array_equal(pd[:, 25].view(np.int32), ph[:, 25].view(np.int32))      # time
    assert np.abs(pd[:, :25] - ph[:, :25]).max() < 5e-5, np.abs(pd[:, :25] - ph[:, :25]).max()
    assert np.abs(ad - ah).max() < 2e-4, np.abs(ad - ah).max()
    assert np.abs(ph[:, 13:16]).max() > 0  # the chain really draws disturbances


def test_env_step_kernel_vs_host_env():
    """covo_env_step (device) against the Python env (the restatement of quadrotor.py:215-263,314-361
    + free.py:114-202) on the same keys and the same action sequence: true state, noisy state, reward, err_pos, done."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    params = env.default_params
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(11), params, (core.lib, core.h), DEV)
    obs, info, state = env.reset(cr.PRNGKey(11), params)
    assert np.array_equal(ep.true.cpu().numpy(), state.pack()) and np.array_equal(ep.noisy.cpu().numpy(), info["noisy_state"].pack())
    rng = np.random.default_rng(5)
    key = cr.PRNGKey(12)
    rewards, errs = [], []
    for t in range(60):
        key, k_step = cr.split(key)
        u = np.clip(np.array([-0.3378, 0, 0, 0]) + 0.3 * rng.normal(size=4), -1.2, 1.2).astype(np.float32)  # also exercises the clip
        ep.step(k_step, torch.from_numpy(u).to(DEV))
        obs, state, reward, done, info = env.step(k_step, state, u, params)
        rewards.append(reward)
        errs.append(info["err_pos"])
        t_dev, n_dev = ep.true.cpu().numpy(), ep.noisy.cpu().numpy()
        assert np.abs(t_dev - state.pack()).max() < 2e-5, (t, np.abs(t_dev - state.pack()).max())
        assert t_dev[25:26].view(np.int32)[0] == state.time
        assert np.abs(n_dev - info["noisy_state"].pack()).max() < 2e-5, t
        # the noise itself is bit-exact: noisy - true on the device = the env's (z * scale) * c added to the DEVICE's true state
        f32 = np.float32
        kp, kv, kq, ko = cr.split(cr.split(cr.split(k_step)[0])[0], 5)[:4]   # base.py:22 -> step_env's info_key -> get_info's four keys
        s_ = f32(params.obs_noise_scale)
        for sl, kk, n_, c_ in ((slice(0, 3), kp, 3, 0.25), (slice(3, 6), kv, 3, 0.5), (slice(6, 10), kq, 4, 0.02), (slice(10, 13), ko, 3, 0.5)):
            want = (t_dev[sl] + cr.normal(kk, (n_,)) * s_ * f32(c_)).astype(f32)
            assert np.array_equal(n_dev[sl], want), (t, sl)
    log = ep.read_log()
    assert log.shape == (60, 4) and np.all(log[:, 3] == 0)
    assert np.abs(log[:, 0] - np.asarray(rewards)).max() < 2e-5 and np.abs(log[:, 1] - np.asarray(errs)).max() < 2e-5


@pytest.mark.parametrize("name", ["mppi", "covo-online", "covo-offline"])
def test_run_episode_equals_python_loop(name):
    """covo_run_episode (one C call enqueues n x {fused step, env step}, host Philox splits in C) must reproduce the
    Python loop over controller.__call__ + DeviceEpisode.step bit for bit: same log, same final mean, same rng."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    task = "hovering" if name == "mppi" else "tracking_zigzag"
    env = cm.envs.Quad3D(task=task, enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    params = env.default_params
    n = 24
    outs = []
    for fused in (False, True):
        controller, _ = cm.envs.get_controller(env, name, "N2048_H32_lam0.01", device=DEV, compute_info=False)
        controller.alias_outputs = True
        core = controller.core
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (core.lib, core.h), DEV)
        cp = controller.reset(ep.state0, params, controller.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if fused:
            cp, rng = controller.run_episode(ep, params, cp, rng, n)
        else:
            for _ in range(n):  # eval_env's run_one_step (quadrotor.py:520-538)
                rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
                u, cp, _ = controller(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                ep.step(rng_step, u)
                rng, rng_control = cr.split(rng)
        outs.append((ep.read_log().copy(), cp.a_mean.cpu().numpy().copy(), ep.true.cpu().numpy().copy(), np.asarray(rng).copy()))
    assert np.array_equal(outs[0][3], outs[1][3])
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert outs[0][0].shape == (n, 4) and np.any(outs[0][0][:, 1] > 0)


def test_closed_loop_on_device():
    """The eval protocol with the env step on the device (one sync per episode): tracking error at the same few-cm
    level as the host-driven loop."""
    import covo_mpc_amd as cm
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    controller, _ = cm.envs.get_controller(env, "covo-online", "N4096_H32_lam0.01", device=DEV, compute_info=False)
    err = cm.envs.eval_env_device(env, controller, total_steps=300, num_trajs=1, verbose=False)
    assert err.shape == (1,) and err[0] < 0.15, err


@pytest.mark.parametrize("name,exchange", [("covo-online", "collective"), ("covo-online", "peer"), ("mppi", "collective"),
                                           ("mppi", "peer"), ("covo-online", "auto"), ("mppi", "auto_fail"),
                                           ("mppi-cov", "collective"), ("mppi-cov", "peer"), ("mppi", "auto_coarse"),
                                           ("mppi-cov0", "collective")])
def test_two_ranks_one_gpu(name, exchange):
    """SURVEY.md 8e through the PRODUCT path: two processes (gloo rendezvous, both on cuda:0) run the sample-sharded
    controller -- fused step writing this shard's rank record (softmax partial + position sums), ONE exchange (all-gather, or
    csrc/exchange.hip's peer writes into hipIpc-mapped buffers), device merge -- and each checks it against the unsharded
    controller on the same keys; with the peer exchange also a sharded episode segment enqueued from C (tests/_dist_gpu_worker.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "_dist_gpu_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29541", script, name, exchange],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "DIST_GPU_OK" in r.stdout


@pytest.mark.parametrize("name", ["covo-online", "mppi-cov"])
def test_two_ranks_two_gpus_rccl(name):
    """The nccl (= RCCL) branch of exchange_records and one GPU per rank: only where the box has two GPUs (the build pool's boxes
    have one: skipped there, so the leg stays 'unexercised on this pool' rather than silently untested on a multi-GPU box)."""
    import os
    import subprocess
    import sys
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL over xGMI)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "_dist_gpu_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", script, name, "collective", "nccl"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "DIST_GPU_OK" in r.stdout


def test_device_status_is_sticky_and_refuses_further_work():
    """A kernel-side failure (the Sigma chain's grid barrier timing out on a shared GPU) must not stay silent: it raises a
    bit in host-mapped memory, the next compute call on the handle returns COVO_E_DEVICE, clearing re-arms the handle."""
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    assert core.device_status() == 0
    A = np.random.default_rng(0).normal(size=(128, 128))
    Rm = torch.from_numpy(0.05 * (A + A.T)).to(DEV).reshape(1, 128, 128)
    core.sigma(Rm, 0.5)
    _lib.check(core.lib.covo_debug_raise_device_status(core.h, _lib.COVO_DEVSTAT_GRID_BARRIER, core.stream()), "raise")
    torch.cuda.synchronize()
    assert core.device_status() == _lib.COVO_DEVSTAT_GRID_BARRIER
    with pytest.raises(_lib.CovoError, match="grid barrier"):
        core.sigma(Rm, 0.5)
    with pytest.raises(_lib.CovoError, match="device status"):
        core.noise_gemm_philox(torch.eye(128, device=DEV), torch.zeros(128, device=DEV), (1, 2))
    assert core.device_status(clear=True) == _lib.COVO_DEVSTAT_GRID_BARRIER and core.device_status() == 0
    S2, L2 = core.sigma(Rm, 0.5)
    assert torch.isfinite(S2).all() and torch.isfinite(L2).all()
    # the adjoint Hessian's costate wait raises its own bit on a time-out (round 4): same contract
    _lib.check(core.lib.covo_debug_raise_device_status(core.h, _lib.COVO_DEVSTAT_ADJOINT, core.stream()), "raise")
    torch.cuda.synchronize()
    with pytest.raises(_lib.CovoError, match="adjoint"):
        core.sigma(Rm, 0.5)
    assert core.device_status(clear=True) == _lib.COVO_DEVSTAT_ADJOINT


def test_shared_device_flag_runs_the_chain_phase_by_phase_with_identical_results():
    """COVO_FLAG_SHARED_DEVICE: no persistent launches (grid barriers) in the Sigma chain; same Sigma and L bit for bit."""
    rng = np.random.default_rng(3)
    A = rng.normal(size=(128, 128))
    Rm = torch.from_numpy(0.5 * (A + A.T) + np.diag(rng.uniform(0, 30, 128))).to(DEV).reshape(1, 128, 128)
    c0 = SamplingCore(64, 32, 0.01, 1.0, device=DEV)
    c1 = SamplingCore(64, 32, 0.01, 1.0, device=DEV, shared_device=True)
    S0, L0 = c0.sigma(Rm, 0.5)
    S1, L1 = c1.sigma(Rm, 0.5)
    assert torch.equal(S0, S1) and torch.equal(L0, L1) and torch.isfinite(S0).all()
    # a batch (the env-batched step, covo-offline's table): per-matrix persistent launches against one-tile squaring launches +
    # the 2 x 2-block launches of the iterations -- and row 0 of the batch against the single matrix
    Rb = torch.cat([Rm * (1.0 + 0.5 * i) + 0.3 * i * torch.eye(128, dtype=Rm.dtype, device=Rm.device) for i in range(13)]).contiguous()
    Sb0, Lb0 = c0.sigma(Rb, 0.5, batch=13)
    Sb1, Lb1 = c1.sigma(Rb, 0.5, batch=13)
    assert torch.equal(Sb0, Sb1) and torch.equal(Lb0, Lb1) and torch.isfinite(Sb0).all()
    assert torch.equal(Sb0[0], S0[0]) and torch.equal(Lb0[0], L0[0])


def test_workspace_growth_drops_the_captured_step_graph(monkeypatch):
    """A captured covo_mpc_step graph holds the Sigma / Hessian workspace addresses; a later larger-batch covo_sigma /
    covo_hessian re-allocates them.  The handle must re-capture instead of replaying launches into freed memory."""
    monkeypatch.setenv("COVO_GRAPH", "1")
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    params = env.default_params
    cg, cpg = cm.envs.get_controller(env, "covo-online", "N1024_H32_lam0.01", device=DEV)
    monkeypatch.setenv("COVO_GRAPH", "0")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    ce, cpe = cm.envs.get_controller(env, "covo-online", "N1024_H32_lam0.01", device=DEV)
    assert cg.core.uses_graph and not ce.core.uses_graph
    obs, info, state = env.reset(cr.PRNGKey(2), params)
    key = cr.PRNGKey(9)
    rng = np.random.default_rng(1)
    for step in range(7):
        key, k_act, k_step = cr.split(key, 3)
        ug, cpg, _ = cg(obs, state, params, k_act, cpg, info)
        ue, cpe, _ = ce(obs, state, params, k_act, cpe, info)
        assert torch.equal(cpg.a_mean, cpe.a_mean) and torch.equal(cpg.a_cov, cpe.a_cov), step
        if step == 3:  # graph captured at step 1, replayed since: now grow both workspaces under it
            A = rng.normal(size=(5, 128, 128))
            Rb = torch.from_numpy(0.05 * (A + np.transpose(A, (0, 2, 1)))).to(DEV)
            S, L = cg.core.sigma(Rb, 0.5, batch=5)
            assert torch.isfinite(S).all()
            ds = info["noisy_state"].to_device(DEV)
            Hs = cg.core.hessian(ds.packed.repeat(5), ds, params.to_c(), cpg.a_mean.reshape(-1).repeat(5), batch=5)
            assert torch.isfinite(Hs).all()
        obs, state, reward, done, info = env.step(k_step, state, ue.cpu().numpy(), params)


@pytest.mark.parametrize("name,task", [("covo-online", "tracking_zigzag"), ("mppi", "hovering")])
def test_controller_step_on_the_jax_bitstream(name, task):
    """noise_stream = "jax": the controller splits its key and draws epsilon exactly as quadjax does on jax.random
    (covo.py:212-220 / mppi.py:53-60); the step then equals the oracle's on that epsilon, and differs from the Philox run."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    from oracle import jax_rng_np as J  # the checker of the jax stream: the oracle's restatement, not the product's twin

    class rj:
        PRNGKey = staticmethod(J.prng_key)
        split = staticmethod(J.split)
        controller_epsilon = staticmethod(J.controller_epsilon)
        controller_epsilon_mppi = staticmethod(J.controller_epsilon_mppi)
    N = 512
    env = cm.envs.Quad3D(task=task, enable_randomizer=False, disturb_type="none", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    params = env.default_params
    c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV)
    c.noise_stream = "jax"
    obs, info, state = env.reset(cr.PRNGKey(3), params)
    rng_act = rj.PRNGKey(11)
    u, cp2, _ = c(obs, state, params, rng_act, cp, info)
    eps = c.core.eps.cpu().numpy()
    act_key = rj.split(rng_act)[1]
    ref = rj.controller_epsilon(act_key, N) if name != "mppi" else rj.controller_epsilon_mppi(act_key, N)
    assert np.abs(eps - ref).max() < 2e-6
    a_dev = c.core.a.permute(1, 0, 2).contiguous().cpu().numpy()
    am = R.shift_mean(cp.a_mean.cpu().numpy().astype(np.float64))
    if name == "mppi":
        a_ref, _ = R.sample_actions_blockdiag(am, np.tile(np.eye(4) * 0.25, (32, 1, 1)), ref.reshape(N, 32, 4).astype(np.float64))
    else:
        a_ref, _ = R.sample_actions_full(am, cp2.a_cov.cpu().numpy().astype(np.float64), ref.astype(np.float64))
    assert np.abs(a_dev - a_ref).max() < 2e-5
    assert np.all(np.isfinite(cp2.a_mean.cpu().numpy())) and abs(float(u[0])) <= 1.0
    c.noise_stream = "philox"
    c.materialize_eps = True
    c(obs, state, params, rng_act, cp, info)
    assert np.abs(c.core.eps.cpu().numpy() - eps).max() > 0.5


def test_errors_are_reported_through_the_abi():
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    with pytest.raises(_lib.CovoError):
        _lib.check(core.lib.covo_shift_mean(core.h, _lib.ptr(core.cost), _lib.ptr(core.cost), core.stream()), "shift")
    with pytest.raises(NotImplementedError):
        SamplingCore(256, 16, 0.01, 1.0, device=DEV)
    cfg = _lib.ConfigC(0, 32, 4, 0.01, 1.0, 0)
    h = C.c_void_p()
    assert core.lib.covo_create(C.byref(cfg), C.byref(h)) == -1 and b"n_local" in core.lib.covo_last_error()


def _sigma_chain_iters(core):
    """(squarings, Newton-Schulz iterations, deflated?) of the LAST batch-1 covo_sigma call, from the chain's scalar slots"""
    out = torch.zeros(32, dtype=torch.float64, device=DEV)
    _lib.check(core.lib.covo_debug_sigma_workspace(core.h, _lib.ptr(out), 11 * 128 * 128, 32, core.stream()))
    o = out.cpu().numpy()
    return int(o[7]), int(o[6]), bool(o[29] != 0.0)  # SC_KWIN, SC_ITERS, SC_GAM


def test_sigma_early_ritz_equals_scan_equals_batch():
    """lambda_min is the Ritz value of X_kwin, kwin = the first filter iterate whose bottom Ritz pair passes its own residual
    test (sigma_ns.hip: ritz_eval / ritz_decide) -- a function of the matrix alone.  The evaluations riding inside the
    squaring launch (one matrix), the scan launch after squarings that run to their own stop (a shared-device handle: the phased
    plan) and the batched chain give the same Sigma and L bit for bit; on real Hessians kwin comes well before the filter's own stop."""
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    mats = [m for k in g.files for m in g[k]]
    n_real = len(mats)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(128, 128))
    w, U = np.linalg.eigh(0.05 * (A + A.T))
    for w01 in (1e-9, 1e-3, 3.0):
        ww = w.copy()
        ww[0] = ww[1] - w01
        mats.append((U * ww) @ U.T)
    mats.append(np.load(os.path.join(HERE, "golden", "sigma_nullblock_small_lmin.npy")))
    mats.append(np.eye(128))
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    scan = SamplingCore(256, 32, 0.01, 1.0, device=DEV, shared_device=True)
    out = torch.zeros(32, dtype=torch.float64, device=DEV)
    res, kwin, ksq = {}, [], []
    for inside, c in ((1, core), (0, scan)):
        for i, Rm in enumerate(mats):
            Sigma, L = c.sigma(torch.from_numpy(Rm[None].copy()).to(DEV), 0.5)
            res[inside, i] = (Sigma[0].cpu().numpy(), L[0].cpu().numpy())
            _lib.check(c.lib.covo_debug_sigma_workspace(c.h, _lib.ptr(out), 11 * 128 * 128, 32, c.stream()))
            o = out.cpu().numpy()
            assert o[26] == 0.0, (inside, i)  # SC_BARFAIL
            if inside == 0:  # the scan path runs the filter to its own stop: SC_KWIN against SC_SQ
                kwin.append(int(o[7]))
                ksq.append(int(o[8]))
                assert 2 <= o[7] <= o[8] <= 16, (i, o[7], o[8])
            ref = R.optimize_sigma(Rm, 0.5, 32, 4)
            assert np.linalg.norm(res[inside, i][0] - ref) / np.linalg.norm(ref) < 1e-6, (inside, i)
    for i in range(len(mats)):
        assert np.array_equal(res[1, i][0], res[0, i][0]) and np.array_equal(res[1, i][1], res[0, i][1]), i
    kwin, ksq = np.array(kwin), np.array(ksq)
    assert np.mean(ksq[:n_real] - kwin[:n_real]) >= 1.5, (kwin, ksq)  # real Hessians: the pair is there ~2.5 squarings early
    Sb, Lb = core.sigma(torch.from_numpy(np.stack(mats)).to(DEV), 0.5, batch=len(mats))
    for i in range(len(mats)):
        assert np.array_equal(Sb[i].cpu().numpy(), res[1, i][0]) and np.array_equal(Lb[i].cpu().numpy(), res[1, i][1]), i


def test_sigma_deflation_on_real_hessians():
    """The deflated Newton-Schulz chain (sigma_ns.hip: bottom eigenpair moved into the spectrum, put back at the end) on
    Hessians of closed-loop and teacher-forced episodes (tests/golden/hessians_r03.npz: dumped by scripts/dump_hessians.py from
    this build's Hessian kernel) and on synthetic spectra: Sigma <= 1e-6 of LAPACK eigh with and without it, fewer iterations
    with it, and the cases it must decline (degenerate bottom, isolated bottom far below, identity)."""
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    mats = [m for k in g.files for m in g[k]]
    rng = np.random.default_rng(4)
    A = rng.normal(size=(128, 128))
    w, U = np.linalg.eigh(0.05 * (A + A.T))
    for w01 in (1e-9, 1e-3, 0.05, 3.0):  # bottom gap from degenerate to isolated
        ww = w.copy()
        ww[0] = ww[1] - w01
        mats.append((U * ww) @ U.T)
    ww = w.copy()
    ww[-1] = ww[0] + 4000.0  # cond 4e5 before deflation
    mats.append((U * ww) @ U.T)
    # found by scripts/fuzz_parity.py (seed 3): lambda_min = -0.015 next to the four exact zeros of the null block, width 1.7e3 --
    # round 2's chain reported lambda_min = 0 (the null rows' unit vectors took all Ritz picks after 13 squarings) and returned NaN
    mats.append(np.load(os.path.join(HERE, "golden", "sigma_nullblock_small_lmin.npy")))
    Z = np.zeros((128, 128))
    Z[:120, :120] = (lambda B: B @ B.T / 120 + 0.3 * np.eye(120))(rng.normal(size=(120, 120)))  # PSD with an 8-dim null block: lambda_min = 0 exactly
    mats.append(Z)
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    saved, n_defl = [], 0
    try:
        for i, Rm in enumerate(mats):
            ref = R.optimize_sigma(Rm, 0.5, 32, 4)
            res = {}
            for on in (1, 0):
                _lib.check(core.lib.covo_debug_set_ns_deflate(core.h, on))
                Sigma, L = core.sigma(torch.from_numpy(Rm[None].copy()).to(DEV), 0.5)
                Sigma, L = Sigma[0].cpu().numpy(), L[0].cpu().numpy().astype(np.float64)
                err = np.linalg.norm(Sigma - ref) / np.linalg.norm(ref)
                assert err < 1e-6, (i, on, err)
                assert np.array_equal(Sigma, Sigma.T)
                assert np.linalg.norm(L @ L.T - Sigma) / np.linalg.norm(Sigma) < 2e-7, (i, on)
                res[on] = _sigma_chain_iters(core)
            assert res[0][2] is False and res[1][1] <= res[0][1], (i, res)
            if i < len(mats) - 7:  # the real Hessians: deflated, and it pays
                assert res[1][2], (i, res)
                saved.append(res[0][1] - res[1][1])
            n_defl += res[1][2]
    finally:
        _lib.check(core.lib.covo_debug_set_ns_deflate(core.h, 1))
    assert np.mean(saved) >= 1.5, saved
    # batched (covo-offline's table path): same matrices in one call, per-matrix deflation state
    Rb = np.stack(mats)
    Sb, Lb = core.sigma(torch.from_numpy(Rb).to(DEV), 0.5, batch=len(mats))
    for i, Rm in enumerate(mats):
        ref = R.optimize_sigma(Rm, 0.5, 32, 4)
        assert np.linalg.norm(Sb[i].cpu().numpy() - ref) / np.linalg.norm(ref) < 1e-6, i


@pytest.mark.parametrize("config", ["samples", "envs"])
def test_bench_multi_rank_path_rehearsal(config):
    """bench.py's N > 1 path (rendezvous on 127.0.0.1, sharding, barrier + max-over-ranks timing, rank-0 JSON line) with two ranks
    SHARING this box's one GPU over gloo (COVO_BENCH_BACKEND=gloo: functional rehearsal only -- the product backend is nccl = RCCL,
    one rank per GPU, which this pool cannot run).  samples: N sharded, one exchange of the rank records per step ("strong");
    envs: BASELINE configs[4], env instances sharded, no collective on the data path ("weak")."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = "29551" if config == "samples" else "29553"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, PYTHONPATH=root, COVO_BENCH_BACKEND="gloo",
               COVO_SHARED_DEVICE="1")
    extra = ["--N", "2048"] if config == "samples" else ["--config", "envs", "--envs-per-gpu", "2", "--N", "1024"]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", port, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4",
                        "--warmup", "2", "--no-closed-loop", "--no-cpu-baseline", "--no-info-leg"] + extra,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # ONE line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 0 and d["metric"] == "mpc_control_steps_per_sec"
    if config == "samples":
        assert d["scaling"] == "strong" and d["config"]["N_local"] == 1024 and "collective" in d["config"]["workload"]
    else:
        assert d["scaling"] == "weak" and d["config"]["envs_total"] == 4 and "no collective" in d["config"]["workload"]


def test_bench_gpus_2_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no torchrun environment (the driver's 1-GPU command shape): the parent launches the two
    ranks itself and relays ONE line with n_gpus = 2 (here the ranks share this box's GPU over gloo: functional only)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONPATH=root, COVO_BENCH_BACKEND="gloo", COVO_SHARED_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--N", "2048",
                        "--no-closed-loop", "--no-cpu-baseline", "--no-info-leg"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["N_local"] == 1024 and d["value"] > 0
    assert d["config"]["timed_episode_steps"] == [37, 112, 187, 262]  # spread over the controller's own 300-step episode


@pytest.mark.parametrize("name,N,lam", [("covo-offline", 8192, "0.01"), ("covo-offline", 1000, "0.5"), ("covo-offline", 16384, "0.01"),
                                        ("mppi", 1024, "0.01"), ("mppi", 100, "5.0"), ("covo-offline", 40, "0.01")])
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_small_fused_step_equals_staged(name, N, lam, graph, monkeypatch):
    """SURVEY 8f-2 at the small configs (csrc/step_small.hip): begin + noise draw + rollout + softmax records + merge as ONE
    launch against the staged launches of the same step (covo_debug_set_fuse_small(0)) -- same device functions, same record
    order, same merge: new mean, actions, costs (and MPPI's shifted covariances) bit for bit, eager and as a captured graph, at
    a full config, ragged sizes, a single partial group and temperatures where every sample carries weight; gamma_mean != 1.
    Round 6: the fused launch's last step is also checked against oracle/ directly (_oracle_check_of_a_fused_step)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    task = "hovering" if name == "mppi" else "tracking_zigzag"
    env = cm.envs.Quad3D(task=task, enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=(N != 1000),
                         generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    lib = _lib.load_library()
    params = env.default_params
    res = []
    try:
        for fuse in (1, 0):
            c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
            _lib.check(lib.covo_debug_set_fuse_small(c.core.h, fuse), "fuse_small")  # (a switch of THIS handle)
            obs, info, state = env.reset(cr.PRNGKey(14), params)
            cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(5))
            if N == 1000:
                cp = cp.replace(gamma_mean=0.7)
            key = cr.PRNGKey(16)
            out = []
            for step in range(5):  # graph: eager, capture, replays
                key, k_act, k_step = cr.split(key, 3)
                am_before = cp.a_mean.cpu().numpy().copy()
                u, cp, _ = c(obs, state, params, k_act, cp, info)
                out.append((cp.a_mean.clone(), c.core.a.clone(), c.core.cost.clone(), cp.a_cov.clone()))
                if fuse == 1 and step == 4:
                    _oracle_check_of_a_fused_step(name, env, params, info["noisy_state"], am_before, k_act, c.core, cp, lam,
                                                  gamma_mean=0.7 if N == 1000 else 1.0, rollover=(N == 1000))
                obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
            assert c.core.device_status() == 0
            res.append(out)
            c.core.close()
    finally:
        pass
    for step, (f, s) in enumerate(zip(*res)):
        for what, x, y in zip(("a_mean", "a", "cost", "a_cov"), f, s):
            assert torch.equal(x, y), (name, N, graph, step, what, (x - y).abs().max().item())
    assert torch.isfinite(res[0][-1][0]).all() and (res[0][-1][0] - res[0][0][0]).abs().max() > 0


def test_small_fused_step_on_a_sharded_rank_leaves_the_merged_record():
    """The fused small step with partial_out set (a sample-sharded rank, N_local <= 16 384: the 8 192-sample shards of BASELINE
    configs[3] under covo-offline / MPPI): the launch's last workgroup writes the rank's merged record {m, s, v} instead of the
    mean -- bit-equal to the staged launches' record."""
    core = SamplingCore(4096, 32, 0.01, 1.0, device=DEV, use_graph=False)
    lib = core.lib
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(3), params)
    from covo_mpc_amd.dynamics.dataclass import as_device_state
    dstate = as_device_state(info["noisy_state"], DEV)
    pc = params.to_c()
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 128, 128, generator=g, dtype=torch.float64)
    L = torch.linalg.cholesky(0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64)).float().to(DEV).contiguous()
    a_mean = (0.1 * torch.randn(128, generator=g)).to(DEV)
    recs = []
    try:
        for fuse in (1, 0):
            _lib.check(lib.covo_debug_set_fuse_small(core.h, fuse), "fuse_small")
            args, am, am_shift, _ = core._prepare_step(_lib.MODE_COVO_OFFLINE, dstate, a_mean, L_table=L, derive_keys=True)
            rec = torch.zeros(_lib.COVO_PARTIAL_FLOATS, device=DEV)
            args.partial_out = rec.data_ptr()
            args.a_mean_shift = am_shift.data_ptr()
            import ctypes as C
            _lib.check(lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 7, 9, None, core.stream()), "covo_mpc_step")
            torch.cuda.synchronize()
            recs.append((rec.clone(), am_shift.clone(), core.cost.clone()))
            core._args_cache = None
    finally:
        _lib.check(lib.covo_debug_set_fuse_small(core.h, 1), "fuse_small")
    assert all(torch.equal(x, y) for x, y in zip(*recs)) and recs[0][0][1] > 0 and torch.isfinite(recs[0][0]).all()
    core.close()


@pytest.mark.parametrize("N,lam", [(65536, "0.01"), (4096, "0.01"), (1000, "1.0"), (70000, "0.01")])
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_streamed_gemm_equals_the_gemm_launch(N, lam, graph, monkeypatch):
    """covo-online's noise GEMM streamed under the factorisation inside the Sigma chain's finalize launch (the default for one
    matrix; sigma_ns.hip: ns_finalize_stream_kernel -- one workgroup factors and sends panel after panel, the others multiply)
    against the GEMM as a launch of its own behind the chain (covo_debug_set_stream_gemm(handle, 0)): actions, costs, a_cov and the new
    mean bit for bit -- at the headline size (8 worker waves own two tiles), a small one (most workers idle), a ragged count, one
    beyond 65 536, eager and as a captured graph, with and without the position statistics.
    Round 6: the streamed launch's last step is also checked against oracle/ directly -- costs of a 2 048-sample subsample at
    N = 65 536, the Sigma it sampled from against the oracle Hessian's eigh-based optimize_sigma (_oracle_check_of_a_fused_step)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    lib = _lib.load_library()
    params = env.default_params
    res = []
    try:
        for on in (1, 0):
            c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam{lam}", device=DEV, compute_info=(N == 4096))
            _lib.check(lib.covo_debug_set_stream_gemm(c.core.h, on), "stream_gemm")  # (a switch of THIS handle)
            obs, info, state = env.reset(cr.PRNGKey(34), params)
            cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(5))
            key = cr.PRNGKey(36)
            out = []
            for step in range(4):
                key, k_act, k_step = cr.split(key, 3)
                am_before = cp.a_mean.cpu().numpy().copy()
                u, cp, _ = c(obs, state, params, k_act, cp, info)
                out.append((cp.a_mean.clone(), c.core.a.clone(), c.core.cost.clone(), cp.a_cov.clone()))
                if on == 1 and step == 3:
                    _oracle_check_of_a_fused_step("covo-online", env, params, info["noisy_state"], am_before, k_act, c.core, cp, lam)
                obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
            assert c.core.device_status() == 0
            res.append(out)
            c.core.close()
    finally:
        pass
    for step, (f, s) in enumerate(zip(*res)):
        for what, x, y in zip(("a_mean", "a", "cost", "a_cov"), f, s):
            assert torch.equal(x, y), (N, graph, step, what, (x - y).abs().max().item())
    assert torch.isfinite(res[0][-1][0]).all() and torch.isfinite(res[0][-1][3]).all()


@pytest.mark.parametrize("kind", ["gaussian", "none"])
def test_folded_begin_equals_the_begin_launch(kind, monkeypatch):
    """eager covo-online steps fold the begin work (mean shift, key derivation, sequence bump) into the Hessian's first
    launch and read args->state where it lies (covo_debug_set_fold_begin(handle, 1), the default) -- against the begin launch of
    its own with the fixed-address state copy (0): actions, costs, a_cov and the new mean bit for bit over a few closed-loop
    steps, and the two settings live side by side on two handles of one process (the switches are per handle since round 6)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type=kind, disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    lib = _lib.load_library()
    params = env.default_params
    ctrls = []
    for on in (1, 0):
        c, _ = cm.envs.get_controller(env, "covo-online", "N4096_H32_lam0.01", device=DEV, compute_info=False)
        _lib.check(lib.covo_debug_set_fold_begin(c.core.h, on), "fold_begin")
        ctrls.append(c)
    obs, info, state = env.reset(cr.PRNGKey(44), params)
    cps = [c.reset(state, params, c.init_control_params, cr.PRNGKey(5)) for c in ctrls]
    key = cr.PRNGKey(46)
    for step in range(4):
        key, k_act, k_step = cr.split(key, 3)
        outs = []
        for i, c in enumerate(ctrls):  # interleaved: two handles with different settings alive at once
            u, cps[i], _ = c(obs, state, params, k_act, cps[i], info)
            outs.append((cps[i].a_mean.clone(), c.core.a.clone(), c.core.cost.clone(), cps[i].a_cov.clone(), u.clone()))
        for what, x, y in zip(("a_mean", "a", "cost", "a_cov", "u"), *outs):
            assert torch.equal(x, y), (kind, step, what, (x - y).abs().max().item())
        obs, state, reward, done, info = env.step(k_step, state, outs[0][4].cpu().numpy(), params)
    assert all(c.core.device_status() == 0 for c in ctrls) and torch.isfinite(outs[0][0]).all()
    for c in ctrls:
        c.core.close()


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_merged_sigma_chain_launch_equals_two_launches(graph, monkeypatch):
    """Round 6 (VERDICT r05 Next 2, what of it pays): the one-matrix Sigma chain's squaring launch (with the evaluations inside) and
    its Newton-Schulz launch as ONE launch whose iteration workgroups wait inside for the chain's result (sigma_ns.hip:
    ns_chain_kernel; covo_debug_set_ns_merged(handle, 1), the default) against the two launches of rounds 4-5 (0): actions, costs,
    a_cov and the new mean of closed-loop covo-online steps bit for bit, eager and as a captured graph, two handles with the two
    settings side by side; the Sigma of the last step against the oracle Hessian's eigh-based optimize_sigma (2e-5)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    lib = _lib.load_library()
    params = env.default_params
    ctrls = []
    for on in (1, 0):
        c, _ = cm.envs.get_controller(env, "covo-online", "N4096_H32_lam0.01", device=DEV, compute_info=False)
        _lib.check(lib.covo_debug_set_ns_merged(c.core.h, on), "ns_merged")
        ctrls.append(c)
    obs, info, state = env.reset(cr.PRNGKey(54), params)
    cps = [c.reset(state, params, c.init_control_params, cr.PRNGKey(5)) for c in ctrls]
    key = cr.PRNGKey(56)
    for step in range(8):
        key, k_act, k_step = cr.split(key, 3)
        am_before = cps[0].a_mean.cpu().numpy().copy()
        outs = []
        for i, c in enumerate(ctrls):
            u, cps[i], _ = c(obs, state, params, k_act, cps[i], info)
            outs.append((cps[i].a_mean.clone(), c.core.a.clone(), c.core.cost.clone(), cps[i].a_cov.clone(), u.clone()))
        for what, x, y in zip(("a_mean", "a", "cost", "a_cov", "u"), *outs):
            assert torch.equal(x, y), (graph, step, what, (x - y).abs().max().item())
        if step == 7:
            _oracle_check_of_a_fused_step("covo-online", env, params, info["noisy_state"], am_before, k_act, ctrls[0].core, cps[0], "0.01")
        obs, state, reward, done, info = env.step(k_step, state, outs[0][4].cpu().numpy(), params)
    assert all(c.core.device_status() == 0 for c in ctrls)
    for c in ctrls:
        c.core.close()


def test_sigma_batch_beyond_residency_persistent_equals_shared_device():
    """the batched persistent launches of the Sigma chain (and, since round 5, the sibling factorisations of B inside the
    finalize launch: 2 x 300 single-CU workgroups) rely on in-order dispatch once the grid exceeds what is resident -- covo-offline's
    300-row table is such a batch.  300 matrices, persistent launches against COVO_FLAG_SHARED_DEVICE (every phase its own launch):
    Sigma and L bit for bit, finite, and a clean device status (no barrier / flag time-out)."""
    rng = np.random.default_rng(11)
    n = 128
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    base = []
    G = rng.standard_normal((n, n)); base.append(0.05 * (G + G.T))
    w = np.concatenate([[-2.0, -1.1, -0.7], np.geomspace(0.01, 900.0, n - 3)]); base.append((Q * w) @ Q.T)
    w = np.concatenate([np.abs(rng.standard_normal(20)) * 50, rng.standard_normal(108) * 0.05]); base.append((Q * w) @ Q.T)
    mats = np.stack([base[i % 3] * (1.0 + 0.01 * i) + 0.003 * i * np.eye(n) for i in range(300)])
    R_d = torch.from_numpy(np.ascontiguousarray(mats)).to(DEV)
    outs = []
    for shared in (False, True):
        core = SamplingCore(256, 32, 0.01, 1.0, device=DEV, shared_device=shared)
        Sig, L = core.sigma(R_d, 0.5, batch=300)
        torch.cuda.synchronize()
        assert core.device_status() == 0
        outs.append((Sig.clone(), L.clone()))
        core.close()
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = np.linalg.eigh(mats[7])
    lam = ref[0] - ref[0].min() + 1e-2
    S7 = (ref[1] * np.exp(0.5 * (2 * np.log(0.5) * 2 + np.log(lam).sum() / n) - 0.5 * np.log(lam))) @ ref[1].T
    assert np.linalg.norm(outs[0][0][7].cpu().numpy() - S7) / np.linalg.norm(S7) < 1e-6
