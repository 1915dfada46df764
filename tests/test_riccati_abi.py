"""CPU: the ABI of the Riccati refinement (covo_riccati / covo_riccati_refine / covo_set_step_riccati, include/covo_hip.h:
COVO_HAS_RICCATI_REFINE), the `riccati` switch of the Python surface (controllers/_options.py: check_riccati -- a switch like refine=,
not a step option) and the fp64 oracle the GPU tests hold the kernel against (tests/riccati_oracle.py), checked against itself:
the sweep's direction against -solve(R + mu I, g) of oracle/ref_torch.py's AD Hessian, its pivots against the spectrum of R, its
gains against the tail problems they solve."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env():
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def test_riccati_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_RICCATI_REFINE 1$", hdr, flags=re.M) and built.COVO_HAS_RICCATI_REFINE == 1
    assert int(re.search(r"#define COVO_RICCATI_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_RICCATI_FLOATS
    assert int(re.search(r"#define COVO_RICCATI_SIDE\s+(\d+)", hdr).group(1)) == 4 == built.COVO_RICCATI_SIDE
    assert int(re.search(r"#define COVO_RICCATI_RUNGS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_RICCATI_RUNGS
    assert float(re.search(r"#define COVO_RICCATI_REG0\s+(\S+)", hdr).group(1)) == 1e-2 == built.COVO_RICCATI_REG0
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    EP, F3 = C.POINTER(built.EnvParamsC), C.POINTER(C.c_float)
    want = {
        "covo_riccati": [P, P, P, P, I, EP, P, P, I, D, P, P, P, P, P, P],
        "covo_riccati_refine": [P, P, P, P, I, EP, F3, P, P, P, D, I, P, P, P],
        "covo_set_step_riccati": [P, P, I],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    # additive: the ABI version did not move and covo_newton_refine keeps its 17 arguments
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    assert len(lib.covo_newton_refine.argtypes) == 17
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_riccati(None, None, 1) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_riccati(None, None, None, None, 0, None, None, None, 0, 1e-2, None, None, None, None, None, None) != 0
    assert b"null handle" in lib.covo_last_error()
    assert lib.covo_riccati_refine(None, None, None, None, 0, None, None, None, None, None, 1e-2, 0, None, None, None) != 0
    assert b"null handle" in lib.covo_last_error()


def test_riccati_is_a_switch_not_a_step_option(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _core
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_riccati
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    assert "riccati" not in STEP_OPTION_DEFAULTS
    assert built.COVO_EPLOG_KINDS == 6 and not any("riccati" in k for k in _core.EPISODE_LOGS)
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, get_controller, eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "riccati" in p and p["riccati"].default is False, fn
    assert "riccati" not in inspect.signature(controllers.BatchedMPPIController.__init__).parameters
    assert Args().riccati is False
    assert callable(SamplingCore.riccati) and callable(SamplingCore.riccati_refine) and callable(SamplingCore.riccati_info)
    assert inspect.signature(SamplingCore.riccati).parameters["reg0"].default == 1e-2
    assert check_riccati(False, "the env-batched MPPI controller", refine=True, sharded=True) is False  # off: nothing to object to
    for what in ("MPPI", "covo-offline", "online"):
        assert check_riccati(True, what) is True


def test_check_riccati_objects_in_a_fixed_order(built, monkeypatch):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import check_riccati
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    batched = "the env-batched MPPI controller"
    # 1. anything but a bool, whatever else is wrong
    for bad in ("yes", 1, None, 0.0):
        with pytest.raises(ValueError, match="riccati="):
            check_riccati(bad, batched, refine=True, sharded=True)
        with pytest.raises(ValueError, match="riccati="):
            SamplingCore(256, 32, 0.01, 1.0, riccati=bad)
    # 2. together with refine=True, ahead of the batched and the sharded objection
    with pytest.raises(ValueError, match="riccati=True together with refine=True"):
        check_riccati(True, batched, refine=True, sharded=True)
    with pytest.raises(ValueError, match="riccati=True together with refine=True"):
        get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", refine=True, riccati=True)
    with pytest.raises(ValueError, match="riccati=True together with refine=True"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, refine=True, riccati=True)
    # 3. the env-batched MPPI / covo-offline controllers, fused or staged, ahead of the sharded objection
    with pytest.raises(NotImplementedError, match="riccati=True with the env-batched MPPI controller"):
        check_riccati(True, batched, sharded=True)
    for staged in (False, True):
        with pytest.raises(NotImplementedError, match="riccati=True with the env-batched covo-offline controller"):
            controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", staged=staged, riccati=True)
    for name in ("mppi", "covo-offline"):
        with pytest.raises(NotImplementedError, match="riccati=True with the env-batched"):
            eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller=name, riccati=True)
    # 4. sample-sharded ranks
    with pytest.raises(NotImplementedError, match="riccati=True on sample-sharded ranks"):
        check_riccati(True, "MPPI", sharded=True)
    import torch.distributed as dist
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="riccati=True on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, riccati=True)
    for name in ("mppi", "covo-online"):
        with pytest.raises(NotImplementedError, match="riccati=True on sample-sharded ranks"):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", process_group=group, riccati=True)

    # the kernel-by-kernel path
    class Stub:
        riccati_on = True

    with pytest.raises(NotImplementedError, match="riccati follows the fused step"):
        SamplingCore.require_fused_for_diag(Stub())


def test_riccati_goes_with_every_single_controller_and_sigma_period(built):
    """accepted: the construction gets as far as the device check (no GPU), or builds (GPU)"""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    for name, kw in (("mppi", {}), ("covo-offline", {}), ("covo-online", {}), ("covo-online", dict(sigma_period=4)),
                     ("covo-online", dict(iters=2, update="guarded"))):
        if torch.cuda.is_available():
            c, _ = get_controller(_env(), name, "N256_H32_lam0.01", device="cuda:0", riccati=True, **kw)
            assert c.core.riccati_on is True and tuple(c.core.riccati_rows.shape) == (1, 8)
            c.core.close()
        else:
            with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
                get_controller(_env(), name, "N256_H32_lam0.01", device="cpu", riccati=True, **kw)


# ---------------------------------------------------------------------------------------------- the oracle against itself
@functools.lru_cache(maxsize=None)
def _oracle_case():
    """make_problem(seed=17), hover + 0.3 noise (the clip is live): the blocks, the AD Hessian and gradient of the same objective"""
    import torch
    from oracle import ref_np as R
    from oracle import ref_torch as RT
    from tests import riccati_oracle as RO
    from tests.conftest import make_problem
    s, p, rng = make_problem(seed=17, time=37)
    b = (R.hover_action(p, 32, np.float64) + 0.3 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1).astype(np.float64)
    assert np.abs(b).max() > 1.0
    forces = RO.step_forces(s, p, "none")
    blk = RO.stage_blocks(s, p, b, "penyaw", forces)
    Rm = RT.hessian(s, p, b, 32, "penyaw", "none", None)
    g = torch.func.jacfwd(RT.make_objective(s, p, 32, "penyaw", "none", None))(torch.as_tensor(b)).numpy()
    return s, p, b, forces, blk, (Rm + Rm.T) / 2.0, g


def test_oracle_direction_is_the_regularised_newton_step():
    from tests import riccati_oracle as RO
    s, p, b, forces, blk, Rm, g = _oracle_case()
    assert np.abs(blk["g"] - g).max() <= 1e-10 * max(1.0, np.abs(g).max())
    lam = np.linalg.eigvalsh(Rm)
    assert lam.min() < 0.0  # the ladder has something to do
    seen = 0
    for j in range(RO.RUNGS):
        mu = 1e-2 * 4.0 ** j
        r = RO.sweep(blk, mu)
        # all 32 pivots positive exactly where R + mu I is positive definite
        assert abs(lam.min() + mu) > 0.05 * abs(lam.min())  # decidable
        assert r["ok"] == bool(lam.min() + mu > 0.0), (j, lam.min(), r["pivots"][-4:])
        if not r["ok"]:
            assert not (r["pivots"][-1] > 0.0)
            continue
        assert len(r["pivots"]) == 128 and min(r["pivots"]) > 0.0
        want = -np.linalg.solve(Rm + mu * np.eye(128), g)
        err = np.abs(r["d"] - want).max()
        print(f"rung {j} mu {mu:g}: |d - d_ref|max {err:.2e} on {np.abs(want).max():.2e}")
        assert err <= 1e-10 * max(1.0, np.abs(want).max()), (j, err)
        assert np.all(r["d"][124:] == 0.0) and np.all(r["K"][31] == 0.0)  # action 31 reaches no reward
        assert np.all(r["d"][np.abs(b) > 1.0] == 0.0)  # a saturated component: B's column is zero
        assert g @ r["d"] < 0.0
        seen += 1
    assert seen >= 2
    j, mu, r = RO.ladder(blk)
    assert j == int(np.argmax(lam.min() + 1e-2 * 4.0 ** np.arange(RO.RUNGS) > 0.0)) and mu == 1e-2 * 4.0 ** j


@pytest.mark.parametrize("k", [0, 12])
def test_oracle_gain_solves_the_tail_problem(k):
    from tests import riccati_oracle as RO
    s, p, b, forces, blk, Rm, g = _oracle_case()
    j, mu, r = RO.ladder(blk)
    want = RO.tail_gain(s, p, b, "penyaw", forces, k, mu, blk["x"][k])
    err = np.abs(r["K"][k] - want).max()
    print(f"K_{k}: err {err:.2e} on {np.abs(want).max():.2e}")
    assert np.abs(want).max() > 1e-2
    assert err <= 1e-10 * max(1.0, np.abs(want).max()), err
