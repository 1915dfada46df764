"""CPU: the ABI of the flight recorder (covo_set_step_plan / covo_set_episode_trace, include/covo_hip.h), the `compute_plan` keyword
of the Python surface, and render_env (quadrotor.py:594-667 without the plots) on the host path."""
import ctypes as C
import inspect
import pickle
import re

import numpy as np

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_plan_trace_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"int covo_set_step_plan\(covo_handle_t h, float \*plan, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_set_episode_trace\(covo_handle_t h, float \*trace, int32_t stride\);", hdr)
    assert re.search(r"#define COVO_HAS_PLAN_TRACE 1\b", hdr)
    assert int(re.search(r"#define COVO_PLAN_FLOATS\s+(\d+)", hdr).group(1)) == 100 == built.COVO_PLAN_FLOATS
    assert int(re.search(r"#define COVO_TRACE_FLOATS\s+(\d+)", hdr).group(1)) == 168 == built.COVO_TRACE_FLOATS
    assert built.COVO_TRACE_FLOATS == 2 * 32 + 4 + built.COVO_PLAN_FLOATS and built.COVO_PLAN_FLOATS == 4 + 3 * built.COVO_H
    for name in ("covo_set_step_plan", "covo_set_episode_trace"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32], name
        assert name in built.EXPORTS
    # the ABI version did not move: the symbols are additive
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_plan(None, None, 0) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_trace(None, None, 0) != 0 and b"null handle" in lib.covo_last_error()


def test_compute_plan_is_a_keyword_defaulting_to_false(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller):
        p = inspect.signature(fn).parameters
        assert "compute_plan" in p and p["compute_plan"].default is False, fn
    assert inspect.signature(eval_env_batched).parameters["trace"].default is False


def _same(a, b):
    """bit-for-bit equality of two state-sequence entries"""
    assert set(a) == set(b), (set(a) ^ set(b))
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
        else:
            assert type(x) is type(y) and x == y, (k, x, y)


def test_render_env_on_the_host_is_the_reference_loop(built, tmp_path, monkeypatch):
    """PID on the host env: 301 entries (the first `done` is time >= 300, seen by the 301st step), entry k entering step k, every
    entry equal bit for bit to the loop of quadrotor.py:594-646 written out here with the same keys; the pickle round-trips."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    from covo_mpc_amd.envs.quadrotor import get_controller, render_env
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device=None)
    controller, cp = get_controller(env, "pid")
    seq = render_env(env, controller, cp, save=False)
    assert len(seq) == 301
    assert all(int(e["time"]) == k for k, e in enumerate(seq))
    assert all("u" not in e and "pos_plan" not in e and "cost_plan" not in e and "traj_dev" not in e and "reward" in e for e in seq)

    rng = cr.PRNGKey(1)
    rng, rng_params = cr.split(rng)
    params = env.sample_params(rng_params)
    rng, rng_reset = cr.split(rng)
    obs, info, state = env.reset(rng_reset, params)
    rng, rng_control = cr.split(rng)
    controller2, _ = get_controller(env, "pid")
    cpar = controller2.reset(state, params, controller2.init_control_params, rng_control)
    ref = []
    while True:
        d = {k: v for k, v in state.__dict__.items() if k != "traj_dev"}
        rng, rng_act, rng_step = cr.split(rng, 3)
        action, cpar, _ = controller2(obs, state, params, rng_act, cpar, info)
        obs, state, reward, done, info = env.step(rng_step, state, action, params)
        d["reward"] = reward
        ref.append(d)
        if done:
            break
    assert len(ref) == len(seq)
    for a, b in zip(seq, ref):
        _same(a, b)

    monkeypatch.chdir(tmp_path)
    controller3, cp3 = get_controller(env, "pid")
    seq2 = render_env(env, controller3, cp3, filename="abc", save=True)
    with open(tmp_path / "results" / "state_seq_abc.pkl", "rb") as f:
        loaded = pickle.load(f)
    assert len(loaded) == len(seq2) == 301
    for a, b, c in zip(loaded, seq2, seq):
        _same(a, b)
        _same(a, c)


def test_main_render_calls_render_env(built, monkeypatch):
    from covo_mpc_amd.envs import quadrotor as q
    calls = []

    def fake_render(env, controller, control_params, repeat_times=1, filename="", save=True, host_env=False):
        calls.append(dict(filename=filename, controller=controller, repeat_times=repeat_times))
        return []

    class FakeEnv:
        def __init__(self, **kw):
            self.kw = kw

    monkeypatch.setattr(q, "render_env", fake_render)
    monkeypatch.setattr(q, "Quad3D", FakeEnv)
    monkeypatch.setattr(q, "get_controller", lambda env, name, params=None, **kw: (("controller", name, kw), None))
    args = q.Args(mode="render", controller="pid", task="tracking_zigzag", name="my_run")
    assert q.Args().mode == "render"
    q.main(args)
    assert len(calls) == 1 and calls[0]["filename"] == "my_run" and calls[0]["controller"][1] == "pid"
    assert calls[0]["controller"][2].get("compute_plan") is True
