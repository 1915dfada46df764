"""CPU: the step options' one table (covo_mpc_amd/controllers/_options.py) against the signatures that carry them, the refusals
that need no device, and the record check_step_options returns."""
import inspect

import pytest


def _entry_points():
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import get_controller
    return (SamplingCore.__init__, controllers.CoVOController.__init__, controllers.MPPIController.__init__,
            controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller)


def test_every_entry_point_carries_the_table_in_its_signature():
    """Names and defaults, so the table and the signatures cannot drift: an option missing from a signature is a KeyError in take(),
    one missing from the table would never be checked or forwarded."""
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS
    from covo_mpc_amd.envs.quadrotor import eval_env_batched
    assert list(STEP_OPTION_DEFAULTS) == ["compute_diag", "compute_plan", "ess_min", "compute_fan", "update", "iters", "elite",
                                          "sigma_period", "compute_post_cov", "sigma_adapt"]
    for fn in _entry_points():
        p = inspect.signature(fn).parameters
        assert not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in p.values()), fn
        for name, default in STEP_OPTION_DEFAULTS.items():
            assert name in p, (fn, name)
            assert p[name].default == default and type(p[name].default) is type(default), (fn, name)
    # eval_env_batched: the driver's three documented renames; it has no ess_min / compute_post_cov of its own
    renames = {"compute_diag": "diag", "compute_plan": "trace", "compute_fan": "fan"}
    p = inspect.signature(eval_env_batched).parameters
    for name, default in STEP_OPTION_DEFAULTS.items():
        mine = renames.get(name, name)
        if name in ("ess_min", "compute_post_cov"):
            assert mine not in p
            continue
        assert p[mine].default == default and type(p[mine].default) is type(default), name
    for name in renames:
        assert name not in p


def test_take_and_unknown_keywords():
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_step_options, take
    ns = dict(STEP_OPTION_DEFAULTS, self=None, N=256, iters=3)
    assert take(ns) == dict(STEP_OPTION_DEFAULTS, iters=3) and list(take(ns)) == list(STEP_OPTION_DEFAULTS)
    with pytest.raises(TypeError, match="compute_fann"):
        check_step_options(256, "online", compute_fann=8)


@pytest.mark.parametrize("option", ["compute_diag", "compute_plan"])
def test_sharded_core_refuses_diag_and_plan_without_a_device(monkeypatch, option):
    """A process group of two ranks: NotImplementedError before the device is looked for, like the other eight options."""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match=f"{option} on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, **{option: True})


def test_check_step_options_returns_the_normalised_record():
    from covo_mpc_amd.controllers._options import StepOptions, check_step_options
    assert check_step_options(256, "online") == StepOptions(
        diag=False, plan=False, ess_min=0.0, fan_K=0, update="softmax", arb_mask=0, iters=1, elite_K=0, sigma_period=1,
        post_cov=False, sigma_adapt=0.0)
    on = check_step_options(N=256, what="online", compute_diag=True, compute_plan=True, compute_fan=8, update="guarded", iters=2,
                            elite=32, sigma_period=4, compute_post_cov=False, sigma_adapt=0.1)
    assert on == StepOptions(diag=True, plan=True, ess_min=0.0, fan_K=8, update="guarded", arb_mask=0b111, iters=2, elite_K=32,
                             sigma_period=4, post_cov=True, sigma_adapt=0.1)
    assert on.post_cov is True  # forced on by sigma_adapt > 0
    with pytest.raises(Exception):  # frozen
        on.iters = 3
    # N not known yet: the two checks that need it are skipped, and their fields say so
    early = check_step_options(None, "online", compute_fan=1000, elite=10 ** 9, ess_min=8)
    assert early.fan_K is None and early.elite_K is None and early.ess_min == 8.0


def test_check_step_options_objects_in_its_fixed_order():
    """Ranges (ValueError) first, in the constructors' order; then the fused env-batched step's refusals; then the sharded ones."""
    from covo_mpc_amd.controllers._options import check_step_options
    with pytest.raises(ValueError, match="sigma_period="):
        check_step_options(256, "online", sigma_period=0, sigma_adapt=2.0, compute_fan=999, update="x", iters=0, elite=999)
    with pytest.raises(ValueError, match="sigma_adapt="):
        check_step_options(256, "online", sigma_adapt=2.0, compute_fan=999, update="x", iters=0, elite=999)
    with pytest.raises(ValueError, match="compute_fan="):
        check_step_options(256, "online", compute_fan=999, update="x", iters=0, elite=999)
    with pytest.raises(ValueError, match="update="):
        check_step_options(256, "online", update="x", iters=0, elite=999)
    with pytest.raises(ValueError, match="iters="):
        check_step_options(256, "online", iters=0, elite=999)
    with pytest.raises(ValueError, match="elite="):
        check_step_options(256, "online", elite=999, sharded=True, fused_batched=True)
    with pytest.raises(ValueError, match="sigma_period=2 with MPPI"):
        check_step_options(256, "MPPI", sigma_period=2)
    with pytest.raises(ValueError, match="elite=4 with gamma_sigma=1.0"):
        check_step_options(256, "MPPI", gamma_sigma=1.0, elite=4)
    with pytest.raises(NotImplementedError, match="elite=8: the elite-set update is not available for the env-batched"):
        check_step_options(256, "the env-batched MPPI controller", fused_batched=True, sharded=True, elite=8, compute_post_cov=True)
    with pytest.raises(NotImplementedError, match="compute_post_cov: the posterior covariance is not available"):
        check_step_options(256, "the env-batched MPPI controller", fused_batched=True, compute_post_cov=True, iters=2, update="best")
    with pytest.raises(NotImplementedError, match="iters=2 with update='best': not available"):
        check_step_options(256, "the env-batched MPPI controller", fused_batched=True, iters=2, update="best", ess_min=8)
    with pytest.raises(NotImplementedError, match="ess_min=8: the ESS floor is not available"):
        check_step_options(256, "the env-batched MPPI controller", fused_batched=True, ess_min=8)
    with pytest.raises(NotImplementedError, match="iters=2 on sample-sharded ranks"):
        check_step_options(256, "online", sharded=True, iters=2, update="best", compute_diag=True)
    with pytest.raises(NotImplementedError, match="ess_min=8 on sample-sharded ranks"):
        check_step_options(256, "online", sharded=True, ess_min=8, compute_post_cov=True, compute_plan=True)
    with pytest.raises(NotImplementedError, match="compute_diag on sample-sharded ranks"):
        check_step_options(256, "online", sharded=True, compute_diag=True, compute_plan=True)


def test_every_entry_point_carries_the_switches():
    """The step switches' table against the signatures, as for the step options above: names, defaults and the defaults' exact types."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_SWITCH_DEFAULTS
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    assert list(STEP_SWITCH_DEFAULTS) == ["refine", "riccati", "riccati_feedback", "plan_hold", "riccati_box"]
    assert STEP_SWITCH_DEFAULTS == {"refine": False, "riccati": False, "riccati_feedback": False, "plan_hold": 1, "riccati_box": False}
    assert type(STEP_SWITCH_DEFAULTS["plan_hold"]) is int
    for fn in (SamplingCore.__init__, controllers.CoVOController.__init__, controllers.MPPIController.__init__,
               controllers.BatchedCoVOController.__init__, get_controller, eval_env_batched):
        p = inspect.signature(fn).parameters
        assert not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in p.values()), fn
        for name, default in STEP_SWITCH_DEFAULTS.items():
            if fn is controllers.MPPIController.__init__ and name == "refine":  # the one documented exception (take_switches)
                assert name not in p
                continue
            assert name in p, (fn, name)
            assert p[name].default == default and type(p[name].default) is type(default), (fn, name)
        # in the table's order
        assert [n for n in p if n in STEP_SWITCH_DEFAULTS] == [n for n in STEP_SWITCH_DEFAULTS if n in p], fn
    # the env-batched MPPI controller carries no switch (its step refuses riccati, which the others build on)
    p = inspect.signature(controllers.BatchedMPPIController.__init__).parameters
    assert not set(STEP_SWITCH_DEFAULTS) & set(p) and "staged" in p
    # the iLQR controllers: riccati is implied, refine has nothing to work with; the batched one takes the other three as keywords,
    # the single one's published parameter list carries no riccati_box (the class ILQRBoxController)
    p = inspect.signature(controllers.BatchedILQRController.__init__).parameters
    assert p["riccati_feedback"].default is None and p["plan_hold"].default == 1 and type(p["plan_hold"].default) is int
    assert p["riccati_box"].default is False and "refine" not in p and "riccati" not in p
    p = inspect.signature(controllers.ILQRController.__init__).parameters
    assert list(p) == ["self", "env", "control_params", "H", "iters", "riccati_feedback", "plan_hold", "compute_plan", "device"]
    assert p["riccati_feedback"].default is None and p["plan_hold"].default == 1
    assert not {"riccati_box", "refine", "riccati"} & set(p)


def test_take_switches_and_unknown_keywords():
    from covo_mpc_amd.controllers._options import STEP_SWITCH_DEFAULTS, check_step_switches, take_switches
    ns = dict(STEP_SWITCH_DEFAULTS, self=None, N=256, riccati=True, plan_hold=3)
    assert take_switches(ns) == dict(STEP_SWITCH_DEFAULTS, riccati=True, plan_hold=3)
    assert list(take_switches(ns)) == list(STEP_SWITCH_DEFAULTS)
    # a namespace without refine (MPPIController's): taken at its default
    del ns["refine"]
    assert take_switches(ns) == dict(STEP_SWITCH_DEFAULTS, riccati=True, plan_hold=3) and take_switches(ns)["refine"] is False
    assert take_switches({}) == STEP_SWITCH_DEFAULTS
    with pytest.raises(TypeError, match=r"check_step_switches: unknown step switches \['riccati_boxx'\]"):
        check_step_switches("online", riccati_boxx=True)
    with pytest.raises(TypeError, match="unknown step switches"):  # a step option is not a switch
        check_step_switches("online", iters=2)


def test_check_step_switches_returns_the_record():
    from covo_mpc_amd.controllers._options import StepSwitches, check_step_switches
    off = check_step_switches("online")
    assert off == StepSwitches(refine=False, riccati=False, riccati_feedback=False, plan_hold=1, riccati_box=False)
    assert off.refine is False and off.riccati is False and type(off.plan_hold) is int
    on = check_step_switches("covo-offline", mode_what="covo-offline", disturb_type="gaussian", riccati=True, riccati_feedback=True,
                             plan_hold=3, riccati_box=True)
    assert on == StepSwitches(refine=False, riccati=True, riccati_feedback=True, plan_hold=3, riccati_box=True)
    assert check_step_switches("a sampling core", mode_what="online", riccati_what="a sampling core", refine=True).refine is True
    with pytest.raises(Exception):  # frozen
        on.plan_hold = 1
