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
