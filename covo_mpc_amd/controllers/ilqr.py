"""iLQR behind quadjax's controller call signature: Riccati sweeps and the closed-loop line search, nothing sampled.

The reference has no gradient-based controller; this one consists of the parts the sampling controllers attach behind their update
(riccati=, riccati_feedback=, plan_hold=: _options.py) and of nothing else.  One control step on the noisy state, with the raw key
rng_act and the incoming mean:
    b_0 = shift(a_mean);   b_{j+1} = the Riccati line search at b_j, j = 0 .. iters - 1;   a_mean <- b_iters;   u = a_mean[0]
(COVO_MODE_ILQR, include/covo_hip.h; csrc/ilqr.hip).  Every iteration sees the step's one state, trajectory slices and the disturbance
inputs a CoVO step derives from rng_act on the device; the key is not walked between iterations, so the objective is one per step.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Any

from .. import _lib
from ..dynamics.dataclass import as_device_state
from .base import BaseController
from ._core import SamplingCore
from ._options import check_ilqr

ILQR_N = 1  # the sample count the controllers' SamplingCore is built at: the smallest it takes (its sample buffers are never launched on)


@dataclass(frozen=True)
class ILQRParams:
    """a_mean (H,4): torch fp32 tensor on the GPU -- the plan, carried from step to step."""
    a_mean: Any
    discount: float = 1.0

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


def build_ilqr_core(n_rows, H, discount, *, iters, switches, compute_plan, device, use_graph=None):
    """The SamplingCore of an iLQR controller for n_rows instances: the Riccati rows [+ feedback rows, hold rows, plan rows] attached
    as a sampling controller attaches them, the iteration count set, the per-iteration logs attached (SamplingCore.attach_ilqr).
    switches: the step switches check_ilqr resolved (riccati_feedback, plan_hold, riccati_box); riccati is implied."""
    core = SamplingCore(ILQR_N, H, 1.0, discount, device=device, compute_info=False, trust_clipped=True, use_graph=use_graph,
                        diag_rows=int(n_rows), compute_plan=compute_plan, iters=iters, riccati=True, **switches)
    core.attach_ilqr()
    return core


class ILQRController(BaseController):
    # riccati_box of the sampling controllers (_options.check_riccati_box): every iteration's sweep solves the control-limited stage
    # problem.  A class attribute, not a constructor keyword -- the constructor's parameter list is a published one; ILQRBoxController
    # below sets it, and get_controller(env, "ilqr", ..., riccati_box=True) builds that class
    riccati_box = False

    def __init__(self, env, control_params, H: int, *, iters: int = 2, riccati_feedback=None, plan_hold: int = 1,
                 compute_plan: bool = False, device=None) -> None:
        # ValueError / NotImplementedError before anything is built; riccati_feedback=None: True on the 13-state plants, False on drag / mixed
        self.iters, self.riccati_feedback, self.plan_hold = check_ilqr(
            iters, riccati_feedback=riccati_feedback, plan_hold=plan_hold, disturb_type=getattr(env, "disturb_type", None),
            compute_plan=compute_plan, riccati_box=self.riccati_box)
        super().__init__(env, control_params)
        self.H = H
        self.alias_outputs = False  # True: the returned a_mean aliases the controller's buffer (no clone)
        self._params_c(env.default_params)  # raises now if env.reward_fn / disturb_type is not one the kernels evaluate
        switches = dict(riccati_feedback=self.riccati_feedback, plan_hold=self.plan_hold, riccati_box=self.riccati_box)
        self.core = build_ilqr_core(1, H, getattr(control_params, "discount", 1.0), iters=self.iters, switches=switches,
                                    compute_plan=bool(compute_plan), device=device)

    def reset(self, env_state=None, env_params=None, control_params=None, key=None):
        """Episode start: with a plan hold the schedule restarts -- the first step of the episode plans."""
        self.core.restart_plan_hold()
        self.core.estimator_reset()
        self.core.force_observer_reset()
        return super().reset(env_state, env_params, control_params, key)

    def run_episode(self, episode, env_params, control_params, rng, n_steps):
        """n_steps closed-loop steps (this controller + the device env step) enqueued by one C call; keys threaded like eval_env's
        run_one_step.  -> (control_params with the final mean, rng)."""
        am, _, rng = self.core.run_episode(_lib.MODE_ILQR, episode, self._params_c(env_params), control_params.a_mean, rng, n_steps,
                                           rollout_deterministic=True)
        a_mean = am.view(self.H, 4)
        if not self.alias_outputs:
            a_mean = a_mean.clone()
        return control_params.replace(a_mean=a_mean), rng

    def __call__(self, obs, env_state, env_params, rng_act, control_params: ILQRParams, info):
        core = self.core
        dstate = as_device_state(info["noisy_state"], core.device)
        dstate = core.estimated(dstate, control_params.a_mean, lambda: self._params_c(env_params))  # (an attached StateEstimator)
        am, _ = core.step(_lib.MODE_ILQR, dstate, self._params_c(env_params), control_params.a_mean, rng_act, derive_keys=True,
                          rollout_deterministic=True)
        a_mean_new = am.view(self.H, 4)
        if not self.alias_outputs:
            a_mean_new = a_mean_new.clone()
        return a_mean_new[0], control_params.replace(a_mean=a_mean_new), core.step_info()


class ILQRBoxController(ILQRController):
    """ILQRController over the box sweep: info also carries riccati_box_mask / riccati_box_count / ilqr_box_count"""
    riccati_box = True
