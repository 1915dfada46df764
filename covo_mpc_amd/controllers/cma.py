"""CMA-MPC: a sampling controller that learns its full 128 x 128 covariance from its own samples, with step-size control.

The covariance-matrix-adaptation arm next to MPPI (32 independent 4 x 4 blocks), covo-offline (a table) and covo-online (the optimal
Sigma of an exact Hessian): no Hessian at all.  Every control step but the first of an episode, before it samples,
  shape      Sigma_hat' = c ((1 - gamma) S(L L^T) + gamma S(C)), log det Sigma_hat' = 2 n log sample_sigma -- CMA's rank-mu update on the
             previous step's factor L and posterior covariance C, under the Sigma period's shift S (csrc/sigma_adapt.hip, as it is);
  step size  cumulative step-size adaptation: the evolution path p follows the previous step's mean displacement in the coordinates
             whitened by L, and log s moves with |p| against its expectation under random selection (csrc/cma_path.hip);
  sampling   a = clip(shift(mu) + s L_hat' eps), with rollout, update and after-step launches of the other sampling controllers.
The first step of an episode samples from sample_sigma^2 I.  What the controller keeps between steps -- the factor, the path, log s --
lives on its core's handle; reset() starts it over.  Not taken from CMA-ES: the rank-one update (the path of the covariance), and
active (negative) weights.  controllers/_options.py: check_cma.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Any

from ..dynamics.dataclass import as_device_state
from .base import BaseController
from ._core import SamplingCore
from ._options import check_cma, check_step_options


@dataclass(frozen=True)
class CMAParams:
    """a_mean (H,4), a_cov (128,128): torch fp32 tensors on the GPU.  a_cov on input is ignored (the handle keeps the factor); the
    returned one is the covariance the step sampled from."""
    gamma_mean: float
    discount: float
    sample_sigma: float
    a_mean: Any
    a_cov: Any

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


class CMAController(BaseController):
    """MPPIController's call signature and return triple, reset and run_episode."""

    def __init__(self, env, control_params: CMAParams, N: int, H: int, lam: float, *, gamma: float = 0.2, step_size: bool = True,
                 damping: float = 1.0, s_min: float = 0.1, s_max: float = 4.0, device=None, process_group=None,
                 compute_info: bool = True, propagate_nan=None, compute_plan: bool = False, compute_fan=None, update: str = "softmax",
                 ess_min=None, elite=None, iters: int = 1, use_graph=None, sigma_period: int = 1, sigma_adapt: float = 0.0,
                 sigma_nodes=None, refine: bool = False, riccati: bool = False, riccati_feedback: bool = False, plan_hold: int = 1,
                 riccati_box: bool = False) -> None:
        # ValueError / NotImplementedError before anything is built
        self.cma = check_cma(gamma=gamma, step_size=step_size, damping=damping, s_min=s_min, s_max=s_max, sigma_period=sigma_period,
                             sigma_adapt=sigma_adapt, sigma_nodes=sigma_nodes, refine=refine, riccati=riccati,
                             riccati_feedback=riccati_feedback, plan_hold=plan_hold, riccati_box=riccati_box,
                             process_group=process_group)
        opts = dict(compute_diag=True, compute_plan=compute_plan, ess_min=ess_min, compute_fan=compute_fan, update=update, iters=iters,
                    elite=elite, compute_post_cov=True)
        check_step_options(N, "the CMA controller", **opts)
        super().__init__(env, control_params)
        self.N, self.H, self.lam = N, H, lam
        self.materialize_eps = False  # (the kernel-by-kernel path keeps no factor between steps: __call__ refuses it)
        self.noise_stream = "philox"
        self.alias_outputs = False    # True: returned a_mean / a_cov alias the controller's buffers (no clones)
        self._params_c(env.default_params)  # raises now if env.reward_fn / disturb_type is not one the kernels evaluate
        self.core = SamplingCore(N, H, lam, control_params.discount, device=device, compute_info=compute_info, trust_clipped=True,
                                 propagate_nan=propagate_nan, use_graph=use_graph, **opts)
        self.core.attach_cma(self.cma)

    def reset(self, env_state=None, env_params=None, control_params=None, key=None):
        """Episode start: L = sample_sigma I, p = 0, log s = 0 -- the first step samples from sample_sigma^2 I and adapts nothing."""
        self.core.cma_reset()
        self.core.estimator_reset()
        self.core.force_observer_reset()
        return super().reset(env_state, env_params, control_params, key)

    def _check_call(self):
        check_cma(gamma=self.cma.gamma, step_size=self.cma.step_size, damping=self.cma.damping, s_min=self.cma.s_min,
                  s_max=self.cma.s_max, materialize_eps=self.materialize_eps, noise_stream=self.noise_stream)

    def run_episode(self, episode, env_params, control_params, rng, n_steps):
        """n_steps closed-loop steps (this controller + the device env step) enqueued by one C call; keys threaded like
        eval_env's run_one_step.  -> (control_params with the final mean and the last step's covariance, rng)."""
        from .. import _lib
        self._check_call()
        am, cov, rng = self.core.run_episode(_lib.MODE_CMA, episode, self._params_c(env_params), control_params.a_mean, rng, n_steps,
                                             gamma_mean=control_params.gamma_mean, sample_sigma=control_params.sample_sigma,
                                             rollout_deterministic=True)
        a_mean = am.view(self.H, 4)
        if not self.alias_outputs:
            a_mean, cov = a_mean.clone(), cov.clone()
        return control_params.replace(a_mean=a_mean, a_cov=cov), rng

    def __call__(self, obs, env_state, env_params, rng_act, control_params: CMAParams, info):
        from .. import _lib
        core = self.core
        self._check_call()
        dstate = as_device_state(info["noisy_state"], core.device)
        dstate = core.estimated(dstate, control_params.a_mean, lambda: self._params_c(env_params))  # (an attached StateEstimator)
        # the sampling key and everything drawn from it are derived from the raw rng_act on the device, as for covo-online (step.hip);
        # the sampling rollouts are deterministic, as CoVO's are
        am, cov = core.step(_lib.MODE_CMA, dstate, self._params_c(env_params), control_params.a_mean, rng_act,
                            gamma_mean=control_params.gamma_mean, sample_sigma=control_params.sample_sigma,
                            want_stats=core.compute_info, derive_keys=True, rollout_deterministic=True)
        a_mean_new = am.view(self.H, 4)
        if not self.alias_outputs:
            a_mean_new, cov = a_mean_new.clone(), cov.clone()
        control_params = control_params.replace(a_mean=a_mean_new, a_cov=cov)
        out_info = core.info(dstate) if core.compute_info else {}
        out_info.update(core.step_info())  # the CMA row and whatever the step options attached (_options.py)
        return a_mean_new[0], control_params, out_info
