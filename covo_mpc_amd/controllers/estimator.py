"""The state estimator: an extended Kalman filter between the env step and the control step (csrc/state_estimator.hip).

Every controller plans from the noisy copy of the state the env step hands it.  An attached StateEstimator runs one device launch in
front of the control step that replaces, in place, the 13 kinematic floats (pos, vel, quat, omega) of that packed row by the filter's
estimate: the model of the rollouts in fp64, the applied action a_mean[0], and the force that acted during the step, which the noisy
row carries exactly.  Nothing else of the row changes, and no step path or captured step graph knows about it.

    est = StateEstimator(env, n_inst=1)
    est.attach(controller)       # any single or env-batched controller with a `core`
    ...                          # controller(...) and controller.run_episode(...) now plan from the estimate
    est.rows / est.xhat / est.P  # device tensors: the side rows [n, 8], the estimates [n, 13], the covariances [n, 13, 13]
    est.detach()
"""
from __future__ import annotations

from ._options import check_estimator


class StateEstimator:
    """StateEstimator(env, n_inst=1, obs_std=None, proc_std=None, force_std=None): the filter's constants, checked by
    _options.check_estimator (ValueError naming the keyword).  obs_std / proc_std: four standard deviations (pos, vel, quat, omega);
    the defaults are the env step's own noise, env.default_params.obs_noise_scale (0.25, 0.5, 0.02, 0.5), and (0, dt force_std / m, 0,
    0) with force_std = env.default_params.dyn_noise_scale and each instance's own dt and m."""

    def __init__(self, env, n_inst: int = 1, obs_std=None, proc_std=None, force_std=None):
        dp = env.default_params
        self.env, self.n_inst = env, n_inst
        self._kw = dict(n_inst=n_inst, obs_std=obs_std, proc_std=proc_std, force_std=force_std,
                        obs_noise_scale=float(dp.obs_noise_scale), dyn_noise_scale=float(dp.dyn_noise_scale))
        self.record = check_estimator(**self._kw)
        self.core = None

    def attach(self, controller):
        """Attach to `controller` (any class with a SamplingCore as `core`): its episode drivers enqueue the launch behind every env step,
        its host __call__ passes the noisy state through core.estimated.  NotImplementedError on sample-sharded ranks and on the
        kernel-by-kernel path; ValueError when the controller has more instances than n_inst."""
        core = getattr(controller, "core", None)
        if core is None or not hasattr(core, "attach_estimator"):
            raise TypeError(f"{type(controller).__name__} has no sampling core to attach to")
        check_estimator(**self._kw, process_group=(True if core.world > 1 else None),
                        materialize_eps=bool(getattr(controller, "materialize_eps", False)),
                        noise_stream=getattr(controller, "noise_stream", "philox"))
        if int(core._rows) > int(self.n_inst):
            raise ValueError(f"n_inst={self.n_inst}: the controller has {core._rows} instances")
        if self.core is not None:
            self.detach()
        core.attach_estimator(self.record)
        self.core = core
        return self

    def detach(self):
        """The controller is its old self: the drivers launch nothing more, estimated() returns its argument."""
        if self.core is not None:
            self.core.detach_estimator()
            self.core = None

    def reset(self):
        """The next launch initialises every instance from its measurement (every controller's reset() does this too)."""
        self._attached().estimator_reset()

    def _attached(self):
        if self.core is None:
            raise RuntimeError("the estimator is not attached: call attach(controller) first")
        return self.core

    @property
    def rows(self):
        """float32 [n, 8]: every instance's side row of the last launch (a device tensor, no sync)"""
        return self._attached().est_rows

    @property
    def xhat(self):
        """float64 [n, 13]: the estimates (a view of the device buffer, no sync)"""
        return self._attached().est_xhat[:, :13]

    @property
    def P(self):
        """float64 [n, 13, 13]: the covariances (the device buffer, no sync)"""
        return self._attached().est_P
