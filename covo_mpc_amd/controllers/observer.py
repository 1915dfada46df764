"""The force observer: a 16-state extended Kalman filter that estimates the disturbance force (csrc/force_observer.hip).

The row the env step hands a controller carries the disturbance force exactly -- the force the NEXT plant step integrates.  No flying
system measures it.  An attached ForceObserver runs one device launch in front of the control step that treats that force as unknown:
it appends it to the 13 kinematic coordinates as three random-walk states, estimates all 16 from the kinematic measurements alone
(the model of the rollouts in fp64 and the applied action a_mean[0]), and overwrites floats 0 .. 15 of the packed row in place: the 13
kinematic floats and the three force slots.  The row's own force slots are never an input.  Nothing else of the row changes, the
plant's true state is not touched, and no step path or captured step graph knows about it.

The force model is a random walk: the observer follows a force that persists (periodic, sin, mixed: a gust held for many steps) with a
lag of a few steps; a force that is redrawn every step (gaussian) cannot be predicted from its past, and the estimate is then worse than
assuming zero -- the observer removes the controller's clairvoyance there, it does not replace it.

    obs = ForceObserver(env, n_inst=1)
    obs.attach(controller)                 # any single or env-batched controller with a `core`; not next to a StateEstimator
    ...                                    # controller(...) and controller.run_episode(...) now plan from the observer's row
    obs.rows / obs.xhat / obs.force / obs.P  # device tensors: side rows [n, 8], x^ [n, 13], f^ [n, 3], covariances [n, 16, 16]
    obs.detach()
"""
from __future__ import annotations

from ._options import check_force_observer


class ForceObserver:
    """ForceObserver(env, n_inst=1, obs_std=None, proc_std=None, force_walk_std=None, force_init_std=None): the filter's constants,
    checked by _options.check_force_observer (ValueError naming the keyword).  obs_std / proc_std: four standard deviations (pos, vel,
    quat, omega); the defaults are the env step's own noise, env.default_params.obs_noise_scale (0.25, 0.5, 0.02, 0.5), and (0, 0, 0,
    0).  force_walk_std: the random walk's step in newtons per control step (default env.default_params.dyn_noise_scale: a starting
    point, not a tuned value); force_init_std: the force's standard deviation at an initialisation (default disturb_scale / sqrt(3),
    that of the U(-s, s) force a reset draws)."""

    def __init__(self, env, n_inst: int = 1, obs_std=None, proc_std=None, force_walk_std=None, force_init_std=None):
        dp = env.default_params
        self.env, self.n_inst = env, n_inst
        self._kw = dict(n_inst=n_inst, obs_std=obs_std, proc_std=proc_std, force_walk_std=force_walk_std, force_init_std=force_init_std,
                        obs_noise_scale=float(dp.obs_noise_scale), dyn_noise_scale=float(dp.dyn_noise_scale),
                        disturb_scale=float(dp.disturb_scale))
        self.record = check_force_observer(**self._kw)
        self.core = None

    def attach(self, controller):
        """Attach to `controller` (any class with a SamplingCore as `core`): its episode drivers enqueue the launch behind every env step,
        its host __call__ passes the noisy state through core.estimated.  ValueError when the controller already has a StateEstimator
        or more instances than n_inst; NotImplementedError on sample-sharded ranks and on the kernel-by-kernel path."""
        core = getattr(controller, "core", None)
        if core is None or not hasattr(core, "attach_force_observer"):
            raise TypeError(f"{type(controller).__name__} has no sampling core to attach to")
        check_force_observer(**self._kw, state_estimator=core.estimator is not None, process_group=(True if core.world > 1 else None),
                             materialize_eps=bool(getattr(controller, "materialize_eps", False)),
                             noise_stream=getattr(controller, "noise_stream", "philox"))
        if int(core._rows) > int(self.n_inst):
            raise ValueError(f"n_inst={self.n_inst}: the controller has {core._rows} instances")
        if self.core is not None:
            self.detach()
        core.attach_force_observer(self.record)
        self.core = core
        return self

    def detach(self):
        """The controller is its old self: the drivers launch nothing more, estimated() returns its argument."""
        if self.core is not None:
            self.core.detach_force_observer()
            self.core = None

    def reset(self):
        """The next launch initialises every instance from its measurement (every controller's reset() does this too)."""
        self._attached().force_observer_reset()

    def _attached(self):
        if self.core is None:
            raise RuntimeError("the force observer is not attached: call attach(controller) first")
        return self.core

    @property
    def rows(self):
        """float32 [n, 8]: every instance's side row of the last launch (a device tensor, no sync)"""
        return self._attached().obs_rows

    @property
    def xhat(self):
        """float64 [n, 13]: the kinematic estimates (a view of the device buffer, no sync)"""
        return self._attached().obs_xi[:, :13]

    @property
    def force(self):
        """float64 [n, 3]: the force estimates in newtons (a view of the device buffer, no sync)"""
        return self._attached().obs_xi[:, 13:16]

    @property
    def P(self):
        """float64 [n, 16, 16]: the covariances (the device buffer, no sync)"""
        return self._attached().obs_P
