"""Annealed MPPI: the k passes of a control step under a per-pass noise schedule and weights on standardised costs.

The scheme of DIAL-MPC on MPPI's own step (controllers/mppi.py, csrc/step.hip): pass i of a step's iters=k passes samples
a = clip(mu_i + sigma[i][h] eps), sigma[i][h] = sample_sigma beta_pass^i beta_stage^(31 - h) -- later passes draw from a narrower
distribution around the mean the earlier ones found, near stages of the horizon get less noise than far ones -- and, with temp given,
updates at the temperature temp x std of the pass's own finite costs (csrc/cost_standardise.hip).  Epsilon, the key walk and the
starting means are those of MPPIController(iters=k); beta_pass = beta_stage = 1 with temp=None attaches nothing and IS that
controller.  nodes=M draws the perturbations of a pass as splines over M nodes spread over the horizon (csrc/noise_nodes.hip;
node_interp "linear" or "cubic"), with beta_stage running over the nodes; the mean stays the stage-space 128-vector -- unlike the
published scheme, which keeps node values and re-fits them after every shift, only the PERTURBATIONS are splines here, so there is no
re-fit loss and no second update path.  nodes=32 linear is nodes=None in every output value.  Not taken from the scheme: node-space
means, the nominal as an extra sample (update="guarded" is the project's counterpart), covo modes (controllers/_options.py:
check_dial).
"""
from __future__ import annotations

from .base import BaseController
from .mppi import MPPIController, MPPIParams  # noqa: F401  (the control parameters are MPPI's)
from ._core import SamplingCore
from ._options import check_dial, check_step_options


class DialController(MPPIController):
    """MPPIController's call signature and return triple, reset and run_episode.  control_params.a_cov on input is ignored (the
    schedule owns it); the returned one holds the last pass's blocks sigma[k-1][h]^2 I (under nodes=M: the marginals sigma_e[k-1][h]^2 I,
    the block diagonal of a covariance of rank 4 M).  control_params.gamma_sigma must be 0."""

    def __init__(self, env, control_params: MPPIParams, N: int, H: int, lam: float, *, iters: int = 4, beta_pass: float = 0.5,
                 beta_stage: float = 0.9, temp=0.1, device=None, compute_info: bool = True, propagate_nan=None,
                 compute_diag: bool = False, compute_plan: bool = False, compute_fan=None, update: str = "softmax",
                 compute_post_cov: bool = False, nodes=None, node_interp: str = "linear") -> None:
        opts = dict(compute_diag=compute_diag, compute_plan=compute_plan, compute_fan=compute_fan, update=update, iters=iters,
                    compute_post_cov=compute_post_cov)
        # ValueError before anything is built
        self.anneal = check_dial(iters, beta_pass=beta_pass, beta_stage=beta_stage, temp=temp,
                                 gamma_sigma=getattr(control_params, "gamma_sigma", 0.0),
                                 sample_sigma=getattr(control_params, "sample_sigma", 0.5), nodes=nodes, node_interp=node_interp)
        check_step_options(N, "MPPI", gamma_sigma=0.0, **opts)
        BaseController.__init__(self, env, control_params)
        self.N, self.H, self.lam = N, H, lam
        self.iters, self.beta_pass, self.beta_stage, self.temp = int(iters), float(beta_pass), float(beta_stage), temp
        self.nodes, self.node_interp = nodes, node_interp
        self.materialize_eps = False  # (the kernel-by-kernel path knows no schedule: __call__ refuses it)
        self.noise_stream = "philox"
        self.alias_outputs = False
        self._params_c(env.default_params)  # raises now if env.reward_fn / disturb_type is not one the kernels evaluate
        self.core = SamplingCore(N, H, lam, control_params.discount, device=device, compute_info=compute_info, trust_clipped=True,
                                 propagate_nan=propagate_nan, anneal=self.anneal, **opts)

    def _check_gamma_sigma(self, control_params):
        """Every call: the schedule of a controller is fixed at construction (the table, the captured graphs), so the control
        parameters of a call must still be the ones it was formed from."""
        if self.anneal is None:
            return super()._check_gamma_sigma(control_params)
        check_dial(self.iters, beta_pass=self.beta_pass, beta_stage=self.beta_stage, temp=self.temp,
                   gamma_sigma=control_params.gamma_sigma, sample_sigma=control_params.sample_sigma,
                   materialize_eps=self.materialize_eps, noise_stream=self.noise_stream)  # (nodes= / node_interp= were checked at
        # construction and cannot change; handing them over would rebuild the node tables, ~100 us of numpy, on every call)
        if float(control_params.sample_sigma) != float(self.init_control_params.sample_sigma):
            raise ValueError(f"sample_sigma={control_params.sample_sigma}: the schedule of this controller was formed from "
                             f"sample_sigma={self.init_control_params.sample_sigma} at construction; build another controller")
