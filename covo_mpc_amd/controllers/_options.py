"""The step options of the sampling controllers: the one place that knows their list.

Every entry point -- SamplingCore, CoVOController, MPPIController, BatchedCoVOController, BatchedMPPIController, get_controller and (under
three renames) eval_env_batched -- carries the keywords of STEP_OPTION_DEFAULTS in its signature, gathers them with take(locals()),
has them checked by check_step_options() and forwards them as **opts.  What cannot be combined is listed here too: the refusals of the
env-batched fused step (lifted by staged=True of BatchedMPPIController / BatchedCoVOController(mode="offline"): their constructors then
check with fused_batched=False; staged is a switch of those two controllers, not a step option), of sample-sharded ranks and of the
kernel-by-kernel debug path.  A new option is a keyword in those
signatures, an entry here, and its own attachment block in SamplingCore.__init__ (tests/test_options_abi.py holds the signatures to
this table).  The C side's counterpart is check_step_attachments (csrc/step_attach.hip, walked on the CPU by
tests/host/step_attach_check.cpp against tests/golden/step_refusals.txt): there a new attachment adds its setter, its check lines, and
its cases in that walk with their golden lines.

The step switches (refine, riccati, riccati_feedback, plan_hold, riccati_box) are not step options -- that list is pinned -- but have
the same home: SamplingCore, CoVOController, MPPIController (no refine), BatchedCoVOController, get_controller and eval_env_batched carry
the keywords of STEP_SWITCH_DEFAULTS, gather them with take_switches(locals()), have them checked by check_step_switches() and forward
them as **switches; the iLQR controllers take three of them through check_ilqr.  A new switch is an entry in STEP_SWITCH_DEFAULTS, a
keyword in those signatures, its check_*, and its attachment block in SamplingCore.__init__.

The annealed MPPI controllers (controllers/dial.py, BatchedDialController) are neither: like the iLQR controllers they are controllers of
their own, checked by check_dial at the end of this file, which hands SamplingCore its one anneal= record.  sigma_nodes= of the covo-online
controllers (Sigma optimised over the values of M spline nodes) is a keyword of its own too, checked by check_sigma_nodes below it.

Each option is off by default, and off changes nothing.  "info[...]" names what a single controller's __call__ then returns in its
info dict (SamplingCore.*_info: views of the core's buffers, no sync, no copy); the batched controllers expose the same buffers with
one row per instance.
"""
from __future__ import annotations

from dataclasses import dataclass

from .. import _lib

STEP_OPTION_DEFAULTS = {
    # every step also leaves its sampling diagnostics {ess, cost_min, cost_weighted, cost_mean, weight_sum, n_samples}, formed by the
    # update's own launches (covo_set_step_diag): info["ess"] / ["cost_min"] / ["cost_weighted"] / ["cost_mean"]
    "compute_diag": False,
    # every step also leaves its plan -- the rollout of the new mean itself with the step's own inputs, {cost_plan, pos_plan[H][3]} -- by
    # one extra launch behind the step (covo_set_step_plan, csrc/plan_trace.hip): info["pos_plan"] / ["cost_plan"]; an episode driver
    # records the trace with it
    "compute_plan": False,
    # the ESS floor: every step solves its temperature on the device from its own costs so that the weights' effective sample size is
    # at least ess_min (1 <= ess_min <= N / 2; lam stays the configured one whenever ESS(lam) >= ess_min already)
    # (covo_set_step_ess_floor, csrc/ess_lambda.hip): info["lam_eff"] / ["ess_lam0"]; None / 0: off
    "ess_min": None,
    # = K: every step also leaves K of its N sampled rollouts -- of the samples core.fan_idx names (pre-filled with the stride (s N) / K;
    # a caller may overwrite it between steps; the launch clamps it into [0, N)) -- by one extra launch behind the step
    # (covo_set_step_fan, csrc/sample_fan.hip): info["fan_pos"] / ["fan_cost"] / ["fan_idx"]; None / False: off
    "compute_fan": None,
    # "softmax" | "best" | "guarded".  "best" / "guarded": every step ends with the update arbiter -- the softmax mean (guarded only), the
    # shifted old mean and the best sample are rolled out with the step's own inputs and the cheapest becomes a_mean -- by one extra
    # launch behind the step and ahead of the plan / fan launches (covo_set_step_arbiter, csrc/update_arbiter.hip): info["arb_cost"] /
    # ["arb_choice"] / ["arb_best"] / ["arb_cost_chosen"]; "softmax": nothing attached
    "update": "softmax",
    # = k > 1: every control step runs k sample-rollout-update passes on its one state -- pass 0 is the plain step, pass j >= 1 starts
    # from the mean pass j - 1 committed (no shift) with the raw key split(split(key_{j-1})[0])[0], walked on the device
    # (covo_set_step_iters): info["iter_cost_min"] [k], the minimum sample cost of every pass; 1: nothing attached
    "iters": 1,
    # = K: the elite-set update, the cross-entropy method's rule -- every step (every pass of an iterated one) selects the K samples of
    # smallest key {cost, index} on the device, exactly, and updates with weight 1 on them and 0 on the rest: the new mean is their
    # average (blended by gamma_mean), MPPI with gamma_sigma != 0 refits a_cov to them (covo_set_step_elite, csrc/elite_select.hip,
    # csrc/reduce_elite.hip): info["elite_cost_max"] / ["elite_cost_min"] / ["elite_count"]; None / False / 0: off
    "elite": None,
    # = m > 1 (covo-online only): every m-th control step is the plain step and refreshes Sigma; the m - 1 between skip the Hessian and
    # the Sigma chain and sample from the previous step's factor moved one stage down the horizon on the device
    # (covo_set_step_sigma_period, csrc/sigma_shift.hip): info["sigma_age"]; 1: nothing attached
    "sigma_period": 1,
    # every step also leaves the weighted 128 x 128 covariance of its own samples under its own update's weights, centred on the mean
    # it sampled around, by two extra launches behind the step (covo_set_step_post_cov, csrc/post_cov.hip): info["post_cov"] /
    # ["post_shift"] / ["post_weight"]
    "compute_post_cov": False,
    # = gamma in (0, 1) (covo-online with sigma_period > 1): a reuse step samples from the shifted blend
    # c ((1 - gamma) S(Sigma) + gamma S(C)) of the covariance the previous step sampled from and the posterior covariance C that step
    # left (it implies compute_post_cov) (covo_set_step_sigma_adapt, csrc/sigma_adapt.hip): info["sigma_adapt_fallback"] /
    # ["sigma_adapt_scale"]; 0.0: nothing attached
    "sigma_adapt": 0.0,
}

# the step switches, in the order the signatures list them and check_step_switches checks them.  Each is off by default, and off attaches
# nothing and adds no launch; the C side's counterpart of each check_* is its block of check_step_attachments (csrc/step_attach.hip)
STEP_SWITCH_DEFAULTS = {
    # (covo-online only) every control step ends with a Newton line search on the mean it has just committed -- the gradient g of the
    # Hessian's objective at that mean (csrc/cost_gradient.hip), the direction d = -Sigma (Sigma g) / c^2 from the step's own Sigma and c,
    # the candidates clip(b + 2^(3 - j) d), j = 1 .. 16, next to clip(b) itself, judged by the step's own sampling objective
    # (covo_set_step_refine, csrc/newton_refine.hip): info["refine_cost_base"] / ["refine_cost"] / ["refine_choice"] / ["refine_alpha"] /
    # ["refine_grad_norm"] / ["refine_slope"]
    "refine": False,
    # every control step ends with the line search of refine along a direction that needs neither R nor Sigma -- the Hessian's first
    # two launches at the committed mean leave the stage blocks of the plan, a backward Riccati sweep over them (csrc/riccati.hip) gives
    # d = -(R + mu I)^-1 g on the lowest rung mu = 1e-2 4^j, j < 8, at which R + mu I is positive definite, and clip(b + 2^(3 - j) d),
    # j = 1 .. 16, compete with clip(b) under the step's own sampling objective (covo_set_step_riccati): info["riccati_cost_base"] /
    # ["riccati_cost"] / ["riccati_choice"] / ["riccati_alpha"] / ["riccati_grad_norm"] / ["riccati_slope"] / ["riccati_reg"] /
    # ["riccati_rung"].  It goes with MPPI, covo-offline, covo-online and every sigma_period, next to the step options; under iters=k
    # every pass runs it
    "riccati": False,
    # (on top of riccati) the line search behind every step judges 33 candidates instead of 17.  Candidates 0 .. 16 are riccati's own,
    # bit for bit; 16 + j, j = 1 .. 16, is the closed-loop sequence at the same step size 2^(3 - j): the sweep's feed-forward terms and
    # gains around the nonlinear plant, u_k = clip(b_k + alpha k_k + K_k (x_k - xb_k)) -- the forward pass of DDP / iLQR
    # (covo_set_step_riccati_feedback, csrc/feedback_rollout.hip).  The first cheapest wins, so a closed-loop candidate is committed only
    # when strictly cheaper than every open-loop one: info["riccati_closed"] / ["riccati_cost_open"] / ["riccati_cost_closed"] /
    # ["riccati_gain_max"]
    "riccati_feedback": False,
    # = m > 1 (on top of riccati): every m-th control step, counted from reset(), is the control step as it is (a plan step); the m - 1
    # between sample nothing -- one small launch (covo_set_step_plan_hold, csrc/plan_hold.hip) applies stage j of the law the plan step's
    # Riccati sweep left, u = clip(b_j + alpha k_j + K_j (x - xb_j)), to the measured state, shifts the mean (MPPI: and the covariances)
    # as a step's begin work does and puts u in front: info["plan_age"] (a Python int) / ["hold_gain"] / ["hold_clipped"] /
    # ["hold_flags"] / ["hold_alpha"].  It goes with iters (a plan step runs its k passes), riccati_feedback and every step option but
    # sigma_period; 1: nothing attached
    "plan_hold": 1,
    # (on top of riccati; the iLQR controllers take it too: BatchedILQRController's keyword, the class ILQRBoxController) every stage of
    # every sweep the controller runs solves the box QP of control-limited DDP instead of the unconstrained 4 x 4 system --
    # k_k = argmin 1/2 du^T Quu du + Qu^T du on -1 <= clip(b_k) + du <= 1; a clamped coordinate's k_k is the bound itself and its row of
    # K_k is 0 (covo_set_step_riccati_box, csrc/riccati.hip).  Forward pass, candidates and judge are unchanged: info["riccati_box_mask"]
    # [32] int32 (bits 0-3: coordinate i clamped at the lower bound, 4-7: at the upper) / ["riccati_box_count"] (the clamped coordinates
    # of the last sweep).  It goes with every plant, drag / mixed included: the box lives in the 4 x 4 part
    "riccati_box": False,
}


def take(namespace) -> dict:
    """The step options out of an entry point's locals(), ready to be checked and forwarded as **opts."""
    return {k: namespace[k] for k in STEP_OPTION_DEFAULTS}


def take_switches(namespace) -> dict:
    """The step switches out of an entry point's locals(), ready to be checked and forwarded as **switches.  A name the namespace lacks
    is taken at its default: MPPIController has no refine (there is no Sigma to refine with), the one entry point that lacks a switch."""
    return {k: namespace.get(k, default) for k, default in STEP_SWITCH_DEFAULTS.items()}


@dataclass(frozen=True)
class StepOptions:
    """The step options, checked and normalised (check_step_options).  fan_K / elite_K are None when N was not known yet."""
    diag: bool
    plan: bool
    ess_min: float      # 0.0: off
    fan_K: int          # 0: off
    update: str
    arb_mask: int       # the arbiter's candidate mask (0: "softmax", nothing attached)
    iters: int
    elite_K: int        # 0: off
    sigma_period: int
    post_cov: bool      # forced on by sigma_adapt > 0: a reuse step reads the previous step's posterior covariance
    sigma_adapt: float


_BATCHED_TAKES = "BatchedCoVOController(mode=\"online\") and the single controllers take "
_OR_STAGED = ", or pass staged=True (the staged batched step takes it)"
# the env-batched MPPI / covo-offline step: (is on, message); {o}: the keywords as given
FUSED_BATCHED_REFUSALS = (
    (lambda s, o: s.elite_K,
     "elite={o[elite]}: the elite-set update is not available for the env-batched MPPI / covo-offline step "
     "(one fused launch: it needs the weights before all costs exist); " + _BATCHED_TAKES + "it" + _OR_STAGED),
    (lambda s, o: s.post_cov,
     "compute_post_cov: the posterior covariance is not available for the env-batched MPPI / covo-offline "
     "step (one fused launch: it keeps the samples in LDS and never stores them); " + _BATCHED_TAKES + "it" + _OR_STAGED),
    (lambda s, o: s.iters > 1 and s.update != "softmax",
     "iters={o[iters]} with update={o[update]!r}: not available for the env-batched MPPI / covo-offline step "
     "(its fused launch keeps each pass's starting mean in LDS only); " + _BATCHED_TAKES + "both" + _OR_STAGED),
    (lambda s, o: s.ess_min != 0.0,
     "ess_min={o[ess_min]}: the ESS floor is not available for the env-batched MPPI / covo-offline step "
     "(one fused launch: it needs the temperature before all costs exist); " + _BATCHED_TAKES + "it" + _OR_STAGED),
)

# sample-sharded ranks: option -> (is on, the value the message shows as {v}, message); s: the normalised record, o: the keywords as given
SHARDED_REFUSALS = {
    "iters": (lambda s: s.iters > 1, lambda s, o: s.iters,
              "iters={v} on sample-sharded ranks: every pass would need its own exchange of the rank "
              "records (covo_set_step_iters refuses sample-sharded steps)"),
    "update": (lambda s: s.arb_mask, lambda s, o: s.update,
               "update={v!r} on sample-sharded ranks: a rank's action and cost buffers hold its shard "
               "only (covo_set_step_arbiter refuses sample-sharded steps)"),
    "compute_fan": (lambda s: s.fan_K, None,
                    "compute_fan on sample-sharded ranks: a rank's action buffer holds its shard only "
                    "(covo_set_step_fan refuses sample-sharded steps)"),
    "ess_min": (lambda s: s.ess_min != 0.0, lambda s, o: o["ess_min"],
                "ess_min={v} on sample-sharded ranks: a rank sees only its shard's costs "
                "(covo_set_step_ess_floor refuses sample-sharded steps)"),
    "elite": (lambda s: s.elite_K, lambda s, o: s.elite_K,
              "elite={v} on sample-sharded ranks: a rank sees only its shard's costs "
              "(covo_set_step_elite refuses sample-sharded steps)"),
    "sigma_period": (lambda s: s.sigma_period > 1, lambda s, o: s.sigma_period,
                     "sigma_period={v} on sample-sharded ranks: every rank would have to keep and shift "
                     "the same factor (covo_set_step_sigma_period refuses sample-sharded steps)"),
    "sigma_adapt": (lambda s: s.sigma_adapt > 0.0, lambda s, o: s.sigma_adapt,
                    "sigma_adapt={v} on sample-sharded ranks: it needs the Sigma period and the posterior "
                    "covariance (covo_set_step_sigma_adapt refuses sample-sharded steps)"),
    "compute_post_cov": (lambda s: s.post_cov, None,
                         "compute_post_cov on sample-sharded ranks: a rank's action and cost buffers hold its shard "
                         "only (covo_set_step_post_cov refuses sample-sharded steps)"),
    "compute_diag": (lambda s: s.diag, None,
                     "compute_diag on sample-sharded ranks: the rank records carry no diagnostic sums "
                     "(covo_set_step_diag refuses sample-sharded steps)"),
    "compute_plan": (lambda s: s.plan, None,
                     "compute_plan on sample-sharded ranks: a rank holds only its shard's record until the "
                     "exchange (covo_set_step_plan refuses sample-sharded steps)"),
}


def sharded_refusal(option, v=None) -> NotImplementedError:
    """The refusal of `option`, given as `v`, on sample-sharded ranks."""
    return NotImplementedError(SHARDED_REFUSALS[option][2].format(v=v))


_DEBUG_PATH = " (covo_mpc_step); the kernel-by-kernel path (materialize_eps / noise_stream='jax') "
# the kernel-by-kernel path: (core attribute, its value when off, the attribute the message shows as {v}, message).  The off value
# doubles as the default for cores that lack the attribute: the *_abi tests pass partial stand-ins of SamplingCore
KERNEL_PATH_REFUSALS = (
    ("sigma_period", 1, "sigma_period", "sigma_period={v} acts in the fused step" + _DEBUG_PATH + "computes its Sigma in every step"),
    # (the attribute: core.sigma_adapt is the stand-alone kernel's method)
    ("sigma_adapt_gamma", 0.0, "sigma_adapt_gamma", "sigma_adapt={v} acts in the fused step" + _DEBUG_PATH + "computes its Sigma in every step"),
    ("ess_min", 0.0, "ess_min", "ess_min acts in the fused step" + _DEBUG_PATH + "updates at the configured lam"),
    ("elite", 0, "elite", "elite={v} acts in the fused step" + _DEBUG_PATH + "updates with the softmax weights"),
    ("compute_plan", False, "compute_plan", "compute_plan follows the fused step" + _DEBUG_PATH + "does not produce it"),
    ("compute_fan", 0, "compute_fan", "compute_fan follows the fused step" + _DEBUG_PATH + "does not produce it"),
    ("compute_post_cov", False, "compute_post_cov", "compute_post_cov follows the fused step" + _DEBUG_PATH + "does not produce it"),
    ("arb_mask", 0, "update_rule", "update={v!r} follows the fused step" + _DEBUG_PATH + "updates with the softmax mean only"),
    ("iters", 1, "iters", "iters={v} follows the fused step" + _DEBUG_PATH + "runs one pass per call"),
    ("compute_diag", False, "compute_diag", "compute_diag is formed by the fused step" + _DEBUG_PATH + "does not produce it"),
    ("refine", False, "refine", "refine follows the fused step" + _DEBUG_PATH + "ends with the softmax mean"),
    ("riccati_on", False, "riccati_on", "riccati follows the fused step" + _DEBUG_PATH + "ends with the softmax mean"),
    ("sigma_nodes_M", None, "sigma_nodes_M", "sigma_nodes={v} acts in the fused step" + _DEBUG_PATH + "samples from the full 128 x 128 Sigma"),
)


def check_kernel_path(core) -> None:
    """NotImplementedError for the first attachment of `core` the kernel-by-kernel path cannot honour."""
    for attr, off, shown, message in KERNEL_PATH_REFUSALS:
        if getattr(core, attr, off) != off:
            raise NotImplementedError(message.format(v=getattr(core, shown)))


def check_step_options(N, what, *, gamma_sigma=None, fused_batched=False, sharded=False, **raw) -> StepOptions:
    """The step options as given (**raw: the keywords of STEP_OPTION_DEFAULTS, missing ones at their defaults) -> StepOptions, or the
    first objection, in a fixed order:
    1. each keyword's own range and mode check (_lib.check_*: ValueError).  `what` names the controller in the mode clauses: "online"
       for covo-online, the one mode that takes sigma_period / sigma_adapt.  N=None (not parsed yet) skips compute_fan and elite, the
       two that need it.  gamma_sigma (MPPI): see _lib.check_elite;
    2. fused_batched -- the env-batched MPPI / covo-offline step, one fused launch (not under the controllers' staged=True):
       NotImplementedError for elite, compute_post_cov, iters with an update other than "softmax", ess_min;
    3. sharded -- sample-sharded ranks: NotImplementedError for whatever of SHARDED_REFUSALS is on, in its order."""
    unknown = set(raw) - set(STEP_OPTION_DEFAULTS)
    if unknown:
        raise TypeError(f"check_step_options: unknown step options {sorted(unknown)}")
    o = {**STEP_OPTION_DEFAULTS, **raw}
    sigma_period = _lib.check_sigma_period(o["sigma_period"], what)
    sigma_adapt = _lib.check_sigma_adapt(o["sigma_adapt"], sigma_period, what)
    fan_K = _lib.check_fan(o["compute_fan"], N) if N is not None else None
    arb_mask = _lib.check_update(o["update"])
    iters = _lib.check_iters(o["iters"])
    elite_K = _lib.check_elite(o["elite"], N, o["ess_min"], gamma_sigma) if N is not None else None
    s = StepOptions(diag=bool(o["compute_diag"]), plan=bool(o["compute_plan"]),
                    ess_min=float(o["ess_min"]) if o["ess_min"] is not None else 0.0, fan_K=fan_K, update=o["update"],
                    arb_mask=arb_mask, iters=iters, elite_K=elite_K, sigma_period=sigma_period,
                    post_cov=bool(o["compute_post_cov"]) or sigma_adapt > 0.0, sigma_adapt=sigma_adapt)
    if fused_batched:
        for is_on, message in FUSED_BATCHED_REFUSALS:
            if is_on(s, o):
                raise NotImplementedError(message.format(o=o))
    if sharded:
        for option, (is_on, shown, _) in SHARDED_REFUSALS.items():
            if is_on(s):
                raise sharded_refusal(option, shown(s, o) if shown else None)
    return s


def check_refine(refine, what, *, sigma_period=1, sharded=False) -> bool:
    """refine= (STEP_SWITCH_DEFAULTS) -> bool.  The objections, in a fixed order: anything but a bool (ValueError); `what` other than "online" -- MPPI, covo-offline and their
    env-batched controllers have no Hessian-derived Sigma at the step's mean (ValueError); sigma_period > 1 -- a reuse step has no R,
    and its c means something else (ValueError); sharded -- sample-sharded ranks (NotImplementedError)."""
    if not isinstance(refine, bool):
        raise ValueError(f"refine={refine!r} (True | False)")
    if not refine:
        return False
    if what != "online":
        raise ValueError(f"refine=True with {what}: the Newton refinement needs the Hessian-derived Sigma at the step's mean, which "
                         "only covo-online computes (CoVOController(mode=\"online\"), BatchedCoVOController(mode=\"online\")); "
                         "give refine=False")
    if int(sigma_period) > 1:
        raise ValueError(f"refine=True with sigma_period={sigma_period}: a reuse step has no R and its c means something else; give "
                         "sigma_period=1 or refine=False")
    if sharded:
        raise NotImplementedError("refine=True on sample-sharded ranks: a rank's Sigma chain and costs cover its shard's step only "
                                  "until the exchange (covo_set_step_refine refuses sample-sharded steps)")
    return True


def check_riccati(riccati, what, *, refine=False, sharded=False) -> bool:
    """riccati= (STEP_SWITCH_DEFAULTS) -> bool.  The objections, in a fixed order: anything but a bool (ValueError); together with refine=True -- both polish the committed mean
    (ValueError); `what` one of the env-batched MPPI / covo-offline controllers, fused or staged -- their batches carry no Hessian
    constants (NotImplementedError); sharded -- sample-sharded ranks (NotImplementedError)."""
    if not isinstance(riccati, bool):
        raise ValueError(f"riccati={riccati!r} (True | False)")
    if not riccati:
        return False
    if refine:
        raise ValueError("riccati=True together with refine=True: both polish the committed mean with the same line search; give one "
                         "of them")
    if str(what).startswith("the env-batched"):
        raise NotImplementedError(f"riccati=True with {what}: the env-batched MPPI / covo-offline steps, fused or staged, carry no "
                                  "per-instance Hessian constants; run BatchedCoVOController(mode=\"online\") or single controllers")
    if sharded:
        raise NotImplementedError("riccati=True on sample-sharded ranks: a rank's costs cover its shard's step only until the exchange "
                                  "(covo_set_step_riccati refuses sample-sharded steps)")
    return True


def check_riccati_feedback(feedback, *, riccati, disturb_type=None, what="a sampling controller") -> bool:
    """riccati_feedback= (STEP_SWITCH_DEFAULTS) -> bool.  The objections, in a fixed order: anything but a bool (ValueError); True without riccati=True -- the candidates run under that
    sweep's gains (ValueError); disturb_type drag / mixed -- the 16-state plants, whose force is a state of the sweep and a per-sample
    quantity of the rollout (NotImplementedError; disturb_type=None: not known here, the step refuses it)."""
    if not isinstance(feedback, bool):
        raise ValueError(f"riccati_feedback={feedback!r} (True | False)")
    if not feedback:
        return False
    if riccati is not True:
        raise ValueError(f"riccati_feedback=True with {what} needs riccati=True: the closed-loop candidates run under the gains of "
                         "that sweep; give riccati=True or riccati_feedback=False")
    if disturb_type in ("drag", "mixed"):
        raise NotImplementedError(f"riccati_feedback=True with disturb_type={disturb_type!r}: drag / mixed are 16-state plants -- their "
                                  "force is a state of the sweep and a per-sample quantity of the rollout, and the closed-loop "
                                  "generator carries the 13-state plants only (covo_set_step_riccati_feedback refuses them at the step)")
    return True


def check_riccati_box(box, *, riccati, what="a sampling controller") -> bool:
    """riccati_box= (STEP_SWITCH_DEFAULTS) -> bool.  The objections, in a fixed order: anything but a bool (ValueError); True without riccati=True -- it is that sweep's stage problem
    (ValueError).  Whatever riccati= refuses stays refused by check_riccati."""
    if not isinstance(box, bool):
        raise ValueError(f"riccati_box={box!r} (True | False)")
    if not box:
        return False
    if riccati is not True:
        raise ValueError(f"riccati_box=True with {what} needs riccati=True: the box is the stage problem of that sweep; give "
                         "riccati=True or riccati_box=False")
    return True


def check_plan_hold(plan_hold, *, riccati, sigma_period=1, disturb_type=None, what="a sampling controller") -> int:
    """plan_hold= (STEP_SWITCH_DEFAULTS) -> the period m.  The objections, in a fixed order: anything but an integer in [1, COVO_MAX_PLAN_HOLD] (ValueError); m > 1 without riccati=True -- a
    hold step applies that sweep's gains (ValueError); m > 1 with sigma_period > 1 -- both thin out the step, and sigma_adapt goes with
    it (ValueError); disturb_type drag / mixed -- the 16-state plants, as for riccati_feedback (NotImplementedError; disturb_type=None:
    not known here, the step refuses it).  Whatever riccati= refuses stays refused by check_riccati."""
    import numbers
    if (isinstance(plan_hold, bool) or not isinstance(plan_hold, numbers.Integral) or
            not 1 <= int(plan_hold) <= _lib.COVO_MAX_PLAN_HOLD):
        raise ValueError(f"plan_hold={plan_hold!r} outside [1, {_lib.COVO_MAX_PLAN_HOLD}] (an integer number of control steps per plan; "
                         "1 = off)")
    m = int(plan_hold)
    if m == 1:
        return 1
    if riccati is not True:
        raise ValueError(f"plan_hold={m} with {what} needs riccati=True: a hold step applies the gains of that sweep; give riccati=True "
                         "or plan_hold=1")
    if int(sigma_period) > 1:
        raise ValueError(f"plan_hold={m} with sigma_period={sigma_period}: both thin out the step (and sigma_adapt goes with the Sigma "
                         "period); give one of them as 1")
    if disturb_type in ("drag", "mixed"):
        raise NotImplementedError(f"plan_hold={m} with disturb_type={disturb_type!r}: drag / mixed are 16-state plants -- their force is "
                                  "a state of the sweep, and the hold step carries the 13-state plants only "
                                  "(covo_set_step_plan_hold refuses them at the step)")
    return m


@dataclass(frozen=True)
class StepSwitches:
    """The step switches, checked (check_step_switches)."""
    refine: bool
    riccati: bool
    riccati_feedback: bool
    plan_hold: int      # 1: off
    riccati_box: bool


def check_step_switches(what, *, mode_what=None, riccati_what=None, sigma_period=1, disturb_type=None, sharded=False,
                        **raw) -> StepSwitches:
    """The step switches as given (**raw: the keywords of STEP_SWITCH_DEFAULTS, missing ones at their defaults) -> StepSwitches, or the
    first objection of check_refine, check_riccati, check_riccati_feedback, check_plan_hold, check_riccati_box, in the table's order.
    The names the messages show are the entry point's own: mode_what is the one check_refine shows and tests ("online" for covo-online;
    default: what), riccati_what the one check_riccati does (default: mode_what), `what` the one of the other three."""
    unknown = set(raw) - set(STEP_SWITCH_DEFAULTS)
    if unknown:
        raise TypeError(f"check_step_switches: unknown step switches {sorted(unknown)}")
    o = {**STEP_SWITCH_DEFAULTS, **raw}
    mode_what = what if mode_what is None else mode_what
    refine = check_refine(o["refine"], mode_what, sigma_period=sigma_period, sharded=sharded)
    riccati = check_riccati(o["riccati"], mode_what if riccati_what is None else riccati_what, refine=refine, sharded=sharded)
    feedback = check_riccati_feedback(o["riccati_feedback"], riccati=riccati, disturb_type=disturb_type, what=what)
    m = check_plan_hold(o["plan_hold"], riccati=riccati, sigma_period=sigma_period, disturb_type=disturb_type, what=what)
    box = check_riccati_box(o["riccati_box"], riccati=riccati, what=what)
    return StepSwitches(refine=refine, riccati=riccati, riccati_feedback=feedback, plan_hold=m, riccati_box=box)


def check_ilqr(iters=2, *, riccati_feedback=None, plan_hold=1, disturb_type=None, refine=False, process_group=None,
               what="the iLQR controller", riccati_box=False, **raw):
    """The keywords of the sampling-free controllers (ILQRController, BatchedILQRController, get_controller(env, "ilqr", ...),
    eval_env_batched(controller="ilqr")) -> (iters, riccati_feedback, plan_hold), checked and resolved.  The C side's counterpart is
    check_ilqr_step (csrc/step_attach.hip).

    One control step is b_0 = shift(a_mean), then iters times the Riccati line search of riccati= (with riccati_feedback: over 33
    candidates, the closed-loop forward pass of DDP / iLQR among them) on the step's one state and raw key, a_mean <- b_iters: nothing is
    sampled (COVO_MODE_ILQR, csrc/ilqr.hip).  info["ilqr_rows"] [iters, 8] / ["ilqr_feedback_rows"] [iters, 8] (every iteration's
    Riccati and feedback row) / ["ilqr_cost_first"] / ["ilqr_cost"] / ["ilqr_moved"] / ["ilqr_fixed_at"] / ["ilqr_closed"], next to the
    riccati_* keys (the last iteration) and, under plan_hold, plan_age / hold_*.  **raw: the step options (STEP_OPTION_DEFAULTS); only
    compute_plan means anything here, and iters is this function's own first argument.

    The objections, in a fixed order: iters anything but an integer in [1, COVO_MAX_STEP_ITERS] (ValueError); a sampling step option
    away from its default -- compute_diag, ess_min, compute_fan, update, elite, sigma_period, compute_post_cov, sigma_adapt, in that
    order: each acts on samples, weights or a Sigma, and there are none (ValueError naming it); refine=True -- its direction needs a
    covo-online step's Sigma (ValueError); a process_group -- there are no samples to shard (NotImplementedError); riccati_feedback
    anything but None / True / False (ValueError), True with disturb_type drag / mixed (check_riccati_feedback's NotImplementedError);
    then whatever check_plan_hold objects to; riccati_box anything but a bool (check_riccati_box's ValueError; the sweep is always
    there, so True is accepted).  riccati_feedback=None resolves to True on the 13-state plants and to False on drag /
    mixed, whose closed-loop candidates the generator refuses; an explicit False is honoured."""
    unknown = set(raw) - set(STEP_OPTION_DEFAULTS)
    if unknown:
        raise TypeError(f"check_ilqr: unknown step options {sorted(unknown)}")
    k = _lib.check_iters(iters)
    for name, default in STEP_OPTION_DEFAULTS.items():
        if name in ("iters", "compute_plan") or name not in raw:
            continue
        v = raw[name]
        off = (not v) if default is None else v == default  # (ess_min / compute_fan / elite: None, False and 0 all mean off)
        if not off:
            raise ValueError(f"{name}={v!r} with {what}: a step option of the sampling controllers -- it acts on samples, weights or a "
                             "Sigma, and an iLQR step has none; leave it at its default")
    if not isinstance(refine, bool):
        raise ValueError(f"refine={refine!r} (True | False)")
    if refine:
        raise ValueError(f"refine=True with {what}: the Newton refinement's direction needs the Sigma of a covo-online step, which an "
                         "iLQR step does not compute (its iterations are the Riccati line search already); give refine=False")
    if process_group is not None:
        raise NotImplementedError(f"a process_group with {what}: sample-sharded ranks split a step's samples, and an iLQR step has "
                                  "none; run it on one rank")
    if riccati_feedback is None:
        feedback = disturb_type not in ("drag", "mixed")
    else:
        feedback = check_riccati_feedback(riccati_feedback, riccati=True, disturb_type=disturb_type, what=what)
    m = check_plan_hold(plan_hold, riccati=True, disturb_type=disturb_type, what=what)
    check_riccati_box(riccati_box, riccati=True, what=what)  # (a bool, returned as given: the callers pass it on)
    return k, feedback, m


@dataclass(frozen=True)
class Anneal:
    """The annealed step's attachment, checked (check_dial): what SamplingCore's anneal= keyword takes."""
    sigma: object       # float32 numpy [iters, 32]: sigma[i][h] of pass i, stage h (anneal_schedule)
    temp: float         # 0.0: every pass updates at the configured lam, no solver runs
    beta_pass: float
    beta_stage: float
    # nodes=M (check_dial): the perturbations are splines over M nodes; sigma above is then the stages' marginal sigma_e [iters, 32]
    nodes: object = None        # int M in [2, 32], or None: a draw per stage
    node_interp: str = "linear"
    node_sigma: object = None   # float64 numpy [iters, M]: the schedule over the nodes (node_schedule)
    basis: object = None        # float32 numpy [iters, 32, M]: B[i][h][m] = fp32(node_sigma[i][m] weights[h][m]), what the sampler reads
    weights: object = None      # float64 numpy [32, M]: W[h][m], node m's interpolation weight at stage h (node_basis)


NODE_INTERPS = ("linear", "cubic")


def node_basis(M, interp="linear", H=_lib.COVO_H):
    """W[h][m] = phi_m(h), float64 numpy [H, M]: the value at stage h of the interpolant through the unit vector e_m on the M nodes
    t_m = m (H - 1) / (M - 1) (formed as (m * (H - 1)) / (M - 1): t_0 = 0 and t_{M-1} = H - 1 exactly).  "linear": the hat functions;
    "cubic": the cardinal functions of the natural cubic spline (second derivatives from the tridiagonal system, zero at both ends).
    Evaluated on the node interval [t_j, t_j+1] that holds h with s = (h - t_j) / (t_j+1 - t_j): a stage that is a node gets that
    node's unit vector exactly, rows sum to 1 and reproduce h (sum_m W[h][m] t_m = h) up to rounding; M = H linear is the identity."""
    import numpy as np
    M = int(M)
    if not 2 <= M <= H or interp not in NODE_INTERPS:
        raise ValueError(f"node_basis: M={M} outside [2, {H}] or interp={interp!r} not one of {NODE_INTERPS}")
    t = np.array([(m * (H - 1)) / (M - 1) for m in range(M)], dtype=np.float64)
    d = np.diff(t)
    z = np.zeros((M, M), dtype=np.float64)  # z[:, m]: the second derivatives at the nodes of the spline through e_m
    if interp == "cubic" and M > 2:
        A = np.zeros((M - 2, M - 2), dtype=np.float64)
        for r in range(M - 2):  # row r: node r + 1
            A[r, r] = 2.0 * (d[r] + d[r + 1])
            if r > 0:
                A[r, r - 1] = d[r]
            if r < M - 3:
                A[r, r + 1] = d[r + 1]
        Y = np.eye(M, dtype=np.float64)
        rhs = 6.0 * ((Y[2:] - Y[1:-1]) / d[1:, None] - (Y[1:-1] - Y[:-2]) / d[:-1, None])
        z[1:-1] = np.linalg.solve(A, rhs)
    W = np.zeros((H, M), dtype=np.float64)
    for h in range(H):
        j = min(int(np.searchsorted(t, float(h), side="right")) - 1, M - 2)
        s = (h - t[j]) / d[j]
        u = (t[j + 1] - h) / d[j]  # (not 1 - s: both ends of the interval are then exact)
        W[h, j] += u
        W[h, j + 1] += s
        W[h] += (z[j] * (u * u * u - u) + z[j + 1] * (s * s * s - s)) * (d[j] * d[j] / 6.0)
    return W


def node_schedule(sample_sigma, iters, beta_pass, beta_stage, M, interp="linear", H=_lib.COVO_H):
    """The tables of nodes=M -> (node_sigma float64 [iters, M], basis float32 [iters, H, M], sigma_e float32 [iters, H], W float64):
    node_sigma[i][m] = sample_sigma beta_pass^i beta_stage^(M - 1 - m) -- anneal_schedule's expression with the NODES in the stages'
    place --, basis[i][h][m] = fp32(node_sigma[i][m] W[h][m]) rounded once, and sigma_e[i][h] = fp32(sqrt(sum_m fp64(basis[i][h][m])^2)),
    stage h's marginal standard deviation under the ROUNDED entries.  M = H linear: basis[i] = diag(anneal_schedule(...)[i]) and
    sigma_e = that schedule, word for word (the square of an fp32 number is exact in fp64)."""
    import numpy as np
    s0, bp, bs, M = float(sample_sigma), float(beta_pass), float(beta_stage), int(M)
    W = node_basis(M, interp, H)
    node_sigma = np.array([[s0 * bp ** i * bs ** (M - 1 - m) for m in range(M)] for i in range(int(iters))], dtype=np.float64)
    basis = (node_sigma[:, None, :] * W[None, :, :]).astype(np.float32)
    sigma_e = np.sqrt((basis.astype(np.float64) ** 2).sum(axis=2)).astype(np.float32)
    return node_sigma, basis, sigma_e, W


def anneal_schedule(sample_sigma, iters, beta_pass, beta_stage, H=_lib.COVO_H):
    """sigma[i][h] = fp32(sample_sigma beta_pass^i beta_stage^(H - 1 - h)), i < iters, h < H: formed in fp64, rounded once -> float32
    numpy [iters, H].  Later passes draw from a narrower distribution; near stages of the horizon get less noise than far ones."""
    import numpy as np
    s0, bp, bs = float(sample_sigma), float(beta_pass), float(beta_stage)
    return np.array([[np.float32(s0 * bp ** i * bs ** (H - 1 - h)) for h in range(H)] for i in range(int(iters))], dtype=np.float32)


def check_dial(iters=4, *, beta_pass=0.5, beta_stage=0.9, temp=0.1, gamma_sigma=0.0, sample_sigma=0.5, materialize_eps=False,
               noise_stream="philox", what="the annealed MPPI controller", nodes=None, node_interp="linear"):
    """The keywords of the annealed MPPI controllers (DialController, BatchedDialController, get_controller(env, "dial", ...),
    eval_env_batched(controller="dial")) -> the Anneal record SamplingCore attaches, or None for the neutral element
    (beta_pass = beta_stage = 1 with temp=None: nothing is attached, the controller is MPPIController(iters=k) launch for launch).  The
    C side's counterpart is covo_set_step_anneal's block of check_step_attachments (csrc/step_attach.hip).

    One control step is iters passes of MPPI's sample-rollout-update on its one state (the key walk of iters=).  Pass i draws
    a = clip(mu_i + sigma[i][h] eps) from the schedule of anneal_schedule (control_params.a_cov on input is ignored; on output it is
    the last pass's blocks sigma[k-1][h]^2 I); with temp given the pass's temperature is temp x the population standard deviation of
    its finite costs (csrc/cost_standardise.hip), the configured lam when that is no temperature: info["anneal_sigma"] [k, 32] /
    ["anneal_rows"] [k, 4] / ["anneal_lam"] [k] / ["anneal_std"] [k] / ["anneal_fallback"] [k] bool, and with temp given
    info["lam_eff"], the last pass's.

    nodes=M (2 <= M <= 32; node_interp "linear" or "cubic"): the pass's PERTURBATIONS are splines over M nodes spread over the
    horizon -- a[h] = clip(mu_i[h] + sum_m B[i][h][m] e_m) with the tables of node_schedule (csrc/noise_nodes.hip), beta_stage running
    over the nodes -- drawn in 4 M dimensions; the mean stays the stage-space 128-vector, so nothing behind the sampler changes (unlike
    DIAL-MPC, which keeps node values and re-fits them after every shift).  Anneal.sigma, info["anneal_sigma"] and the returned a_cov
    are then the stages' marginals sigma_e -- only the 4 x 4 block diagonal of the sampled covariance (B B^T) (x) I_4 of rank 4 M;
    info gains "anneal_nodes" and "anneal_node_sigma" [k, M].  With nodes given an Anneal is always returned (also at beta = 1,
    temp=None); nodes=32 linear is nodes=None in every output value.

    The objections, in a fixed order (ValueError naming the keyword): iters anything but an integer in [1, COVO_MAX_STEP_ITERS];
    beta_pass, then beta_stage, anything but a real number in (0, 1]; temp anything but None or a finite real number > 0;
    nodes anything but None or an integer in [2, 32]; node_interp anything but "linear" or "cubic";
    gamma_sigma != 0 -- the schedule owns a_cov; then materialize_eps / noise_stream="jax" (NotImplementedError): the kernel-by-kernel
    path knows no schedule."""
    import math
    import numbers
    k = _lib.check_iters(iters)
    for name, v in (("beta_pass", beta_pass), ("beta_stage", beta_stage)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(float(v)) or not 0.0 < float(v) <= 1.0:
            raise ValueError(f"{name}={v!r} outside (0, 1] (the factor of the noise scale per "
                             f"{'pass' if name == 'beta_pass' else 'stage towards the front of the horizon'}, a real number; 1 = none)")
    if temp is not None and (isinstance(temp, bool) or not isinstance(temp, numbers.Real) or not math.isfinite(float(temp)) or
                             not float(temp) > 0.0):
        raise ValueError(f"temp={temp!r} (None, or a finite real number > 0: the pass's temperature in units of the standard deviation "
                         "of its costs)")
    if nodes is not None and (isinstance(nodes, bool) or not isinstance(nodes, numbers.Integral) or not 2 <= int(nodes) <= _lib.COVO_H):
        raise ValueError(f"nodes={nodes!r} (None, or an integer in [2, {_lib.COVO_H}]: the spline nodes the perturbations of a pass are "
                         "drawn at)")
    if node_interp not in NODE_INTERPS:
        raise ValueError(f"node_interp={node_interp!r} is not one of {NODE_INTERPS}")
    if float(gamma_sigma) != 0.0:
        raise ValueError(f"gamma_sigma={gamma_sigma} with {what}: the schedule owns a_cov, MPPI's covariance adaptation would adapt "
                         "what the next pass overwrites; give gamma_sigma=0")
    if materialize_eps or noise_stream != "philox":
        raise NotImplementedError(f"{what} acts in the fused step (covo_mpc_step); the kernel-by-kernel path (materialize_eps / "
                                  "noise_stream='jax') knows no schedule and updates at the configured lam")
    if nodes is not None:
        node_sigma, basis, sigma_e, W = node_schedule(sample_sigma, k, beta_pass, beta_stage, int(nodes), node_interp)
        return Anneal(sigma=sigma_e, temp=0.0 if temp is None else float(temp), beta_pass=float(beta_pass), beta_stage=float(beta_stage),
                      nodes=int(nodes), node_interp=node_interp, node_sigma=node_sigma, basis=basis, weights=W)
    if float(beta_pass) == 1.0 and float(beta_stage) == 1.0 and temp is None:
        return None
    return Anneal(sigma=anneal_schedule(sample_sigma, k, beta_pass, beta_stage), temp=0.0 if temp is None else float(temp),
                  beta_pass=float(beta_pass), beta_stage=float(beta_stage))


@dataclass(frozen=True)
class CMA:
    """The CMA controller's keywords, checked (check_cma): what SamplingCore.attach_cma attaches."""
    gamma: float
    step_size: bool
    damping: float
    s_min: float
    s_max: float


def check_cma(*, gamma=0.2, step_size=True, damping=1.0, s_min=0.1, s_max=4.0, sigma_period=1, sigma_adapt=0.0, sigma_nodes=None,
              refine=False, riccati=False, riccati_feedback=False, plan_hold=1, riccati_box=False, process_group=None,
              materialize_eps=False, noise_stream="philox", what="the CMA controller") -> CMA:
    """The keywords of the CMA controllers (CMAController, BatchedCMAController, get_controller(env, "cma", ...),
    eval_env_batched(controller="cma")) -> the CMA record SamplingCore.attach_cma attaches.  The C side's counterpart is check_cma_step
    (csrc/step_attach.hip).

    Every control step but the first of an episode adapts a full 128 x 128 sampling covariance to the previous step's samples: the shape
    is sigma_adapt's blend c ((1 - gamma) S(L L^T) + gamma S(C)) at log det = 2 n log sample_sigma (csrc/sigma_adapt.hip as it is), the
    step size s follows cumulative step-size adaptation on the whitened mean displacement (csrc/cma_path.hip), and the step samples from
    s^2 times the shape: info["cma_scale"] / ["cma_path_norm"] / ["cma_mu_eff"] / ["cma_flags"] / ["cma_rows"] [8].  step_size=False
    keeps s = 1.  It implies compute_post_cov and compute_diag and goes with compute_plan, compute_fan, update=, ess_min, elite and iters.

    The objections, in a fixed order, each naming the keyword: sigma_period > 1, sigma_adapt > 0, sigma_nodes, refine, then riccati,
    riccati_feedback, plan_hold > 1 and riccati_box (ValueError: the controller decides its own Sigma every step and keeps no Hessian);
    gamma anything but a real number in [0, 1), step_size anything but a bool, damping anything but a finite real number > 0, s_min /
    s_max anything but finite real numbers with 0 < s_min <= 1 <= s_max (ValueError); then process_group (NotImplementedError: a
    sample-sharded step has neither the posterior covariance nor the diagnostics) and the kernel-by-kernel path, materialize_eps /
    noise_stream="jax" (NotImplementedError: it keeps no factor between steps)."""
    import math
    import numbers
    if int(sigma_period) != 1:
        raise ValueError(f"sigma_period={sigma_period} with {what}: it adapts its covariance every step and never refreshes one; give "
                         "sigma_period=1")
    if float(sigma_adapt) != 0.0:
        raise ValueError(f"sigma_adapt={sigma_adapt} with {what}: the controller runs that blend itself, at gamma=; give sigma_adapt=0")
    if sigma_nodes is not None:
        raise ValueError(f"sigma_nodes={sigma_nodes} with {what}: the node-space Sigma is derived from a Hessian, which this controller "
                         "never forms; give sigma_nodes=None")
    if refine is not False:
        raise ValueError(f"refine={refine!r} with {what}: the Newton refinement needs the Hessian-derived Sigma of covo-online; give "
                         "refine=False")
    for name, v, off in (("riccati", riccati, False), ("riccati_feedback", riccati_feedback, False), ("plan_hold", plan_hold, 1),
                         ("riccati_box", riccati_box, False)):
        if v != off or isinstance(v, bool) != isinstance(off, bool):
            raise ValueError(f"{name}={v!r} with {what}: the Riccati switches belong to the sampling controllers with a Hessian path "
                             f"(MPPI, covo-offline, covo-online, ilqr); give {name}={off!r}")

    def real(v):
        return not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))
    if not real(gamma) or not 0.0 <= float(gamma) < 1.0:
        raise ValueError(f"gamma={gamma!r} outside [0, 1) (the weight of the previous step's posterior covariance in the shape, a real "
                         "number; 0 = the shape only shifts)")
    if not isinstance(step_size, bool):
        raise ValueError(f"step_size={step_size!r} (True | False)")
    if not real(damping) or not float(damping) > 0.0:
        raise ValueError(f"damping={damping!r} (a finite real number > 0: the factor on the step-size damping d_sigma)")
    if not real(s_min) or not real(s_max) or not 0.0 < float(s_min) <= 1.0 <= float(s_max):
        raise ValueError(f"s_min={s_min!r}, s_max={s_max!r}: the step size's bounds relative to sample_sigma must be finite real numbers "
                         "with 0 < s_min <= 1 <= s_max")
    if process_group is not None:
        raise NotImplementedError(f"process_group with {what}: a sample-sharded step has neither the posterior covariance nor the "
                                  "diagnostics the next step adapts to (covo_set_step_post_cov and covo_set_step_diag refuse "
                                  "sample-sharded steps)")
    if materialize_eps or noise_stream != "philox":
        raise NotImplementedError(f"{what} acts in the fused step (covo_mpc_step); the kernel-by-kernel path (materialize_eps / "
                                  "noise_stream='jax') keeps no factor between steps")
    return CMA(gamma=float(gamma), step_size=step_size, damping=float(damping), s_min=float(s_min), s_max=float(s_max))


@dataclass(frozen=True)
class SigmaNodes:
    """covo-online in node space, checked (check_sigma_nodes): what SamplingCore's sigma_nodes= keyword resolves to."""
    M: int              # nodes, 2 .. COVO_SIGMA_NODES_MAX; d = 4 M
    node_interp: str
    weights: object     # float64 numpy [32, M]: W[h][m] (node_basis)


def check_sigma_nodes(sigma_nodes, node_interp="linear", *, what="online", sigma_period=1, sigma_adapt=0.0, refine=False, sharded=False):
    """sigma_nodes= of the covo-online controllers (CoVOController(mode="online"), BatchedCoVOController(mode="online"), SamplingCore)
    -> the SigmaNodes record, or None for off.  Neither a step option nor a step switch -- both tables are pinned --: a keyword of its
    own, off by default, and off attaches nothing.  The C side's counterpart is covo_set_step_sigma_nodes' block of
    check_step_attachments (csrc/step_attach.hip).

    = M: every covo-online step (every pass under iters=k) samples from the optimal covariance of the NODE-parameterised problem
    J(mu + (W (x) I_4) e), W = node_basis(M, node_interp): R_M = P^T R P (d = 4 M), Sigma_M = optimize_sigma(R_M) in d dimensions
    (log det Sigma_M = 2 d log sample_sigma: sample_sigma is the scale of a node value, as for dial's nodes=M), a = clip(mu + P L_M eps)
    with eps the first M normal4 of the step's stream -- one launch of one workgroup per instance in the place of the Sigma chain and
    its finalize launch (csrc/sigma_nodes.hip).  control_params.a_cov is then P Sigma_M P^T, of rank d.  info["sigma_nodes"] (M) /
    ["sigma_node_cov"] float64 [d, d] / ["sigma_node_rows"] [8] = {lam_min, lam_max of R_M, largest, smallest eigenvalue of Sigma_M,
    log det Sigma_M, sweeps, flags, d}; flags != 0: that step fell back to sigma^2 I_d (R_M not finite 1, no convergence 2, pivot 4).
    It goes with compute_diag, compute_plan, compute_fan, update=, ess_min, elite, iters, compute_post_cov and riccati with its switches.

    The objections, in a fixed order: sigma_nodes anything but None or an integer in [2, COVO_SIGMA_NODES_MAX] (ValueError);
    node_interp anything but "linear" or "cubic" (ValueError, checked as given, also with sigma_nodes=None); `what` other than "online"
    -- MPPI, covo-offline, dial and ilqr form no Hessian per step (ValueError); sigma_period > 1, then sigma_adapt > 0 -- a reuse step
    shifts a 128 x 128 factor and there is none --, then refine=True -- its direction needs the full-rank Sigma (ValueError); sharded --
    sample-sharded ranks (NotImplementedError).  The kernel-by-kernel path (materialize_eps / noise_stream='jax') refuses it at the call
    (check_kernel_path: NotImplementedError)."""
    import numbers
    top = _lib.COVO_SIGMA_NODES_MAX
    if sigma_nodes is not None and (isinstance(sigma_nodes, bool) or not isinstance(sigma_nodes, numbers.Integral) or
                                    not 2 <= int(sigma_nodes) <= top):
        raise ValueError(f"sigma_nodes={sigma_nodes!r} (None, or an integer in [2, {top}]: the spline nodes whose 4 M values the sampling "
                         "covariance is optimised over)")
    if node_interp not in NODE_INTERPS:
        raise ValueError(f"node_interp={node_interp!r} is not one of {NODE_INTERPS}")
    if sigma_nodes is None:
        return None
    M = int(sigma_nodes)
    if what != "online":
        raise ValueError(f"sigma_nodes={M} with {what}: the node-space Sigma is derived from the Hessian at the step's mean, which only "
                         "covo-online forms (CoVOController(mode=\"online\"), BatchedCoVOController(mode=\"online\")); give "
                         "sigma_nodes=None")
    if int(sigma_period) > 1:
        raise ValueError(f"sigma_nodes={M} with sigma_period={sigma_period}: a reuse step shifts the 128 x 128 factor of the previous "
                         "step, and a node-space step leaves none; give sigma_period=1 or sigma_nodes=None")
    if float(sigma_adapt) > 0.0:
        raise ValueError(f"sigma_nodes={M} with sigma_adapt={sigma_adapt}: it belongs to the reuse steps of a Sigma period; give "
                         "sigma_adapt=0 or sigma_nodes=None")
    if refine is True:
        raise ValueError(f"sigma_nodes={M} with refine=True: the Newton refinement's direction needs the full-rank Sigma, and this one "
                         f"has rank {4 * M}; give refine=False (riccati=True needs no Sigma) or sigma_nodes=None")
    if sharded:
        raise NotImplementedError(f"sigma_nodes={M} on sample-sharded ranks: covo_set_step_sigma_nodes refuses sample-sharded steps")
    return SigmaNodes(M=M, node_interp=node_interp, weights=node_basis(M, node_interp))


@dataclass(frozen=True)
class Estimator:
    """What check_estimator returns: the four measurement and the four process standard deviations (pos, vel, quat, omega; a negative
    velocity entry of proc_std: derive it from force_std and the instance's own dt and m) and force_std."""
    obs_std: tuple
    proc_std: tuple
    force_std: float


OBS_GROUP_SCALE = (0.25, 0.5, 0.02, 0.5)  # the env step's noise on pos, vel, quat, omega per unit obs_noise_scale (quadrotor.py:356-361)


def check_estimator(*, n_inst=1, obs_std=None, proc_std=None, force_std=None, obs_noise_scale=0.05, dyn_noise_scale=0.05,
                    process_group=None, materialize_eps=False, noise_stream="philox", what="the state estimator") -> Estimator:
    """The keywords of controllers.StateEstimator -> the Estimator record SamplingCore.attach_estimator attaches.  The C side's
    counterpart is estimator_fill_model (csrc/state_estimator.hip).

    obs_std=None: obs_noise_scale (0.25, 0.5, 0.02, 0.5), the env step's own noise; proc_std=None: (0, derive, 0, 0), the velocity
    allowance dt force_std / m of a force the model does not know; force_std=None: dyn_noise_scale.

    The objections, each naming the keyword: n_inst anything but an integer in [1, COVO_MAX_ENVS]; obs_std anything but four positive
    finite real numbers; proc_std anything but four finite real numbers >= 0 (the velocity entry may be negative: derive); force_std
    anything but a finite real number >= 0 (ValueError); then process_group (NotImplementedError: sample-sharded ranks) and the
    kernel-by-kernel path, materialize_eps / noise_stream="jax" (NotImplementedError)."""
    import math
    import numbers

    def real(v):
        return not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))

    def four(v):
        try:
            v = tuple(v)
        except TypeError:
            return None
        return v if len(v) == 4 and all(real(x) for x in v) else None
    if isinstance(n_inst, bool) or not isinstance(n_inst, numbers.Integral) or not 1 <= int(n_inst) <= _lib.COVO_MAX_ENVS:
        raise ValueError(f"n_inst={n_inst!r} with {what}: an integer in [1, {_lib.COVO_MAX_ENVS}]")
    obs = tuple(float(obs_noise_scale) * g for g in OBS_GROUP_SCALE) if obs_std is None else four(obs_std)
    if obs is None or not all(float(x) > 0.0 for x in obs):
        raise ValueError(f"obs_std={obs_std!r} with {what}: four positive finite standard deviations (pos, vel, quat, omega), or None for "
                         "the env step's own")
    proc = (0.0, -1.0, 0.0, 0.0) if proc_std is None else four(proc_std)
    if proc is None or any(float(x) < 0.0 for i, x in enumerate(proc) if i != 1):
        raise ValueError(f"proc_std={proc_std!r} with {what}: four finite standard deviations >= 0 (pos, vel, quat, omega; a negative "
                         "velocity entry derives dt force_std / m), or None")
    fs = float(dyn_noise_scale) if force_std is None else force_std
    if not real(fs) or float(fs) < 0.0:
        raise ValueError(f"force_std={force_std!r} with {what}: a finite standard deviation >= 0 in newtons, or None for dyn_noise_scale")
    if process_group is not None:
        raise NotImplementedError(f"process_group with {what}: covo_set_step_estimator refuses sample-sharded steps")
    if materialize_eps or noise_stream != "philox":
        raise NotImplementedError(f"{what} on the kernel-by-kernel path (materialize_eps / noise_stream={noise_stream!r}): it is "
                                  "attached to the fused step's controllers")
    return Estimator(obs_std=tuple(float(x) for x in obs), proc_std=tuple(float(x) for x in proc), force_std=float(fs))


@dataclass(frozen=True)
class Observer:
    """What check_force_observer returns: the four measurement and the four process standard deviations (pos, vel, quat, omega), the
    force's random-walk step and its initial standard deviation, in newtons."""
    obs_std: tuple
    proc_std: tuple
    force_walk_std: float
    force_init_std: float


def check_force_observer(*, n_inst=1, obs_std=None, proc_std=None, force_walk_std=None, force_init_std=None, obs_noise_scale=0.05,
                         dyn_noise_scale=0.05, disturb_scale=0.2, state_estimator=False, process_group=None, materialize_eps=False,
                         noise_stream="philox", what="the force observer") -> Observer:
    """The keywords of controllers.ForceObserver -> the Observer record SamplingCore.attach_force_observer attaches.  The C side's
    counterpart is observer_fill_model (csrc/force_observer.hip).

    obs_std=None: obs_noise_scale (0.25, 0.5, 0.02, 0.5), the env step's own noise, as check_estimator resolves it; proc_std=None:
    (0, 0, 0, 0); force_walk_std=None: dyn_noise_scale newtons per step (a starting point, not a tuned value); force_init_std=None:
    disturb_scale / sqrt(3), the standard deviation of the U(-s, s) force a reset draws.

    The objections, each naming the keyword: n_inst anything but an integer in [1, COVO_MAX_ENVS]; obs_std anything but four positive
    finite real numbers; proc_std anything but four finite real numbers >= 0; force_walk_std / force_init_std anything but a finite
    real number >= 0; state_estimator: the controller already has a StateEstimator (ValueError); then process_group
    (NotImplementedError: sample-sharded ranks) and the kernel-by-kernel path, materialize_eps / noise_stream="jax"
    (NotImplementedError)."""
    import math
    import numbers

    def real(v):
        return not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))

    def four(v):
        try:
            v = tuple(v)
        except TypeError:
            return None
        return v if len(v) == 4 and all(real(x) for x in v) else None
    if isinstance(n_inst, bool) or not isinstance(n_inst, numbers.Integral) or not 1 <= int(n_inst) <= _lib.COVO_MAX_ENVS:
        raise ValueError(f"n_inst={n_inst!r} with {what}: an integer in [1, {_lib.COVO_MAX_ENVS}]")
    obs = tuple(float(obs_noise_scale) * g for g in OBS_GROUP_SCALE) if obs_std is None else four(obs_std)
    if obs is None or not all(float(x) > 0.0 for x in obs):
        raise ValueError(f"obs_std={obs_std!r} with {what}: four positive finite standard deviations (pos, vel, quat, omega), or None for "
                         "the env step's own")
    proc = (0.0, 0.0, 0.0, 0.0) if proc_std is None else four(proc_std)
    if proc is None or any(float(x) < 0.0 for x in proc):
        raise ValueError(f"proc_std={proc_std!r} with {what}: four finite standard deviations >= 0 (pos, vel, quat, omega), or None")
    fw = float(dyn_noise_scale) if force_walk_std is None else force_walk_std
    if not real(fw) or float(fw) < 0.0:
        raise ValueError(f"force_walk_std={force_walk_std!r} with {what}: a finite standard deviation >= 0 in newtons per step, or None "
                         "for dyn_noise_scale")
    fi = abs(float(disturb_scale)) / math.sqrt(3.0) if force_init_std is None else force_init_std
    if not real(fi) or float(fi) < 0.0:
        raise ValueError(f"force_init_std={force_init_std!r} with {what}: a finite standard deviation >= 0 in newtons, or None for "
                         "disturb_scale / sqrt(3)")
    if state_estimator:
        raise ValueError(f"{what} on a controller that already has a StateEstimator attached (state_estimator): two filters must not "
                         "write one row -- detach it first")
    if process_group is not None:
        raise NotImplementedError(f"process_group with {what}: covo_set_step_force_observer refuses sample-sharded steps")
    if materialize_eps or noise_stream != "philox":
        raise NotImplementedError(f"{what} on the kernel-by-kernel path (materialize_eps / noise_stream={noise_stream!r}): it is "
                                  "attached to the fused step's controllers")
    return Observer(obs_std=tuple(float(x) for x in obs), proc_std=tuple(float(x) for x in proc), force_walk_std=float(fw),
                    force_init_std=float(fi))
