// step_attach.hip -- the attachment layer of the C ABI: everything a step checks before it launches (the seven check_* functions,
// called from capi.hip) and the extern "C" setters that only record on the handle what is attached.  Host code only: no kernel, no HIP
// runtime call and no launch in here -- a setter that allocates, copies, synchronises or reads the device status lives in capi.hip.
// tests/host/step_attach_check.cpp compiles this file with stubs for covo_set_error, exchange_ready and batch_small_refusal and walks
// every refusal, the documented order of each function and every setter's epoch / log / schedule bookkeeping under a sanitizer,
// against tests/golden/step_refusals.txt.  A new attachment adds its setter, its check lines, and its cases there plus the golden.
#include <cstdint>
#include <cstring>
#include "covo_common.hpp"

// reward / disturbance selectors of covo_env_params
int check_model(const covo_env_params *p, const char *what)
{
    if (p->reward_kind != COVO_REWARD_PENYAW && p->reward_kind != COVO_REWARD_REALWORLD) {
        covo_set_error("%s: reward_kind=%d (COVO_REWARD_*)", what, p->reward_kind);
        return COVO_E_BADARG;
    }
    if (p->disturb_kind < COVO_DISTURB_NONE || p->disturb_kind > COVO_DISTURB_MIXED) {
        covo_set_error("%s: disturb_kind=%d (COVO_DISTURB_*)", what, p->disturb_kind);
        return COVO_E_BADARG;
    }
    if (covo_needs_tables(*p) && p->disturb_period <= 0) {
        covo_set_error("%s: disturb_period=%d", what, p->disturb_period);
        return COVO_E_BADARG;
    }
    return 0;
}

// ---- what a step checks about everything attached to its handle -- diagnostics, plan / trace, sample fan, update arbiter, ESS floor,
// iterations, elite set -- for every entry point alike (covo_mpc_step, covo_run_episode and, through check_batch_step, the four env-batched
// ones): a step of n_samples samples for n_inst instances.  The order is fixed: first what a sample-sharded step
// (partial_out != NULL) cannot have at all, in the order above; then, in the same order, each attachment's own ranges and the rows
// of its buffer.  A new attachment adds its lines here (and its log to covo_eplog_kinds, covo_common.hpp), nowhere else.
int check_step_attachments(const covo_ctx *h, int n_samples, int n_inst, bool sharded, int derive_keys, int mode, const float *a_cov,
                           const covo_env_params *params, const char *what, float gamma_sigma, bool fused_batch)
{
    if (sharded) {
        REQUIRE(covo_diag_target(h) == nullptr,
                "%s: sampling diagnostics (covo_set_step_diag / covo_set_episode_diag_log) are not available for sample-sharded "
                "steps (partial_out != NULL): the rank records carry no diagnostic sums; detach the buffer", what);
        REQUIRE(!covo_plan_on(h),
                "%s: the plan / episode trace (covo_set_step_plan / covo_set_episode_trace) is not available for sample-sharded "
                "steps (partial_out != NULL): a rank holds only its shard's record until the exchange; detach the buffer", what);
        REQUIRE(!covo_fan_on(h),
                "%s: the sample fan (covo_set_step_fan / covo_set_episode_fan) is not available for sample-sharded steps "
                "(partial_out != NULL): a rank's action buffer holds its shard only; detach the buffer", what);
        REQUIRE(!covo_arb_on(h),
                "%s: the update arbiter (covo_set_step_arbiter) is not available for sample-sharded steps (partial_out != NULL): "
                "a rank's action and cost buffers hold its shard only; detach it", what);
        REQUIRE(!covo_ess_on(h),
                "%s: the ESS floor (covo_set_step_ess_floor, ess_min=%g) is not available for sample-sharded steps (partial_out != NULL): "
                "a rank sees only its shard's costs; turn it off (ess_min = 0)", what, (double)h->ess_min);
        REQUIRE(covo_step_iters(h) == 1,
                "%s: iterations per step (covo_set_step_iters, iters=%d) are not available for sample-sharded steps (partial_out != NULL): "
                "every pass would need its own exchange of the rank records; set iters = 1", what, covo_step_iters(h));
        REQUIRE(covo_elite_target(h) == nullptr,
                "%s: the elite-set update (covo_set_step_elite, K=%d) is not available for sample-sharded steps (partial_out != NULL): "
                "a rank sees only its shard's costs; turn it off (K = 0)", what, h->elite_K);
        REQUIRE(covo_sigma_period(h) == 1,
                "%s: the Sigma period (covo_set_step_sigma_period, period=%d) is not available for sample-sharded steps (partial_out != NULL): "
                "every rank would have to keep and shift the same factor; set period = 1", what, covo_sigma_period(h));
        REQUIRE(!covo_post_cov_on(h),
                "%s: the posterior covariance (covo_set_step_post_cov) is not available for sample-sharded steps (partial_out != NULL): "
                "a rank's action and cost buffers hold its shard only; detach the buffer", what);
        REQUIRE(!covo_sigma_adapt_on(h),
                "%s: Sigma adapt (covo_set_step_sigma_adapt, gamma=%g) is not available for sample-sharded steps (partial_out != NULL): "
                "it needs the Sigma period and the posterior covariance, which sample-sharded steps cannot have; turn it off (gamma = 0)",
                what, (double)h->adapt_gamma);
        REQUIRE(!covo_refine_on(h),
                "%s: the Newton refinement (covo_set_step_refine) is not available for sample-sharded steps (partial_out != NULL): "
                "a rank's Sigma chain and costs cover its shard's step only until the exchange; detach it", what);
        REQUIRE(!covo_riccati_on(h),
                "%s: the Riccati refinement (covo_set_step_riccati) is not available for sample-sharded steps (partial_out != NULL): "
                "a rank's costs cover its shard's step only until the exchange; detach it", what);
        REQUIRE(!covo_eprow_any(h),
                "%s: the episode logs of the attachments' rows (covo_set_episode_rows) are not available for sample-sharded steps "
                "(partial_out != NULL): none of the attachments they follow is; detach them", what);
    }
    REQUIRE(covo_diag_target(h) == nullptr || n_inst <= covo_diag_capacity(h),
            "%s: %d instances, the diagnostic buffer (covo_set_step_diag) has %d rows", what, n_inst, covo_diag_capacity(h));
    REQUIRE(h->plan_out == nullptr || n_inst <= h->plan_n, "%s: %d instances, the plan buffer (covo_set_step_plan) has %d rows", what,
            n_inst, h->plan_n);
    if (covo_fan_on(h)) {
        REQUIRE(h->fan_K <= n_samples, "%s: the sample fan (covo_set_step_fan) has K=%d > n_samples=%d", what, h->fan_K, n_samples);
        REQUIRE(n_inst <= h->fan_n, "%s: %d instances, the fan buffer (covo_set_step_fan) has n_inst=%d", what, n_inst, h->fan_n);
    }
    REQUIRE(!covo_arb_on(h) || n_inst <= h->arb_n, "%s: %d instances, the arbiter buffer (covo_set_step_arbiter) has n_inst=%d", what,
            n_inst, h->arb_n);
    if (covo_ess_on(h)) {  // ess_min in the range the solver's bracket covers
        REQUIRE(h->ess_min >= 1.0f && h->ess_min <= 0.5f * (float)n_samples,
                "%s: ess_min=%g (covo_set_step_ess_floor) outside [1, n_samples / 2 = %g]", what, (double)h->ess_min, 0.5 * n_samples);
        REQUIRE(n_inst <= covo_lam_capacity(h), "%s: %d instances, the temperature buffer (covo_set_step_ess_floor) has %d rows", what,
                n_inst, covo_lam_capacity(h));
    }
    if (covo_elite_target(h) != nullptr) {
        REQUIRE(!covo_ess_on(h),
                "%s: the elite-set update (covo_set_step_elite, K=%d) together with the ESS floor (covo_set_step_ess_floor, ess_min=%g): "
                "both define the update's weights; turn one of them off", what, h->elite_K, (double)h->ess_min);
        REQUIRE(h->elite_K >= 1 && h->elite_K <= n_samples, "%s: K=%d (covo_set_step_elite) outside [1, n_samples = %d]", what,
                h->elite_K, n_samples);
        REQUIRE(n_inst <= covo_elite_capacity(h), "%s: %d instances, the elite buffer (covo_set_step_elite) has %d rows", what, n_inst,
                covo_elite_capacity(h));
    }
    if (covo_step_iters(h) > 1) {  // the key chain of the passes is walked from the raw controller key
        REQUIRE(n_inst <= h->iter_n, "%s: %d instances, the iteration log (covo_set_step_iters) has n_inst=%d", what, n_inst, h->iter_n);
        REQUIRE(derive_keys == 1,
                "%s: iterations per step (covo_set_step_iters, iters=%d) need derive_keys = 1 (every pass derives its keys from the raw "
                "controller key on the device)", what, covo_step_iters(h));
    }
    if (covo_sigma_period(h) > 1) {  // only covo-online decides a Sigma per step
        REQUIRE(mode == COVO_MODE_COVO_ONLINE,
                "%s: the Sigma period (covo_set_step_sigma_period, period=%d) belongs to covo-online steps; this step's mode is %s, which "
                "computes no Sigma per step; set period = 1", what, covo_sigma_period(h), mode == COVO_MODE_MPPI ? "MPPI" : "covo-offline");
        REQUIRE(((uintptr_t)a_cov & 15) == 0, "%s: a_cov must be 16-byte aligned under a Sigma period (covo_set_step_sigma_period)", what);
    }
    REQUIRE(!covo_post_cov_on(h) || n_inst <= h->post_n, "%s: %d instances, the posterior covariance buffer (covo_set_step_post_cov) has "
            "n_inst=%d", what, n_inst, h->post_n);
    if (covo_sigma_adapt_on(h)) {  // a reuse step reads the previous step's posterior covariance
        REQUIRE(mode == COVO_MODE_COVO_ONLINE,
                "%s: Sigma adapt (covo_set_step_sigma_adapt, gamma=%g) belongs to the reuse steps of covo-online; this step's mode is %s, "
                "which computes no Sigma per step; turn it off (gamma = 0)", what, (double)h->adapt_gamma,
                mode == COVO_MODE_MPPI ? "MPPI" : "covo-offline");
        REQUIRE(covo_sigma_period(h) > 1,
                "%s: Sigma adapt (covo_set_step_sigma_adapt, gamma=%g) with a Sigma period of 1: every step refreshes Sigma and nothing "
                "would ever adapt; set a period above 1 (covo_set_step_sigma_period) or turn it off (gamma = 0)", what,
                (double)h->adapt_gamma);
        REQUIRE(covo_post_cov_on(h),
                "%s: Sigma adapt (covo_set_step_sigma_adapt, gamma=%g) without a posterior covariance target: a reuse step blends the "
                "covariance the previous step left there; attach one (covo_set_step_post_cov) or turn it off (gamma = 0)", what,
                (double)h->adapt_gamma);
        REQUIRE(n_inst <= h->adapt_n, "%s: %d instances, the Sigma adapt rows (covo_set_step_sigma_adapt) have n_inst=%d", what, n_inst,
                h->adapt_n);
    }
    if (covo_refine_on(h)) {  // the direction is Sigma^2 g / c^2 of THIS step's Hessian
        REQUIRE(mode == COVO_MODE_COVO_ONLINE,
                "%s: the Newton refinement (covo_set_step_refine) belongs to covo-online steps; this step's mode is %s, which has no "
                "Hessian-derived Sigma at the step's mean; detach it", what, mode == COVO_MODE_MPPI ? "MPPI" : "covo-offline");
        REQUIRE(covo_sigma_period(h) == 1,
                "%s: the Newton refinement (covo_set_step_refine) together with a Sigma period (covo_set_step_sigma_period, period=%d): a "
                "reuse step has no R and its c means something else; set period = 1 or detach it", what, covo_sigma_period(h));
        REQUIRE(n_inst <= h->refine_n, "%s: %d instances, the refine buffer (covo_set_step_refine) has n_inst=%d", what, n_inst,
                h->refine_n);
        REQUIRE(((uintptr_t)a_cov & 15) == 0, "%s: a_cov must be 16-byte aligned under the Newton refinement (covo_set_step_refine)", what);
    }
    if (covo_riccati_on(h)) {  // every mode and every step of a Sigma period: the sweep needs neither R nor Sigma
        REQUIRE(!covo_refine_on(h),
                "%s: the Riccati refinement (covo_set_step_riccati) together with the Newton refinement (covo_set_step_refine): both "
                "polish the committed mean; detach one of them", what);
        REQUIRE(n_inst <= h->riccati_n, "%s: %d instances, the riccati buffer (covo_set_step_riccati) has n_inst=%d", what, n_inst,
                h->riccati_n);
    }
    if (covo_feedback_on(h)) {  // the closed-loop candidates of the Riccati refinement's line search
        REQUIRE(covo_riccati_on(h),
                "%s: Riccati feedback (covo_set_step_riccati_feedback) without the Riccati refinement (covo_set_step_riccati): the "
                "closed-loop candidates run under that sweep's gains; attach it or detach the feedback rows", what);
        REQUIRE(n_inst <= h->feedback_n, "%s: %d instances, the feedback buffer (covo_set_step_riccati_feedback) has n_inst=%d", what,
                n_inst, h->feedback_n);
        for (int e = 0; e < n_inst; ++e)
            REQUIRE(params[e].disturb_kind != COVO_DISTURB_DRAG && params[e].disturb_kind != COVO_DISTURB_MIXED,
                    "%s: Riccati feedback (covo_set_step_riccati_feedback) with disturb_kind=%d (drag / mixed, instance %d): a 16-state "
                    "plant, whose force is a state of the sweep and a per-sample quantity of the rollout; detach the feedback rows", what,
                    params[e].disturb_kind, e);
    }
    if (covo_box_on(h)) {  // the box form of the Riccati refinement's sweep (16-state plants included: the box lives in the 4 x 4 part)
        REQUIRE(covo_riccati_on(h),
                "%s: the Riccati box (covo_set_step_riccati_box) without the Riccati refinement (covo_set_step_riccati): it is that "
                "sweep's stage problem; attach it or detach the masks", what);
        REQUIRE(n_inst <= h->box_n, "%s: %d instances, the box masks (covo_set_step_riccati_box) have n_inst=%d rows", what, n_inst,
                h->box_n);
    }
    if (h->plan_hold > 1) {  // the steps between two plan steps apply the sweep's law: they need the sweep, and every step a Sigma of its own
        REQUIRE(covo_riccati_on(h),
                "%s: the plan hold (covo_set_step_plan_hold, period=%d) without the Riccati refinement (covo_set_step_riccati): a hold "
                "step applies the gains of that sweep; attach it or set period = 1", what, h->plan_hold);
        REQUIRE(covo_sigma_period(h) == 1,
                "%s: the plan hold (covo_set_step_plan_hold, period=%d) together with a Sigma period (covo_set_step_sigma_period, "
                "period=%d): both thin out the step; set one of them to 1", what, h->plan_hold, covo_sigma_period(h));
        for (int e = 0; e < n_inst; ++e)
            REQUIRE(params[e].disturb_kind != COVO_DISTURB_DRAG && params[e].disturb_kind != COVO_DISTURB_MIXED,
                    "%s: the plan hold (covo_set_step_plan_hold) with disturb_kind=%d (drag / mixed, instance %d): a 16-state plant, whose "
                    "force is a state of the sweep; the hold step carries the 13-state plants only; set period = 1", what,
                    params[e].disturb_kind, e);
        REQUIRE(n_inst <= h->hold_n, "%s: %d instances, the hold rows (covo_set_step_plan_hold) have n_inst=%d", what, n_inst, h->hold_n);
    }
    if (covo_nodes_on(h)) {  // the spline nodes: a sampler under the annealed schedule, nothing of their own besides
        REQUIRE(covo_anneal_sched_on(h),
                "%s: the spline nodes (covo_set_step_nodes, n_nodes=%d) without an attached schedule (covo_set_step_anneal with a "
                "table): the schedule launch writes the marginals a_cov reports; attach it, or turn the nodes off (a null table)", what,
                h->nodes_M);
        REQUIRE(h->nodes_passes == h->anneal_passes,
                "%s: the spline nodes (covo_set_step_nodes) were set for n_pass=%d passes, the schedule (covo_set_step_anneal) for "
                "n_pass=%d: the basis table has one slice per pass; set both to the same count", what, h->nodes_passes, h->anneal_passes);
        REQUIRE(h->nodes_M >= 2 && h->nodes_M <= COVO_H, "%s: n_nodes=%d (covo_set_step_nodes) outside [2, %d]", what, h->nodes_M, COVO_H);
    }
    if (covo_sigma_nodes_on(h)) {  // covo-online in node space: its one launch stands in the place of the Sigma chain of EVERY step
        REQUIRE(h->sn_M >= 2 && h->sn_M <= COVO_SIGMA_NODES_MAX, "%s: M=%d (covo_set_step_sigma_nodes) outside [2, %d]", what, h->sn_M,
                COVO_SIGMA_NODES_MAX);
        REQUIRE(covo_sigma_period(h) == 1,
                "%s: Sigma in node space (covo_set_step_sigma_nodes, M=%d) together with a Sigma period (covo_set_step_sigma_period, "
                "period=%d): a reuse step shifts a 128 x 128 factor, and there is none; set period = 1 or turn it off (a null W)", what,
                h->sn_M, covo_sigma_period(h));
        REQUIRE(!covo_sigma_adapt_on(h),
                "%s: Sigma in node space (covo_set_step_sigma_nodes, M=%d) together with Sigma adapt (covo_set_step_sigma_adapt, gamma=%g): "
                "it belongs to the reuse steps of a Sigma period; turn one of them off", what, h->sn_M, (double)h->adapt_gamma);
        REQUIRE(!covo_refine_on(h),
                "%s: Sigma in node space (covo_set_step_sigma_nodes, M=%d) together with the Newton refinement (covo_set_step_refine): its "
                "direction needs the full-rank Sigma, and this one has rank %d; detach one of them", what, h->sn_M, 4 * h->sn_M);
        REQUIRE(mode == COVO_MODE_COVO_ONLINE,
                "%s: Sigma in node space (covo_set_step_sigma_nodes, M=%d) belongs to covo-online steps; this step's mode is %d, which "
                "forms no Hessian per step; turn it off (a null W)", what, h->sn_M, mode);
        REQUIRE(!sharded,
                "%s: Sigma in node space (covo_set_step_sigma_nodes, M=%d) is not available for sample-sharded steps (partial_out != "
                "NULL); turn it off (a null W)", what, h->sn_M);
        REQUIRE(n_inst <= h->sn_n, "%s: %d instances, the side rows (covo_set_step_sigma_nodes) have n_inst=%d", what, n_inst, h->sn_n);
    }
    if (covo_anneal_on(h)) {  // the annealed step: MPPI's block-diagonal draw under a per-pass table, weights on standardised costs
        REQUIRE(mode == COVO_MODE_MPPI,
                "%s: the annealed step (covo_set_step_anneal) belongs to MPPI steps (COVO_MODE_MPPI): its schedule writes the 4 x 4 block "
                "factors only that mode samples from; this step's mode is %d; turn it off (a null table and temp = 0)", what, mode);
        REQUIRE(h->anneal_passes == covo_step_iters(h),
                "%s: the annealed step (covo_set_step_anneal) was set for n_pass=%d passes, this step runs iters=%d "
                "(covo_set_step_iters): the table has one row per pass; set both to the same count", what, h->anneal_passes,
                covo_step_iters(h));
        REQUIRE(gamma_sigma == 0.0f,
                "%s: the annealed step (covo_set_step_anneal) together with gamma_sigma=%g: the schedule owns a_cov, MPPI's covariance "
                "adaptation would adapt what the next pass overwrites; set gamma_sigma = 0", what, (double)gamma_sigma);
        REQUIRE(!covo_anneal_temp_on(h) || !covo_ess_on(h),
                "%s: the annealed step's standardised temperature (covo_set_step_anneal, temp=%g) together with the ESS floor "
                "(covo_set_step_ess_floor, ess_min=%g): both define the update's weights; turn one of them off", what,
                (double)h->anneal_temp, (double)h->ess_min);
        REQUIRE(!covo_anneal_temp_on(h) || covo_elite_target(h) == nullptr,
                "%s: the annealed step's standardised temperature (covo_set_step_anneal, temp=%g) together with the elite-set update "
                "(covo_set_step_elite, K=%d): both define the update's weights; turn one of them off", what, (double)h->anneal_temp,
                h->elite_K);
        REQUIRE(!sharded,
                "%s: the annealed step (covo_set_step_anneal) is not available for sample-sharded steps (partial_out != NULL): a rank "
                "sees only its shard's costs; turn it off (a null table and temp = 0)", what);
        REQUIRE(!fused_batch,
                "%s: the annealed step (covo_set_step_anneal) is not available for the env-batched step's one fused launch, which "
                "shifts and factors a_cov itself and needs the temperature before all costs exist; run the staged batch "
                "(covo_set_step_batched_staged)", what);
        REQUIRE(h->anneal_rows == nullptr || n_inst <= h->anneal_n,
                "%s: %d instances, the per-pass rows (covo_set_step_anneal) have n_inst=%d", what, n_inst, h->anneal_n);
    }
    return 0;
}

// ---- what a step in COVO_MODE_ILQR checks ahead of check_step_attachments, for every entry point alike: the sweep it consists of is
// attached, and nothing that belongs to a sampling step is.  The order is fixed: the sharded step, the sweep, the other refinement,
// then the sampling attachments in check_step_attachments' order, the raw key, the rows of the logs
int check_ilqr_step(const covo_ctx *h, int n_inst, bool sharded, int derive_keys, const char *what)
{
    REQUIRE(!sharded,
            "%s: an iLQR step (COVO_MODE_ILQR) is not available for sample-sharded steps (partial_out != NULL): it has no samples to "
            "shard; run it on one rank", what);
    REQUIRE(covo_riccati_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) without the Riccati refinement (covo_set_step_riccati): its iterations are that sweep "
            "and its line search; attach the rows", what);
    REQUIRE(!covo_refine_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) together with the Newton refinement (covo_set_step_refine): its direction needs the "
            "Sigma of a covo-online step, which an iLQR step does not compute; detach it", what);
    REQUIRE(covo_diag_target(h) == nullptr,
            "%s: an iLQR step (COVO_MODE_ILQR) together with sampling diagnostics (covo_set_step_diag / covo_set_episode_diag_log): "
            "nothing is sampled; detach the buffer", what);
    REQUIRE(!covo_fan_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) together with the sample fan (covo_set_step_fan / covo_set_episode_fan): nothing is "
            "sampled; detach the buffer", what);
    REQUIRE(!covo_arb_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) together with the update arbiter (covo_set_step_arbiter): there is no softmax mean and "
            "no best sample to arbitrate; detach it", what);
    REQUIRE(!covo_ess_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) together with the ESS floor (covo_set_step_ess_floor, ess_min=%g): there are no "
            "weights; turn it off (ess_min = 0)", what, (double)h->ess_min);
    REQUIRE(covo_elite_target(h) == nullptr,
            "%s: an iLQR step (COVO_MODE_ILQR) together with the elite-set update (covo_set_step_elite, K=%d): there are no samples "
            "to select from; turn it off (K = 0)", what, h->elite_K);
    REQUIRE(covo_sigma_period(h) == 1,
            "%s: an iLQR step (COVO_MODE_ILQR) together with a Sigma period (covo_set_step_sigma_period, period=%d): it computes no "
            "Sigma; set period = 1", what, covo_sigma_period(h));
    REQUIRE(!covo_post_cov_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) together with the posterior covariance (covo_set_step_post_cov): nothing is sampled; "
            "detach the buffer", what);
    REQUIRE(!covo_sigma_adapt_on(h),
            "%s: an iLQR step (COVO_MODE_ILQR) together with Sigma adapt (covo_set_step_sigma_adapt, gamma=%g): it computes no Sigma; "
            "turn it off (gamma = 0)", what, (double)h->adapt_gamma);
    REQUIRE(derive_keys == 1,
            "%s: an iLQR step (COVO_MODE_ILQR) needs derive_keys = 1 (its disturbance inputs are derived from the raw controller key "
            "on the device)", what);
    const bool logs = h->ilqr_rows != nullptr || h->ilqr_fb_rows != nullptr || h->ilqr_summary != nullptr;
    REQUIRE(!logs || n_inst <= h->ilqr_n, "%s: %d instances, the iLQR logs (covo_set_step_ilqr) have n_inst=%d", what, n_inst, h->ilqr_n);
    REQUIRE(h->ilqr_costs == nullptr || n_inst <= h->ilqr_costs_n, "%s: %d instances, the iLQR cost buffer (covo_debug_ilqr_costs) has "
            "n_inst=%d", what, n_inst, h->ilqr_costs_n);
    REQUIRE(h->ilqr_box == nullptr || n_inst <= h->ilqr_box_n, "%s: %d instances, the iLQR box counts (covo_set_step_ilqr_box) have "
            "n_inst=%d", what, n_inst, h->ilqr_box_n);
    return 0;
}

// ---- what a step in COVO_MODE_CMA checks ahead of check_step_attachments, for every entry point alike: its attachment, the two
// targets the next step reads, and nothing that decides a Sigma another way
int check_cma_step(const covo_ctx *h, int n_inst, bool sharded, const float *a_cov, const char *what)
{
    REQUIRE(!sharded,
            "%s: a CMA step (COVO_MODE_CMA) is not available for sample-sharded steps (partial_out != NULL): it needs the posterior "
            "covariance and the diagnostics, which sample-sharded steps cannot have; run it on one rank", what);
    REQUIRE(covo_cma_on(h), "%s: a CMA step (COVO_MODE_CMA) without covo_set_step_cma on the handle: its rows and its path live there; "
            "attach them", what);
    REQUIRE(n_inst <= h->cma_n, "%s: %d instances, the CMA rows (covo_set_step_cma) have n_inst=%d", what, n_inst, h->cma_n);
    REQUIRE(covo_post_cov_on(h), "%s: a CMA step (COVO_MODE_CMA) without a posterior covariance target: the next step adapts to the "
            "covariance and the displacement this one leaves there; attach one (covo_set_step_post_cov)", what);
    REQUIRE(h->post_aux_out != nullptr, "%s: a CMA step (COVO_MODE_CMA) needs the posterior covariance's side rows (covo_set_step_post_cov, "
            "aux): the step size reads the displacement and the weight sum there", what);
    REQUIRE(covo_diag_target(h) != nullptr, "%s: a CMA step (COVO_MODE_CMA) without a diagnostics target: the next step reads this one's "
            "effective sample size there; attach one (covo_set_step_diag)", what);
    REQUIRE(covo_sigma_period(h) == 1, "%s: a CMA step (COVO_MODE_CMA) together with a Sigma period (covo_set_step_sigma_period, "
            "period=%d): it adapts its covariance every step and never refreshes one; set period = 1", what, covo_sigma_period(h));
    REQUIRE(!covo_sigma_adapt_on(h), "%s: a CMA step (COVO_MODE_CMA) together with Sigma adapt (covo_set_step_sigma_adapt, gamma=%g): "
            "the step runs that blend itself at covo_set_step_cma's gamma; turn it off (gamma = 0)", what, (double)h->adapt_gamma);
    REQUIRE(!covo_sigma_nodes_on(h), "%s: a CMA step (COVO_MODE_CMA) together with Sigma in node space (covo_set_step_sigma_nodes, "
            "M=%d): it forms no Hessian; turn it off (a null W)", what, h->sn_M);
    REQUIRE(a_cov != nullptr && ((uintptr_t)a_cov & 15) == 0, "%s: a CMA step (COVO_MODE_CMA) needs a_cov (float[128][128] per "
            "instance, 16-byte aligned): the shape is formed and scaled there", what);
    return 0;
}

// an episode driver that writes rows [first_row, first_row + n_steps) of every attached log (the single driver: first_row = 0)
int check_episode_logs(const covo_ctx *h, int first_row, int n_steps, const char *what)
{
    // the first offender is reported: four logs with setters of their own, then covo_set_episode_rows' kinds, then the hold log
    static const int order[COVO_EPLOG_ALL] = {COVO_EPLOG_DIAG,  COVO_EPLOG_TRACE, COVO_EPLOG_FAN,   COVO_EPLOG_ARB,      COVO_EPLOG_LAM, COVO_EPLOG_ELITE,
                                              COVO_EPLOG_ITERS, COVO_EPLOG_SIGMA, COVO_EPLOG_POST_AUX, COVO_EPLOG_POST_COV, COVO_EPLOG_HOLD};
    for (const int k : order)
        REQUIRE(h->eplog[k].log == nullptr || (first_row >= 0 && first_row + n_steps <= h->eplog[k].stride),
                "%s: %s rows [%d, %d) outside [0, %d) (%s)", what, covo_eplog_kinds[k].name, first_row, first_row + n_steps,
                h->eplog[k].stride, covo_eplog_kinds[k].setter);
    return 0;
}

// every argument check of a single step (covo_mpc_step, and each step of covo_run_episode): nothing is launched before all of them
// have passed
int check_single_step(const covo_ctx *h, const covo_env_params *params, const covo_step_args *args, const char *what)
{
    REQUIRE((args->mode >= 0 && args->mode <= COVO_MODE_ILQR) || args->mode == COVO_MODE_CMA, "%s: mode=%d", what, args->mode);
    REQUIRE(args->n_samples > 0 && args->n_samples <= h->cfg.n_local, "%s: n_samples=%d outside (0, %d]", what, args->n_samples,
            h->cfg.n_local);
    REQUIRE(args->state && args->pos_traj && args->vel_traj && args->a_mean && args->a && args->cost && args->groupmin && args->T > 0,
            "%s: null buffer", what);
    REQUIRE(args->mode != COVO_MODE_COVO_OFFLINE || (args->L_table && args->n_table > 0), "%s: offline needs L_table", what);
    REQUIRE(args->mode != COVO_MODE_MPPI || args->a_cov, "%s: mppi needs a_cov", what);
    CHECK_MODEL(params, what);
    REQUIRE(args->gamma_sigma == 0.0f || args->mode == COVO_MODE_MPPI, "%s: gamma_sigma != 0 is MPPI's covariance adaptation (mppi.py:119-125)",
            what);
    REQUIRE(!covo_needs_tables(*params) || args->derive_keys == 1, "%s: disturb_kind=%d needs derive_keys = 1 (the per-step "
            "disturbance tables are derived from the raw controller key on the device)", what, params->disturb_kind);
    REQUIRE(h->plan_hold <= 1 || (((uintptr_t)args->a_mean | (uintptr_t)args->a_mean_in | (uintptr_t)args->a_cov) & 15) == 0,
            "%s: a_mean, a_mean_in and a_cov must be 16-byte aligned under the plan hold (covo_set_step_plan_hold)", what);
    if (args->mode == COVO_MODE_ILQR)
        if (int rc = check_ilqr_step(h, 1, args->partial_out != nullptr, args->derive_keys, what)) return rc;
    if (args->mode == COVO_MODE_CMA)
        if (int rc = check_cma_step(h, 1, args->partial_out != nullptr, args->a_cov, what)) return rc;
    return check_step_attachments(h, args->n_samples, 1, args->partial_out != nullptr, args->derive_keys, args->mode, args->a_cov, params, what,
                                  args->gamma_sigma);
}

// the per-instance models of one env-batched launch: valid selectors, and one kernel variant for all of them.  env_step: the launch
// also steps the environments (covo_env_step_batched, the episode drivers), whose variant hangs on two more fields
int check_batch_models(const covo_env_params *params, int E, bool env_step, const char *what)
{
    for (int e = 0; e < E; ++e) {
        CHECK_MODEL(&params[e], what);
        bool same = params[e].reward_kind == params[0].reward_kind && params[e].rollover_terminate == params[0].rollover_terminate &&
                    params[e].disturb_kind == params[0].disturb_kind;
        if (env_step) same = same && params[e].max_steps_in_episode == params[0].max_steps_in_episode && params[e].reset_traj == params[0].reset_traj;
        REQUIRE(same, "%s: instance %d differs from instance 0 in reward_kind / rollover_terminate / disturb_kind%s (one kernel variant "
                "per launch); disturb_params / period / scale may differ", what, e, env_step ? " / max_steps_in_episode / reset_traj" : "");
    }
    return 0;
}

// every argument check of a batched step in `mode` (covo_mpc_step_batched / _mode, and with episode set covo_run_episode_batched /
// _mode, whose launches also step the environments): nothing is launched before all of them have passed.  *norm: the argument
// block with its padding zeroed (it is a cache key)
int check_batch_step(covo_ctx *h, const covo_batch_args *args, const covo_batch_mode_args *m, const covo_env_params *params,
                     bool episode, const char *what, covo_batch_mode_args *norm)
{
    REQUIRE(args->n_envs > 0 && args->n_envs <= COVO_MAX_ENVS, "%s: n_envs=%d outside (0, %d]", what, args->n_envs, COVO_MAX_ENVS);
    REQUIRE(args->n_samples > 0 && args->n_samples <= h->cfg.n_local, "%s: n_samples=%d outside (0, %d]", what, args->n_samples,
            h->cfg.n_local);
    const int mode = m ? m->mode : COVO_MODE_COVO_ONLINE;
    REQUIRE(mode == COVO_MODE_MPPI || mode == COVO_MODE_COVO_ONLINE || mode == COVO_MODE_COVO_OFFLINE || mode == COVO_MODE_ILQR ||
                mode == COVO_MODE_CMA,
            "%s: mode=%d is not a COVO_MODE_*", what, mode);
    REQUIRE(args->states && args->pos_traj && args->vel_traj && args->a_mean && args->a && args->cost &&
                (args->groupmin || mode != COVO_MODE_COVO_ONLINE) && args->T > 0,
            "%s: null buffer", what);
    // (for every mode: the callers take the mode from it.  Only the MPPI / covo-offline batches key their scratch by it)
    std::memset(norm, 0, sizeof(*norm));
    norm->base.n_envs = args->n_envs; norm->base.n_samples = args->n_samples; norm->base.T = args->T;
    norm->base.states = args->states; norm->base.pos_traj = args->pos_traj; norm->base.vel_traj = args->vel_traj;
    norm->base.a_mean = args->a_mean; norm->base.a_cov = args->a_cov; norm->base.a = args->a; norm->base.cost = args->cost;
    norm->base.groupmin = args->groupmin; norm->base.gamma_mean = args->gamma_mean; norm->base.sample_sigma = args->sample_sigma;
    norm->mode = mode;
    norm->gamma_sigma = m ? m->gamma_sigma : 0.0f;
    if (mode == COVO_MODE_COVO_OFFLINE) {
        norm->n_table = m->n_table;
        norm->L_table = m->L_table;
        norm->L_table_stride = m->L_table_stride;
    }
    int rc = check_batch_models(params, args->n_envs, episode, what);
    if (rc) return rc;
    if (mode == COVO_MODE_ILQR) {  // nothing of the sampling batches' lists applies: its own, then the attachments'
        if ((rc = check_ilqr_step(h, args->n_envs, false, 1, what))) return rc;
        REQUIRE(h->plan_hold <= 1 || ((uintptr_t)args->a_mean & 15) == 0,
                "%s: a_mean must be 16-byte aligned under the plan hold (covo_set_step_plan_hold)", what);
        return check_step_attachments(h, args->n_samples, args->n_envs, false, 1, mode, args->a_cov, params, what);
    }
    if (mode == COVO_MODE_CMA) {  // covo-online's staged batch: its own list, then the attachments'
        if ((rc = check_cma_step(h, args->n_envs, false, args->a_cov, what))) return rc;
        REQUIRE(args->groupmin != nullptr, "%s: a CMA step (COVO_MODE_CMA) needs base.groupmin (float[n_envs][ceil(n_samples / 64)])", what);
        REQUIRE(!covo_riccati_on(h), "%s: the Riccati refinement (covo_set_step_riccati) is not available for the env-batched CMA step: "
                "that batch carries no per-instance Hessian constants for it; detach it", what);
        REQUIRE(h->plan_hold <= 1, "%s: the plan hold (covo_set_step_plan_hold) is not available for a CMA step; set period = 1", what);
        return check_step_attachments(h, args->n_samples, args->n_envs, false, 1, mode, args->a_cov, params, what);
    }
    // covo_set_step_batched_staged: the MPPI / covo-offline batch runs its staged launch sequence, which takes what the fused launch
    // refuses below and has its own short list further down
    const bool staged = mode != COVO_MODE_COVO_ONLINE && covo_batched_staged(h);
    REQUIRE(mode == COVO_MODE_COVO_ONLINE || staged || !covo_ess_on(h),
            "%s: the ESS floor (covo_set_step_ess_floor, ess_min=%g) is not available for the env-batched MPPI / covo-offline step: its "
            "one fused launch needs the temperature before all costs exist, and there is no staged batched fallback; turn it off "
            "(ess_min = 0)", what, (double)h->ess_min);
    REQUIRE(mode == COVO_MODE_COVO_ONLINE || staged || covo_elite_target(h) == nullptr,
            "%s: the elite-set update (covo_set_step_elite, K=%d) is not available for the env-batched MPPI / covo-offline step: its "
            "one fused launch needs the weights before all costs exist, and there is no staged batched fallback; turn it off "
            "(K = 0)", what, h->elite_K);
    REQUIRE(mode == COVO_MODE_COVO_ONLINE || staged || covo_step_iters(h) == 1 || !covo_arb_on(h),
            "%s: iterations per step (covo_set_step_iters, iters=%d) together with the update arbiter (covo_set_step_arbiter) are not "
            "available for the env-batched MPPI / covo-offline step: its fused launch keeps each pass's starting mean in LDS only; "
            "detach one of them", what, covo_step_iters(h));
    REQUIRE(mode == COVO_MODE_COVO_ONLINE || staged || !covo_post_cov_on(h),
            "%s: the posterior covariance (covo_set_step_post_cov) is not available for the env-batched MPPI / covo-offline step: its "
            "one fused launch keeps the samples in LDS and never stores them, and there is no staged batched fallback; detach the "
            "buffer", what);
    REQUIRE(mode == COVO_MODE_COVO_ONLINE || !covo_riccati_on(h),
            "%s: the Riccati refinement (covo_set_step_riccati) is not available for the env-batched MPPI / covo-offline step, fused or "
            "staged: those batches carry no per-instance Hessian constants; detach it", what);
    REQUIRE(h->plan_hold <= 1 || ((uintptr_t)args->a_mean & 15) == 0,
            "%s: a_mean must be 16-byte aligned under the plan hold (covo_set_step_plan_hold)", what);
    if ((rc = check_step_attachments(h, args->n_samples, args->n_envs, false, 1, mode, args->a_cov, params, what, norm->gamma_sigma,
                                     mode != COVO_MODE_COVO_ONLINE && !staged))) return rc;  // (batched steps derive their keys)
    if (mode == COVO_MODE_COVO_ONLINE) return 0;
    REQUIRE(mode != COVO_MODE_MPPI || args->a_cov != nullptr, "%s: MPPI needs base.a_cov (float[n_envs][H][4][4])", what);
    REQUIRE(mode != COVO_MODE_COVO_OFFLINE || (m->L_table != nullptr && m->n_table > 0 && m->L_table_stride >= 0),
            "%s: covo-offline needs L_table (the per-instance Sigma factor table is missing: n_table=%d)", what, m->n_table);
    if (staged) {
        REQUIRE(args->groupmin != nullptr, "%s: the staged batched step (covo_set_step_batched_staged) needs base.groupmin "
                "(float[n_envs][ceil(n_samples / 64)]): its update reads the per-wave cost minima the rollout leaves there", what);
        REQUIRE(m->gamma_sigma == 0.0f || mode == COVO_MODE_MPPI, "%s: gamma_sigma != 0 is MPPI's covariance adaptation "
                "(mppi.py:119-125); this step's mode is covo-offline", what);
        REQUIRE(m->gamma_sigma == 0.0f || !covo_update_staged(h), "%s: gamma_sigma != 0 together with %s is not available for the "
                "staged batched step (covo_set_step_batched_staged): that covariance update has no instance dimension; set "
                "gamma_sigma = 0 or detach it", what,
                covo_elite_target(h) ? "the elite-set update (covo_set_step_elite)" : "the ESS floor (covo_set_step_ess_floor)");
        REQUIRE(!exchange_ready(h), "%s: the staged batched step (covo_set_step_batched_staged) is not available on a sample-sharded "
                "handle (covo_exchange_connect): the instances of a batch are whole", what);
        return 0;
    }
    int which = 0;
    const char *why = batch_small_refusal(h, norm, params, &which);
    REQUIRE(why == nullptr, "%s: instance %d cannot take the batched fused launch: %s (there is no staged batched fallback)", what,
            which, why);
    return 0;
}

// what every setter asks of the rows of a buffer it attaches (attached: there is one), in the setter's name
int check_setter_rows(const char *setter, bool attached, int n_inst)
{
    REQUIRE(!attached || (n_inst > 0 && n_inst <= COVO_MAX_ENVS), "%s: n_inst=%d outside (0, %d]", setter, n_inst, COVO_MAX_ENVS);
    return 0;
}

extern "C" {

// ---- per-HANDLE experiment switches (CovoOpts, covo_common.hpp); every setter bumps the handle's epoch: its captured step graphs
// hold the old launch set / kernel arguments and are re-captured at the next step
int covo_debug_set_stream_gemm(covo_handle_t h, int on)
{
    REQUIRE(h, "covo_debug_set_stream_gemm: null handle");
    h->opt.stream_gemm = on ? 1 : 0;
    ++h->opt.epoch;
    return 0;
}

int covo_debug_set_fuse_small(covo_handle_t h, int on)
{
    REQUIRE(h, "covo_debug_set_fuse_small: null handle");
    h->opt.fuse_small = on ? 1 : 0;
    ++h->opt.epoch;
    return 0;
}

int covo_debug_set_fold_begin(covo_handle_t h, int on)
{
    REQUIRE(h, "covo_debug_set_fold_begin: null handle");
    h->opt.fold_begin = on ? 1 : 0;
    ++h->opt.epoch;
    return 0;
}

int covo_debug_set_ns_deflate(covo_handle_t h, int on)
{
    REQUIRE(h, "covo_debug_set_ns_deflate: null handle");
    h->opt.ns_deflate = on ? 1 : 0;
    ++h->opt.epoch;
    return 0;
}

int covo_debug_set_ns_merged(covo_handle_t h, int on)
{
    REQUIRE(h, "covo_debug_set_ns_merged: null handle");
    h->opt.ns_merged = on ? 1 : 0;
    ++h->opt.epoch;
    return 0;
}

int covo_debug_set_ns_coherence(covo_handle_t h, int force_agent)
{
    REQUIRE(h, "covo_debug_set_ns_coherence: null handle");
    h->opt.ns_force_agent = force_agent ? 1 : 0;
    ++h->opt.epoch;
    return 0;
}

// ---- the staged env-batched MPPI / covo-offline step (step.hip: covo_step_batched_staged_impl).  A switch of the handle like the ones
// above: the captured batched graphs hold the other launch set
int covo_set_step_batched_staged(covo_handle_t h, int32_t on)
{
    REQUIRE(h, "covo_set_step_batched_staged: null handle");
    const int v = on ? 1 : 0;
    if (v != h->batched_staged) ++h->opt.epoch;
    h->batched_staged = v;
    return 0;
}

// ---- per-step sampling diagnostics.  The captured step graphs bake in where the steps write: a change of that target bumps the
// epoch like a debug switch (attaching the episode log next to a step buffer changes no launch of a step: its rows are copied by
// an eager launch of the episode drivers)
int covo_set_step_diag(covo_handle_t h, float *diag, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_diag: null handle");
    if (int rc = check_setter_rows("covo_set_step_diag", diag != nullptr, n_inst)) return rc;
    const float *before = covo_diag_target(h);
    h->diag_out = diag;
    h->diag_n = diag ? n_inst : 0;
    if (covo_diag_target(h) != before) ++h->opt.epoch;
    return 0;
}

// what the six setters of the episode logs share (covo_eplog_kinds, covo_common.hpp): with a log, stride > 0 (stride_fmt: the setter's
// own text) and the attachment the log follows is on; the null-handle check and the setter's extras stay with the setter
static int set_episode_log(covo_ctx *h, int kind, float *log, int stride, const char *stride_fmt)
{
    const covo_eplog_kind &k = covo_eplog_kinds[kind];
    REQUIRE(log == nullptr || stride > 0, stride_fmt, stride);
    if (log != nullptr && k.on != nullptr && !k.on(h)) {
        if (kind < COVO_EPLOG_KINDS) covo_set_error("covo_set_episode_rows: kind=%d: %s", kind, k.off);
        else covo_set_error("%s", k.off);
        return COVO_E_BADARG;
    }
    h->eplog[kind] = {log, log ? stride : 0};
    return 0;
}

int covo_set_episode_diag_log(covo_handle_t h, float *log, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_diag_log: null handle");
    const float *before = covo_diag_target(h);
    const int rc = set_episode_log(h, COVO_EPLOG_DIAG, log, stride, "covo_set_episode_diag_log: stride=%d");
    if (covo_diag_target(h) != before) ++h->opt.epoch;
    return rc;
}

// ---- the ESS floor (ess_lambda.hip).  The captured step graphs bake in the staged launch set, ess_min and where the solver writes:
// any change bumps the epoch.  The valid range of ess_min depends on the step's sample count: checked at the step (check_step_attachments)
int covo_set_step_ess_floor(covo_handle_t h, float ess_min, float *lam_out, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_ess_floor: null handle");
    REQUIRE(ess_min >= 0.0f && ess_min < __builtin_inff(), "covo_set_step_ess_floor: ess_min=%g is not a finite number >= 0 (0 = off)",
            (double)ess_min);
    if (int rc = check_setter_rows("covo_set_step_ess_floor", lam_out != nullptr, n_inst)) return rc;
    if (ess_min != h->ess_min || lam_out != h->lam_out) ++h->opt.epoch;
    h->ess_min = ess_min;
    h->lam_out = lam_out;
    h->lam_n = lam_out ? n_inst : 0;
    if (covo_lam_target(h) == nullptr) covo_eprow_drop(h, COVO_EPLOG_LAM);  // off, the log with it
    return 0;
}

int covo_step_nodes(covo_handle_t h, int32_t *n_pass, int32_t *n_nodes)
{
    REQUIRE(h, "covo_step_nodes: null handle");
    REQUIRE(n_pass && n_nodes, "covo_step_nodes: bad argument");
    *n_pass = h->nodes_passes;
    *n_nodes = h->nodes_M;
    return 0;
}

// ---- the elite-set update (elite_select.hip, reduce_elite.hip).  The captured step graphs bake in the staged launch set, K and where
// the selector writes: any change bumps the epoch.  The valid range of K depends on the step's sample count: checked at the step
// (check_step_attachments)
int covo_set_step_elite(covo_handle_t h, int32_t K, float *rows_out, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_elite: null handle");
    REQUIRE(K >= 0, "covo_set_step_elite: K=%d is negative (0 = off; a step takes K in [1, n_samples])", K);
    if (int rc = check_setter_rows("covo_set_step_elite", rows_out != nullptr, n_inst)) return rc;
    if (K != h->elite_K || rows_out != h->elite_out) ++h->opt.epoch;
    h->elite_K = K;
    h->elite_out = rows_out;
    h->elite_n = rows_out ? n_inst : 0;
    if (covo_elite_target(h) == nullptr) covo_eprow_drop(h, COVO_EPLOG_ELITE);  // off, the log with it
    return 0;
}

// ---- the flight recorder (plan_trace.hip).  Its launch is eager and follows the step: attaching or detaching a buffer changes no
// captured step graph
int covo_set_step_plan(covo_handle_t h, float *plan, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_plan: null handle");
    if (int rc = check_setter_rows("covo_set_step_plan", plan != nullptr, n_inst)) return rc;
    h->plan_out = plan;
    h->plan_n = plan ? n_inst : 0;
    return 0;
}

int covo_set_episode_trace(covo_handle_t h, float *trace, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_trace: null handle");
    return set_episode_log(h, COVO_EPLOG_TRACE, trace, stride, "covo_set_episode_trace: stride=%d");
}

// ---- the sample fan (sample_fan.hip).  Like the plan's, its launch is eager and follows the step: no captured step graph changes
int covo_set_step_fan(covo_handle_t h, float *fan, const int32_t *idx, int32_t K, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_fan: null handle");
    if (fan == nullptr && K == 0) {  // off, the log with it
        h->fan_out = nullptr;
        h->fan_idx = nullptr;
        h->fan_K = h->fan_n = 0;
        covo_eprow_drop(h, COVO_EPLOG_FAN);
        return 0;
    }
    REQUIRE(K >= 1 && K <= COVO_FAN_MAX, "covo_set_step_fan: K=%d outside [1, %d]", K, COVO_FAN_MAX);
    if (int rc = check_setter_rows("covo_set_step_fan", true, n_inst)) return rc;
    REQUIRE(K <= h->cfg.n_local, "covo_set_step_fan: K=%d > n_samples: the handle has n_local=%d samples", K, h->cfg.n_local);
    REQUIRE(h->eplog[COVO_EPLOG_FAN].log == nullptr || K == h->fan_K, "covo_set_step_fan: K=%d differs from the attached episode log's K=%d "
            "(detach it first: covo_set_episode_fan(h, NULL, 0))", K, h->fan_K);
    h->fan_out = fan;
    h->fan_idx = idx;
    h->fan_K = K;
    h->fan_n = n_inst;
    return 0;
}

int covo_set_episode_fan(covo_handle_t h, float *fanlog, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_fan: null handle");
    return set_episode_log(h, COVO_EPLOG_FAN, fanlog, stride, "covo_set_episode_fan: stride=%d");  // (its rows are [fan_K][COVO_FAN_FLOATS])
}

// ---- the update arbiter (update_arbiter.hip).  Like the plan's and the fan's, its launch is eager and follows the step: no captured
// step graph changes
int covo_set_step_arbiter(covo_handle_t h, float *rows, int32_t mask, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_arbiter: null handle");
    if (rows == nullptr) {  // off, the log with it
        h->arb_out = nullptr;
        h->arb_mask = h->arb_n = 0;
        covo_eprow_drop(h, COVO_EPLOG_ARB);
        return 0;
    }
    REQUIRE(mask >= 1 && mask <= 7, "covo_set_step_arbiter: mask=%d outside [1, 7] (bit 0: softmax mean, 1: nominal, 2: best sample)", mask);
    if (int rc = check_setter_rows("covo_set_step_arbiter", true, n_inst)) return rc;
    h->arb_out = rows;
    h->arb_mask = mask;
    h->arb_n = n_inst;
    return 0;
}

int covo_set_episode_arbiter_log(covo_handle_t h, float *log, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_arbiter_log: null handle");
    return set_episode_log(h, COVO_EPLOG_ARB, log, stride, "covo_set_episode_arbiter_log: stride=%d");
}

// ---- iterations per control step: K sample-rollout-update passes per call on the step's one state (step.hip enqueues them).  The
// captured step graphs hold all K passes and the log's address: a change bumps the epoch like a debug switch
int covo_set_step_iters(covo_handle_t h, int32_t iters, float *iter_log, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_iters: null handle");
    REQUIRE(iters >= 1 && iters <= COVO_MAX_STEP_ITERS, "covo_set_step_iters: iters=%d outside [1, %d]", iters, COVO_MAX_STEP_ITERS);
    const bool on = iters > 1 && iter_log != nullptr;
    if (int rc = check_setter_rows("covo_set_step_iters", on, n_inst)) return rc;
    const int before = covo_step_iters(h);
    const float *log_before = before > 1 ? h->iter_log : nullptr;
    h->iters = on ? iters : 1;
    h->iter_log = on ? iter_log : nullptr;
    h->iter_n = on ? n_inst : 0;
    if (covo_step_iters(h) != before || h->iter_log != log_before) ++h->opt.epoch;
    if (covo_step_iters(h) != before) covo_eprow_drop(h, COVO_EPLOG_ITERS);  // off or another row width: the log goes
    return 0;
}

// ---- the Sigma period (sigma_shift.hip): every m-th covo-online step is today's step, the m - 1 between shift the previous step's
// factor (step.hip: the reuse branch of enqueue_step / batch_enqueue, with a graph of its own next to the step's: no epoch bump).
// Which modes may carry a period is checked at the step (check_step_attachments)
int covo_set_step_sigma_period(covo_handle_t h, int32_t period)
{
    REQUIRE(h, "covo_set_step_sigma_period: null handle");
    REQUIRE(period >= 1 && period <= COVO_MAX_SIGMA_PERIOD, "covo_set_step_sigma_period: period=%d outside [1, %d] (1 = off: every step "
            "computes its own Sigma)", period, COVO_MAX_SIGMA_PERIOD);
    h->sigma_period = period;
    h->sigma_age = 0;
    if (covo_sigma_period(h) == 1) covo_eprow_drop(h, COVO_EPLOG_SIGMA);  // off, the log with it
    return 0;
}

int covo_step_sigma_age(covo_handle_t h, int32_t *next_age, int32_t *last_age)
{
    REQUIRE(h, "covo_step_sigma_age: null handle");
    if (next_age) *next_age = covo_sigma_period(h) > 1 ? h->sigma_age : 0;
    if (last_age) *last_age = h->sigma_last_age;
    return 0;
}

// ---- Sigma adapt (sigma_adapt.hip): a reuse step of the Sigma period blends the previous step's posterior covariance, which the
// after-step frame left in the attached post_cov target, into the covariance it shifts.  The reuse step's captured graph holds gamma
// and the rows' address: a change bumps the epoch like a debug switch; the schedule restarts.  What the step needs next to it (a
// post_cov target, covo-online, a period above 1) is checked at the step (check_step_attachments)
int covo_set_step_sigma_adapt(covo_handle_t h, float gamma, float *rows_out, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_sigma_adapt: null handle");
    const bool on = rows_out != nullptr && gamma != 0.0f;
    REQUIRE(!on || (gamma > 0.0f && gamma < 1.0f), "covo_set_step_sigma_adapt: gamma=%g outside (0, 1) (0 or rows_out = NULL: off)",
            (double)gamma);
    if (int rc = check_setter_rows("covo_set_step_sigma_adapt", on, n_inst)) return rc;
    REQUIRE(!on || ((uintptr_t)rows_out & 15) == 0, "covo_set_step_sigma_adapt: rows_out must be 16-byte aligned");
    h->adapt_gamma = on ? gamma : 0.0f;
    h->adapt_rows = on ? rows_out : nullptr;
    h->adapt_n = on ? n_inst : 0;
    h->sigma_age = 0;
    ++h->opt.epoch;
    return 0;
}

// ---- the episode logs of the attachments' rows (episode_rows.hip).  The copy is one eager launch of the episode drivers behind the
// step: attaching or detaching a log changes no captured step graph
int covo_set_episode_rows(covo_handle_t h, int32_t kind, float *log, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_rows: null handle");
    REQUIRE(kind >= 0 && kind < COVO_EPLOG_KINDS, "covo_set_episode_rows: kind=%d outside [0, %d) (COVO_EPLOG_*)", kind, COVO_EPLOG_KINDS);
    return set_episode_log(h, kind, log, stride, "covo_set_episode_rows: stride=%d");
}

// the box form of every sweep a step of this handle runs (riccati.hip).  The sweep's launches are eager and follow the step; a change
// of the switch still bumps the epoch, so no captured step graph outlives it.  What the step needs next to it is checked at the step
int covo_set_step_riccati_box(covo_handle_t h, int32_t *masks, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_riccati_box: null handle");
    if (masks == nullptr) {
        if (h->box_masks != nullptr) ++h->opt.epoch;
        h->box_masks = nullptr;
        h->box_n = 0;
        return 0;
    }
    if (int rc = check_setter_rows("covo_set_step_riccati_box", true, n_inst)) return rc;
    REQUIRE(covo_riccati_on(h) && n_inst <= h->riccati_n,
            "covo_set_step_riccati_box: n_inst=%d needs the Riccati refinement attached on the handle with at least as many instances "
            "(covo_set_step_riccati: %d)", n_inst, h->riccati_n);
    if (h->box_masks == nullptr) ++h->opt.epoch;
    h->box_masks = masks;
    h->box_n = n_inst;
    return 0;
}

// ---- the per-iteration logs of the iLQR steps (ilqr.hip).  Their launches are eager and follow the step: no epoch bump
int covo_set_step_ilqr(covo_handle_t h, float *rows, float *fb_rows, float *summary, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_ilqr: null handle");
    const bool on = rows != nullptr || fb_rows != nullptr || summary != nullptr;
    if (int rc = check_setter_rows("covo_set_step_ilqr", on, n_inst)) return rc;
    h->ilqr_rows = rows;
    h->ilqr_fb_rows = fb_rows;
    h->ilqr_summary = summary;
    h->ilqr_n = on ? n_inst : 0;
    return 0;
}

int covo_set_step_ilqr_box(covo_handle_t h, int32_t *counts, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_ilqr_box: null handle");
    if (int rc = check_setter_rows("covo_set_step_ilqr_box", counts != nullptr, n_inst)) return rc;
    h->ilqr_box = counts;
    h->ilqr_box_n = counts ? n_inst : 0;
    return 0;
}

int covo_debug_ilqr_costs(covo_handle_t h, float *costs, int32_t n_inst)
{
    REQUIRE(h, "covo_debug_ilqr_costs: null handle");
    if (int rc = check_setter_rows("covo_debug_ilqr_costs", costs != nullptr, n_inst)) return rc;
    h->ilqr_costs = costs;
    h->ilqr_costs_n = costs ? n_inst : 0;
    return 0;
}

int covo_step_plan_age(covo_handle_t h, int32_t *next_age, int32_t *last_age)
{
    REQUIRE(h, "covo_step_plan_age: null handle");
    if (next_age) *next_age = covo_plan_hold(h) > 1 ? h->plan_age : 0;
    if (last_age) *last_age = h->plan_last_age;
    return 0;
}

int covo_set_episode_hold_log(covo_handle_t h, float *log, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_hold_log: null handle");
    // (a missing plan hold is reported ahead of a bad stride)
    REQUIRE(log == nullptr || covo_plan_hold(h) > 1, "%s", covo_eplog_kinds[COVO_EPLOG_HOLD].off);
    return set_episode_log(h, COVO_EPLOG_HOLD, log, stride, "covo_set_episode_hold_log: stride=%d");
}

}  // extern "C"
