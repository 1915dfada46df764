// step_attach_check.cpp -- the attachment layer of covo_mpc_amd/csrc/step_attach.hip without a device: the seven check_* functions a
// step runs before it launches and the setters that only record on the handle, on hand-built handles and argument blocks.  Prints
// one line per case; tests/test_host.py::test_step_attachment_checks_under_a_sanitizer builds it with -fsanitize=address,undefined and
// compares the output to tests/golden/step_refusals.txt.  Four parts: every refusal once (function | case | rc | text); the order
// (each pair of refusals that are neighbours in a function's order, both arranged: the earlier text is expected); the clean cases;
// the setters (rc, epoch bump, dropped logs, schedule fields per transition, and their own refusals).
//   hipcc --offload-host-only -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all -O1 -g -std=c++17 step_attach_check.cpp
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>
#include "../../covo_mpc_amd/csrc/step_attach.hip"

static float *R;    // every attached float buffer points into main's stack array (16-byte aligned): nothing dereferences it
static int32_t *I;  // ... and every int32 buffer
static float *odd() { return R + 1; }  // not 16-byte aligned

static char g_err[1024];
void covo_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int g_failed = 0;
#define EXPECT(cond, ...)                                                \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                    \
            std::printf("\n");                                           \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

// a bare handle as covo_create leaves it (zeroed, its own rows), n valid instances, and the argument blocks of a covo-online step
struct Fx {
    covo_ctx h{};
    covo_env_params p[3]{};
    covo_step_args a{};        // check_single_step's; check_step_attachments and check_ilqr_step get its fields the way that one passes them
    covo_batch_mode_args m{};  // check_batch_step's (plain: m.base alone, as covo_mpc_step_batched passes it)
    int n;
    bool fused = false, env_step = false, plain = false;
    int first_row = 0, n_steps = 8;  // check_episode_logs'
    bool exchange = false;           // what the stubs answer
    const char *small_why = nullptr;
    int small_which = 0;
    explicit Fx(int n_inst) : n(n_inst)
    {
        h.cfg.n_local = 256;
        h.cfg.H = COVO_H;
        h.cfg.du = COVO_DU;
        h.cfg.lam = 0.01f;
        h.diag_scratch = h.lam_own = h.elite_own = R;
        for (covo_env_params &q : p) {
            q.reward_kind = COVO_REWARD_PENYAW;
            q.disturb_kind = COVO_DISTURB_NONE;
            q.disturb_period = 50;
            q.max_steps_in_episode = 300;
        }
        a.mode = m.mode = COVO_MODE_COVO_ONLINE;
        a.n_samples = m.base.n_samples = 256;
        a.T = m.base.T = 320;
        a.state = m.base.states = R;
        a.pos_traj = m.base.pos_traj = R;
        a.vel_traj = m.base.vel_traj = R;
        a.a_mean = m.base.a_mean = R;
        a.a_cov = m.base.a_cov = R;
        a.a = m.base.a = R;
        a.cost = m.base.cost = R;
        a.groupmin = m.base.groupmin = R;
        a.gamma_mean = m.base.gamma_mean = 1.0f;
        a.sample_sigma = m.base.sample_sigma = 0.5f;
        a.derive_keys = 1;
        m.base.n_envs = n;
    }
    Fx(const Fx &) = delete;
};
static const Fx *g_fx = nullptr;
bool exchange_ready(const covo_ctx *) { return g_fx->exchange; }
const char *batch_small_refusal(const covo_ctx *, const covo_batch_mode_args *, const covo_env_params *, int *which)
{
    *which = g_fx->small_which;
    return g_fx->small_why;
}

enum Fn { MODEL, ATTACH, ILQR, EPLOGS, SINGLE, BMODELS, BATCH };
static int call(Fn fn, Fx &f, std::string *text)
{
    g_fx = &f;
    g_err[0] = 0;
    const covo_step_args &a = f.a;
    covo_batch_mode_args norm;
    int rc = 0;
    switch (fn) {
    case MODEL: rc = check_model(&f.p[0], "walk"); break;
    case ATTACH:
        rc = check_step_attachments(&f.h, a.n_samples, f.n, a.partial_out != nullptr, a.derive_keys, a.mode, a.a_cov, f.p, "walk",
                                    a.gamma_sigma, f.fused);
        break;
    case ILQR: rc = check_ilqr_step(&f.h, f.n, a.partial_out != nullptr, a.derive_keys, "walk"); break;
    case EPLOGS: rc = check_episode_logs(&f.h, f.first_row, f.n_steps, "walk"); break;
    case SINGLE: rc = check_single_step(&f.h, f.p, &a, "walk"); break;
    case BMODELS: rc = check_batch_models(f.p, f.n, f.env_step, "walk"); break;
    case BATCH: rc = check_batch_step(&f.h, &f.m.base, f.plain ? nullptr : &f.m, f.p, f.env_step, "walk", &norm); break;
    }
    *text = g_err;
    return rc;
}

// ---- what the cases are arranged from.  An attachment goes on once, with exactly f.n rows: a case that arranges its offence behind
// another case's keeps what that one set
static void set_mode(Fx &f, int mode)
{
    f.a.mode = f.m.mode = mode;
    if (mode == COVO_MODE_COVO_OFFLINE) {
        f.a.L_table = f.m.L_table = R;
        f.a.n_table = f.m.n_table = 1;
    }
}
static void sampling(Fx &f) { if (f.m.mode == COVO_MODE_COVO_ONLINE) set_mode(f, COVO_MODE_MPPI); }  // a batch that is not covo-online
static void staged(Fx &f) { sampling(f); f.h.batched_staged = 1; }
static void shard(Fx &f) { f.a.partial_out = R; }
static void eplog(Fx &f, int kind, int stride) { f.h.eplog[kind].log = R; f.h.eplog[kind].stride = stride; }
static void diag(Fx &f) { if (!f.h.diag_out) { f.h.diag_out = R; f.h.diag_n = f.n; } }
static void plan(Fx &f) { if (!f.h.plan_out) { f.h.plan_out = R; f.h.plan_n = f.n; } }
static void fan(Fx &f) { if (!f.h.fan_out) { f.h.fan_out = R; f.h.fan_K = 4; f.h.fan_n = f.n; } }
static void arb(Fx &f) { if (!f.h.arb_out) { f.h.arb_out = R; f.h.arb_mask = 7; f.h.arb_n = f.n; } }
static void ess(Fx &f) { if (f.h.ess_min == 0.0f) { f.h.ess_min = 4.0f; f.h.lam_out = R; f.h.lam_n = f.n; } }
static void elite(Fx &f) { if (!f.h.elite_K) { f.h.elite_K = 4; f.h.elite_out = R; f.h.elite_n = f.n; } }
static void iters(Fx &f) { if (!f.h.iter_log) { f.h.iters = 3; f.h.iter_log = R; f.h.iter_n = f.n; } }
static void period(Fx &f) { if (f.h.sigma_period <= 1) f.h.sigma_period = 2; }
static void post(Fx &f) { if (!f.h.post_cov_out) { f.h.post_cov_out = f.h.post_aux_out = R; f.h.post_n = f.n; } }
static void adapt_rows(Fx &f) { if (!f.h.adapt_rows) { f.h.adapt_rows = R; f.h.adapt_gamma = 0.5f; f.h.adapt_n = f.n; } }
static void adapt(Fx &f) { period(f); post(f); adapt_rows(f); }
static void refine(Fx &f) { if (!f.h.refine_out) { f.h.refine_out = R; f.h.refine_n = f.n; } }
static void riccati(Fx &f) { if (!f.h.riccati_out) { f.h.riccati_out = R; f.h.riccati_n = f.n; } }
static void feedback(Fx &f) { riccati(f); if (!f.h.feedback_out) { f.h.feedback_out = R; f.h.feedback_n = f.n; } }
static void box(Fx &f) { riccati(f); if (!f.h.box_masks) { f.h.box_masks = I; f.h.box_n = f.n; } }
static void hold(Fx &f) { riccati(f); if (f.h.plan_hold <= 1) { f.h.plan_hold = 2; f.h.hold_rows = R; f.h.hold_n = f.n; } }
static void ilqr_mode(Fx &f) { set_mode(f, COVO_MODE_ILQR); riccati(f); }
static void ilqr_logs(Fx &f)
{
    ilqr_mode(f);
    f.h.ilqr_rows = f.h.ilqr_fb_rows = f.h.ilqr_summary = f.h.ilqr_costs = R;
    f.h.ilqr_box = I;
    f.h.ilqr_n = f.h.ilqr_costs_n = f.h.ilqr_box_n = f.n;
}
static void anneal(Fx &f)  // (one pass: the bare handle's iters)
{
    if (f.h.anneal_passes) return;
    set_mode(f, COVO_MODE_MPPI);
    f.h.anneal_passes = f.h.anneal_sched = 1;
    f.h.anneal_rows = R;
    f.h.anneal_n = f.n;
}
static void nodes(Fx &f) { anneal(f); if (!f.h.nodes_M) { f.h.nodes_M = 4; f.h.nodes_passes = f.h.anneal_passes; } }
// the logs next to the attachments they follow, n_steps rows each (not the elite and hold logs: their attachments exclude the ESS
// floor's and the Sigma period's)
static void logs(Fx &f)
{
    fan(f), arb(f), ess(f), iters(f), period(f), post(f);
    for (int k = 0; k < COVO_EPLOG_ALL; ++k)
        if (k != COVO_EPLOG_ELITE && k != COVO_EPLOG_HOLD) eplog(f, k, f.n_steps);
}

// ---- the refusals, per function in its documented order.  apart: why this refusal and the NEXT one of the list cannot both hold
struct Case {
    const char *tag;
    void (*arrange)(Fx &);
    const char *apart;
};
#define C(tag, ...) {tag, [](Fx &f) { __VA_ARGS__; }, nullptr}
#define X(tag, apart, ...) {tag, [](Fx &f) { __VA_ARGS__; }, apart}

static const std::vector<Case> model_cases = {
    C("reward_kind", f.p[0].reward_kind = 7),
    X("disturb_kind", "the period is read of a valid disturbance kind only", f.p[0].disturb_kind = 9),
    C("disturb_period", f.p[0].disturb_kind = COVO_DISTURB_PERIODIC; f.p[0].disturb_period = 0),
};

static const std::vector<Case> attach_cases = {
    C("sharded: diagnostics", shard(f); diag(f)),
    C("sharded: plan", shard(f); plan(f)),
    C("sharded: fan", shard(f); fan(f)),
    C("sharded: arbiter", shard(f); arb(f)),
    C("sharded: ESS floor", shard(f); ess(f)),
    C("sharded: iterations", shard(f); iters(f)),
    C("sharded: elite set", shard(f); elite(f)),
    C("sharded: Sigma period", shard(f); period(f)),
    C("sharded: posterior covariance", shard(f); post(f)),
    C("sharded: Sigma adapt", shard(f); adapt_rows(f)),
    C("sharded: Newton refinement", shard(f); refine(f)),
    C("sharded: Riccati refinement", shard(f); riccati(f)),
    X("sharded: episode rows", "a diagnostic target on a sharded step is the first refusal of the sharded block", shard(f);
      eplog(f, COVO_EPLOG_LAM, 8)),
    C("diagnostic rows", diag(f); f.h.diag_n = 2),
    C("plan rows", plan(f); f.h.plan_n = 2),
    C("fan K above n_samples", fan(f); f.h.fan_K = 64; f.a.n_samples = 32),
    C("fan rows", fan(f); f.h.fan_n = 2),
    C("arbiter rows", arb(f); f.h.arb_n = 2),
    C("ESS range", ess(f); f.h.ess_min = 0.5f),
    C("temperature rows", ess(f); f.h.lam_n = 2),
    C("elite set + ESS floor", elite(f); ess(f)),
    C("elite K range", elite(f); f.h.elite_K = 300),
    C("elite rows", elite(f); f.h.elite_n = 2),
    C("iteration log rows", iters(f); f.h.iter_n = 2),
    C("iterations without derive_keys", iters(f); f.a.derive_keys = 0),
    C("Sigma period off covo-online", period(f); set_mode(f, COVO_MODE_MPPI)),
    C("Sigma period a_cov alignment", period(f); f.a.a_cov = odd()),
    C("posterior covariance rows", post(f); f.h.post_n = 2),
    C("Sigma adapt off covo-online", adapt_rows(f); set_mode(f, COVO_MODE_COVO_OFFLINE)),
    C("Sigma adapt without a period", adapt_rows(f); f.h.sigma_period = 1),
    C("Sigma adapt without post_cov", adapt_rows(f); period(f); f.h.post_cov_out = nullptr),
    X("Sigma adapt rows", "the Newton refinement's mode refusal needs a step off covo-online, which Sigma adapt refuses first",
      adapt(f); f.h.adapt_n = 2),
    X("Newton refinement off covo-online", "a Sigma period off covo-online is refused by the period's own mode check first",
      refine(f); set_mode(f, COVO_MODE_MPPI)),
    C("Newton refinement + Sigma period", refine(f); period(f)),
    C("Newton refinement rows", refine(f); f.h.refine_n = 2),
    C("Newton refinement a_cov alignment", refine(f); f.a.a_cov = odd()),
    C("Riccati + Newton refinement", riccati(f); refine(f)),
    X("Riccati rows", "feedback without the Riccati refinement needs it detached", riccati(f); f.h.riccati_n = 2),
    C("feedback without Riccati", feedback(f); f.h.riccati_out = nullptr),
    C("feedback rows", feedback(f); f.h.feedback_n = 2),
    X("feedback plant", "the box without the Riccati refinement needs it detached, which the feedback rows refuse first", feedback(f);
      f.p[1].disturb_kind = COVO_DISTURB_DRAG),
    C("box without Riccati", box(f); f.h.riccati_out = nullptr),
    X("box rows", "the plan hold without the Riccati refinement needs it detached, which the box masks refuse first", box(f);
      f.h.box_n = 2),
    C("plan hold without Riccati", hold(f); f.h.riccati_out = nullptr),
    C("plan hold + Sigma period", hold(f); period(f)),
    C("plan hold plant", hold(f); f.p[2].disturb_kind = COVO_DISTURB_MIXED),
    C("plan hold rows", hold(f); f.h.hold_n = 2),
    C("nodes without a schedule", nodes(f); f.h.anneal_sched = 0),
    C("nodes pass count", nodes(f); f.h.nodes_passes = 2),
    C("nodes range", nodes(f); f.h.nodes_M = 33),
    C("anneal off MPPI", anneal(f); set_mode(f, COVO_MODE_COVO_ONLINE)),
    C("anneal pass count", anneal(f); f.h.anneal_passes = 2),
    C("anneal + gamma_sigma", anneal(f); f.a.gamma_sigma = 0.5f),
    X("anneal temperature + ESS floor", "the elite set next to the ESS floor is refused as that pair first", anneal(f);
      f.h.anneal_temp = 1.0f; ess(f)),
    X("anneal temperature + elite set", "a sharded step refuses the elite set in its sharded block", anneal(f); f.h.anneal_temp = 1.0f;
      elite(f)),
    C("anneal sharded", anneal(f); shard(f)),
    C("anneal fused batch", anneal(f); f.fused = true),
    C("anneal rows", anneal(f); f.h.anneal_n = 2),
};

static const std::vector<Case> ilqr_cases = {
    C("sharded", shard(f)),
    C("without Riccati", f.h.riccati_out = nullptr),
    C("Newton refinement", riccati(f); refine(f)),
    C("diagnostics", riccati(f); diag(f)),
    C("fan", riccati(f); fan(f)),
    C("arbiter", riccati(f); arb(f)),
    C("ESS floor", riccati(f); ess(f)),
    C("elite set", riccati(f); elite(f)),
    C("Sigma period", riccati(f); period(f)),
    C("posterior covariance", riccati(f); post(f)),
    C("Sigma adapt", riccati(f); adapt_rows(f)),
    C("without derive_keys", riccati(f); f.a.derive_keys = 0),
    C("log rows", riccati(f); f.h.ilqr_summary = R; f.h.ilqr_n = 2),
    C("cost rows", riccati(f); f.h.ilqr_costs = R; f.h.ilqr_costs_n = 2),
    C("box count rows", riccati(f); f.h.ilqr_box = I; f.h.ilqr_box_n = 2),
};

// (rows [0, 8) of a log of 4)
static const std::vector<Case> eplog_cases = {
    C("diagnostic log", eplog(f, COVO_EPLOG_DIAG, 4)),          C("trace", eplog(f, COVO_EPLOG_TRACE, 4)),
    C("fan log", eplog(f, COVO_EPLOG_FAN, 4)),                  C("arbiter log", eplog(f, COVO_EPLOG_ARB, 4)),
    C("temperature log", eplog(f, COVO_EPLOG_LAM, 4)),          C("elite log", eplog(f, COVO_EPLOG_ELITE, 4)),
    C("iteration log", eplog(f, COVO_EPLOG_ITERS, 4)),          C("Sigma log", eplog(f, COVO_EPLOG_SIGMA, 4)),
    C("posterior side-row log", eplog(f, COVO_EPLOG_POST_AUX, 4)), C("posterior covariance log", eplog(f, COVO_EPLOG_POST_COV, 4)),
    C("hold log", eplog(f, COVO_EPLOG_HOLD, 4)),
};
static const std::vector<Case> eplog_extra = {
    C("a negative first row", eplog(f, COVO_EPLOG_TRACE, 64); f.first_row = -1),
};

static const std::vector<Case> single_cases = {
    C("mode", f.a.mode = 4),
    C("n_samples", f.a.n_samples = 257),
    C("null buffer", f.a.state = nullptr),
    X("offline without L_table", "MPPI's a_cov is asked of another mode", f.a.mode = COVO_MODE_COVO_OFFLINE; f.a.L_table = nullptr),
    C("MPPI without a_cov", f.a.mode = COVO_MODE_MPPI; f.a.a_cov = nullptr),
    C("check_model's", f.p[0].reward_kind = 7),
    C("gamma_sigma off MPPI", f.a.gamma_sigma = 0.5f),
    C("tables without derive_keys", f.p[0].disturb_kind = COVO_DISTURB_PERIODIC; f.a.derive_keys = 0),
    C("plan hold alignment", f.h.plan_hold = 2; f.a.a_mean = odd()),
    C("check_ilqr_step's", f.a.mode = COVO_MODE_ILQR; f.h.riccati_out = nullptr),
    C("check_step_attachments'", plan(f); f.h.plan_n = 0),
};

static const std::vector<Case> bmodels_cases = {
    C("check_model's", f.p[1].disturb_kind = COVO_DISTURB_PERIODIC; f.p[1].disturb_period = 0),
    C("instance differs", f.p[1].reward_kind = COVO_REWARD_REALWORLD),
};
static const std::vector<Case> bmodels_extra = {
    C("instance differs, env step", f.env_step = true; f.p[2].reset_traj = COVO_TRAJ_ZIGZAG),
};

// check_batch_step's three paths behind its common head: the fused MPPI / covo-offline launch, the staged one, the iLQR step
static const std::vector<Case> batch_cases = {
    C("n_envs", f.m.base.n_envs = COVO_MAX_ENVS + 1),
    C("n_samples", f.m.base.n_samples = 257),
    C("mode", f.m.mode = 4),
    C("null buffer", f.m.base.states = nullptr),
    C("check_batch_models'", f.p[1].reward_kind = COVO_REWARD_REALWORLD),
    C("fused: ESS floor", sampling(f); ess(f)),
    C("fused: elite set", sampling(f); elite(f)),
    C("fused: iterations + arbiter", sampling(f); iters(f); arb(f)),
    C("fused: posterior covariance", sampling(f); post(f)),
    C("Riccati off covo-online", sampling(f); riccati(f)),
    C("plan hold alignment", sampling(f); f.h.plan_hold = 2; f.m.base.a_mean = odd()),
    C("check_step_attachments'", sampling(f); plan(f); f.h.plan_n = 2),
    X("MPPI without a_cov", "covo-offline's table is asked of another mode", set_mode(f, COVO_MODE_MPPI); f.m.base.a_cov = nullptr),
    C("covo-offline without L_table", set_mode(f, COVO_MODE_COVO_OFFLINE); f.m.L_table = nullptr),
    C("fused launch refusal", sampling(f); f.small_why = "the stub's reason"; f.small_which = 2),
};
static const std::vector<Case> batch_staged_cases = {
    C("staged: covo-offline without L_table", staged(f); set_mode(f, COVO_MODE_COVO_OFFLINE); f.m.L_table = nullptr),
    C("staged: groupmin", staged(f); f.m.base.groupmin = nullptr),
    C("staged: gamma_sigma off MPPI", staged(f); set_mode(f, COVO_MODE_COVO_OFFLINE); f.m.gamma_sigma = 0.5f),
    C("staged: gamma_sigma + elite set", staged(f); f.m.gamma_sigma = 0.5f; elite(f)),
    C("staged: sharded handle", staged(f); f.exchange = true),
};
static const std::vector<Case> batch_ilqr_cases = {
    C("iLQR: check_batch_models'", ilqr_mode(f); f.p[1].reward_kind = COVO_REWARD_REALWORLD),
    C("iLQR: check_ilqr_step's", ilqr_mode(f); diag(f)),
    C("iLQR: plan hold alignment", ilqr_mode(f); f.h.plan_hold = 2; f.m.base.a_mean = odd()),
    C("iLQR: check_step_attachments'", ilqr_mode(f); plan(f); f.h.plan_n = 2),
};

// a refusal's text with its numbers blanked: the later offence of a pair may change a value the earlier text prints (K=300 for K=4)
static std::string shape(const std::string &text)
{
    std::string out;
    for (const char c : text)
        if (c < '0' || c > '9') out += c;
        else if (out.empty() || out.back() != '#') out += '#';
    return out;
}

static int g_refusals = 0, g_pairs = 0, g_apart = 0;
static void walk(Fn fn, const char *name, int n, const std::vector<Case> &cases, bool ordered = true)
{
    std::vector<std::string> alone;
    std::string text;
    for (const Case &c : cases) {
        Fx f(n);
        c.arrange(f);
        const int rc = call(fn, f, &text);
        std::printf("%s | %s | %d | %s\n", name, c.tag, rc, text.c_str());
        EXPECT(rc == COVO_E_BADARG && !text.empty(), "%s | %s: rc=%d", name, c.tag, rc);
        alone.push_back(text);
        ++g_refusals;
    }
    for (size_t i = 0; ordered && i + 1 < cases.size(); ++i) {
        const Case &first = cases[i], &second = cases[i + 1];
        ++g_pairs;
        if (first.apart != nullptr) {
            std::printf("order | %s | %s > %s | cannot coexist: %s\n", name, first.tag, second.tag, first.apart);
            ++g_apart;
            continue;
        }
        Fx f(n);
        second.arrange(f);
        first.arrange(f);
        const int rc = call(fn, f, &text);
        std::printf("order | %s | %s > %s | %d | %s\n", name, first.tag, second.tag, rc, text.c_str());
        EXPECT(shape(text) == shape(alone[i]), "%s: %s and %s arranged: %s", name, first.tag, second.tag, text.c_str());
    }
}

static void clean(Fn fn, const char *tag, int n, void (*arrange)(Fx &))
{
    Fx f(n);
    if (arrange != nullptr) arrange(f);
    if (fn == BATCH && f.m.mode == COVO_MODE_MPPI && f.h.anneal_passes) f.h.batched_staged = 1;  // (the annealed step's batch)
    std::string text;
    const int rc = call(fn, f, &text);
    std::printf("clean | %s, %d instance%s | %d%s%s\n", tag, n, n == 1 ? "" : "s", rc, text.empty() ? "" : " | ", text.c_str());
    EXPECT(rc == 0 && text.empty(), "%s: rc=%d %s", tag, rc, text.c_str());
}

static void clean_cases()
{
    clean(SINGLE, "single covo-online", 1, nullptr);
    clean(SINGLE, "single MPPI", 1, [](Fx &f) { set_mode(f, COVO_MODE_MPPI); });
    clean(SINGLE, "single covo-offline", 1, [](Fx &f) { set_mode(f, COVO_MODE_COVO_OFFLINE); });
    clean(SINGLE, "single iLQR with Riccati rows", 1, ilqr_mode);
    clean(EPLOGS, "episode logs, none attached", 1, nullptr);
    for (int n : {1, 3}) {
        clean(BMODELS, "batch models", n, nullptr);
        clean(BATCH, "batched covo-online (covo_batch_args alone)", n, [](Fx &f) { f.plain = true; });
        clean(BATCH, "batched covo-online", n, nullptr);
        clean(BATCH, "batched fused MPPI", n, [](Fx &f) { set_mode(f, COVO_MODE_MPPI); });
        clean(BATCH, "batched fused covo-offline", n, [](Fx &f) { set_mode(f, COVO_MODE_COVO_OFFLINE); });
        clean(BATCH, "batched staged MPPI", n, staged);
        clean(BATCH, "batched staged covo-offline", n, [](Fx &f) { set_mode(f, COVO_MODE_COVO_OFFLINE); staged(f); });
        clean(BATCH, "batched iLQR with Riccati rows", n, ilqr_mode);
    }
    // each attachment alone (with what it cannot be without), in the mode it belongs to, with exactly enough rows
    static const struct { const char *name; void (*attach)(Fx &); } atts[] = {
        {"diagnostics", diag}, {"plan", plan}, {"fan", fan}, {"arbiter", arb}, {"ESS floor", ess}, {"elite set", elite},
        {"iterations", iters}, {"Sigma period", period}, {"posterior covariance", post}, {"Sigma adapt", adapt},
        {"Newton refinement", refine}, {"Riccati refinement", riccati}, {"Riccati feedback", feedback}, {"Riccati box", box},
        {"plan hold", hold}, {"iLQR logs", ilqr_logs}, {"annealed step", anneal}, {"spline nodes", nodes}, {"episode logs", logs}};
    for (const auto &at : atts) {
        const std::string single = std::string("single step + ") + at.name, batch = std::string("batched step + ") + at.name;
        clean(SINGLE, single.c_str(), 1, at.attach);
        clean(BATCH, batch.c_str(), 1, at.attach);
        clean(BATCH, batch.c_str(), 3, at.attach);
    }
    clean(EPLOGS, "episode logs of exactly n_steps rows", 3, logs);
}

// ---- the setters: off -> on, on -> the same again, on -> another buffer or value, on -> off; once with no episode log attached and
// once with all of them.  Before every transition the schedule fields stand at 5 and (second round) every log is attached again
struct Setter {
    const char *name;
    int (*on)(covo_ctx *), (*other)(covo_ctx *), (*off)(covo_ctx *);
    void (*before)(covo_ctx *);  // what the setter needs on the handle, or null
};
#define S(name, on, other, off) {#name, [](covo_ctx *h) { return name on; }, [](covo_ctx *h) { return name other; }, [](covo_ctx *h) { return name off; }, nullptr}
#define SB(name, before, on, other, off) {#name, [](covo_ctx *h) { return name on; }, [](covo_ctx *h) { return name other; }, [](covo_ctx *h) { return name off; }, [](covo_ctx *h) { before; }}
static const Setter setters[] = {
    S(covo_debug_set_stream_gemm, (h, 1), (h, 2), (h, 0)),
    S(covo_debug_set_fuse_small, (h, 1), (h, 2), (h, 0)),
    S(covo_debug_set_fold_begin, (h, 1), (h, 2), (h, 0)),
    S(covo_debug_set_ns_deflate, (h, 1), (h, 2), (h, 0)),
    S(covo_debug_set_ns_merged, (h, 1), (h, 2), (h, 0)),
    S(covo_debug_set_ns_coherence, (h, 1), (h, 2), (h, 0)),
    S(covo_set_step_batched_staged, (h, 1), (h, 2), (h, 0)),
    S(covo_set_step_diag, (h, R, 3), (h, R + 4, 2), (h, nullptr, 0)),
    S(covo_set_episode_diag_log, (h, R, 8), (h, R + 4, 16), (h, nullptr, 0)),
    S(covo_set_step_ess_floor, (h, 4.0f, R, 3), (h, 8.0f, R, 3), (h, 0.0f, nullptr, 0)),
    S(covo_set_step_elite, (h, 4, R, 3), (h, 4, R + 4, 3), (h, 0, nullptr, 0)),
    S(covo_set_step_plan, (h, R, 3), (h, R + 4, 2), (h, nullptr, 0)),
    S(covo_set_episode_trace, (h, R, 8), (h, R + 4, 16), (h, nullptr, 0)),
    SB(covo_set_step_fan, h->fan_K = 4, (h, R, I, 4, 3), (h, R + 4, nullptr, 4, 2), (h, nullptr, nullptr, 0, 0)),
    SB(covo_set_episode_fan, h->fan_K = 4, (h, R, 8), (h, R + 4, 16), (h, nullptr, 0)),
    S(covo_set_step_arbiter, (h, R, 7, 3), (h, R, 1, 3), (h, nullptr, 0, 0)),
    SB(covo_set_episode_arbiter_log, h->arb_out = R, (h, R, 8), (h, R + 4, 16), (h, nullptr, 0)),
    S(covo_set_step_iters, (h, 3, R, 3), (h, 4, R, 3), (h, 1, nullptr, 0)),
    S(covo_set_step_sigma_period, (h, 4), (h, 8), (h, 1)),
    S(covo_set_step_sigma_adapt, (h, 0.5f, R, 3), (h, 0.25f, R, 3), (h, 0.0f, nullptr, 0)),
    SB(covo_set_episode_rows, h->ess_min = 4.0f, (h, COVO_EPLOG_LAM, R, 8), (h, COVO_EPLOG_LAM, R + 4, 16), (h, COVO_EPLOG_LAM, nullptr, 0)),
    SB(covo_set_step_riccati_box, h->riccati_out = R; h->riccati_n = 3, (h, I, 3), (h, I + 4, 2), (h, nullptr, 0)),
    S(covo_set_step_ilqr, (h, R, R, R, 3), (h, R, nullptr, nullptr, 2), (h, nullptr, nullptr, nullptr, 0)),
    S(covo_set_step_ilqr_box, (h, I, 3), (h, I + 4, 2), (h, nullptr, 0)),
    S(covo_debug_ilqr_costs, (h, R, 3), (h, R + 4, 2), (h, nullptr, 0)),
    SB(covo_set_episode_hold_log, h->plan_hold = 2; h->hold_rows = R, (h, R, 8), (h, R + 4, 16), (h, nullptr, 0)),
};

static covo_ctx bare_handle()
{
    covo_ctx h{};
    h.cfg.n_local = 256;
    h.diag_scratch = h.lam_own = h.elite_own = R;
    return h;
}

static void transition(const Setter &s, covo_ctx *h, bool with_logs, const char *tag, int (*step)(covo_ctx *))
{
    static const char *const kinds[COVO_EPLOG_ALL] = {"LAM", "ELITE", "ITERS", "SIGMA", "POST_AUX", "POST_COV", "DIAG", "TRACE", "FAN", "ARB", "HOLD"};
    bool had[COVO_EPLOG_ALL];
    for (int k = 0; k < COVO_EPLOG_ALL; ++k) {
        if (with_logs && h->eplog[k].log == nullptr) h->eplog[k].log = R + 8, h->eplog[k].stride = 8;
        had[k] = h->eplog[k].log != nullptr;
    }
    h->sigma_age = h->plan_age = 5;
    const int epoch = h->opt.epoch;
    g_err[0] = 0;
    const int rc = step(h);
    std::string dropped;
    for (int k = 0; k < COVO_EPLOG_ALL; ++k)
        if (had[k] && h->eplog[k].log == nullptr) dropped += std::string(dropped.empty() ? "" : " ") + kinds[k];
    std::printf("%s | %s | %s | rc=%d epoch+%d dropped=[%s] sigma_age=%d plan_age=%d%s%s\n", s.name, with_logs ? "every log attached" : "no log attached",
                tag, rc, h->opt.epoch - epoch, dropped.c_str(), h->sigma_age, h->plan_age, rc ? " | " : "", g_err);
}

static void refusal(const char *setter, const char *tag, int rc)
{
    std::printf("%s | %s | %d | %s\n", setter, tag, rc, g_err);
    EXPECT(rc == COVO_E_BADARG && g_err[0] != 0, "%s | %s: rc=%d", setter, tag, rc);
    g_err[0] = 0;
}
#define REFUSE(name, tag, before, ...)  \
    do {                                \
        covo_ctx ctx = bare_handle();   \
        covo_ctx *h = &ctx;             \
        before;                         \
        refusal(#name, tag, name(__VA_ARGS__)); \
    } while (0)

static void setter_cases()
{
    for (const Setter &s : setters)
        for (int with_logs = 0; with_logs < 2; ++with_logs) {
            covo_ctx h = bare_handle();
            if (s.before != nullptr) s.before(&h);
            transition(s, &h, with_logs, "off -> on", s.on);
            transition(s, &h, with_logs, "on -> same", s.on);
            transition(s, &h, with_logs, "on -> other", s.other);
            transition(s, &h, with_logs, "on -> off", s.off);
        }
    g_err[0] = 0;
    for (const Setter &s : setters) refusal(s.name, "null handle", s.on(nullptr));
    int32_t x = -1, y = -1;
    refusal("covo_step_sigma_age", "null handle", covo_step_sigma_age(nullptr, &x, &y));
    refusal("covo_step_plan_age", "null handle", covo_step_plan_age(nullptr, &x, &y));
    refusal("covo_step_nodes", "null handle", covo_step_nodes(nullptr, &x, &y));
    REFUSE(covo_step_nodes, "null outputs", , h, nullptr, &y);

    REFUSE(covo_set_step_diag, "n_inst = 0", , h, R, 0);
    REFUSE(covo_set_step_diag, "n_inst above COVO_MAX_ENVS", , h, R, COVO_MAX_ENVS + 1);
    REFUSE(covo_set_episode_diag_log, "stride = 0", , h, R, 0);
    REFUSE(covo_set_step_ess_floor, "ess_min negative", , h, -1.0f, R, 3);
    REFUSE(covo_set_step_ess_floor, "ess_min infinite", , h, __builtin_inff(), R, 3);
    REFUSE(covo_set_step_ess_floor, "ess_min NaN", , h, __builtin_nanf(""), R, 3);
    REFUSE(covo_set_step_ess_floor, "n_inst = 0", , h, 4.0f, R, 0);
    REFUSE(covo_set_step_elite, "K negative", , h, -1, R, 3);
    REFUSE(covo_set_step_elite, "n_inst above COVO_MAX_ENVS", , h, 4, R, COVO_MAX_ENVS + 1);
    REFUSE(covo_set_step_plan, "n_inst = 0", , h, R, 0);
    REFUSE(covo_set_episode_trace, "stride = 0", , h, R, 0);
    REFUSE(covo_set_step_fan, "K = 0 with a buffer", , h, R, nullptr, 0, 3);
    REFUSE(covo_set_step_fan, "K above COVO_FAN_MAX", , h, R, nullptr, COVO_FAN_MAX + 1, 3);
    REFUSE(covo_set_step_fan, "n_inst = 0", , h, R, nullptr, 4, 0);
    REFUSE(covo_set_step_fan, "K above n_local", h->cfg.n_local = 2, h, R, nullptr, 4, 3);
    REFUSE(covo_set_step_fan, "K differs from the attached log's", h->fan_K = 4; h->eplog[COVO_EPLOG_FAN].log = R, h, R, nullptr, 8, 3);
    REFUSE(covo_set_episode_fan, "stride = 0", h->fan_K = 4, h, R, 0);
    REFUSE(covo_set_episode_fan, "no fan size", , h, R, 8);
    REFUSE(covo_set_step_arbiter, "mask = 0", , h, R, 0, 3);
    REFUSE(covo_set_step_arbiter, "mask = 8", , h, R, 8, 3);
    REFUSE(covo_set_step_arbiter, "n_inst = 0", , h, R, 7, 0);
    REFUSE(covo_set_episode_arbiter_log, "stride = 0", h->arb_out = R, h, R, 0);
    REFUSE(covo_set_episode_arbiter_log, "no arbiter", , h, R, 8);
    REFUSE(covo_set_step_iters, "iters = 0", , h, 0, R, 3);
    REFUSE(covo_set_step_iters, "iters above COVO_MAX_STEP_ITERS", , h, COVO_MAX_STEP_ITERS + 1, R, 3);
    REFUSE(covo_set_step_iters, "n_inst = 0", , h, 3, R, 0);
    REFUSE(covo_set_step_sigma_period, "period = 0", , h, 0);
    REFUSE(covo_set_step_sigma_period, "period above COVO_MAX_SIGMA_PERIOD", , h, COVO_MAX_SIGMA_PERIOD + 1);
    REFUSE(covo_set_step_sigma_adapt, "gamma = 1", , h, 1.0f, R, 3);
    REFUSE(covo_set_step_sigma_adapt, "n_inst = 0", , h, 0.5f, R, 0);
    REFUSE(covo_set_step_sigma_adapt, "rows_out alignment", , h, 0.5f, odd(), 3);
    REFUSE(covo_set_episode_rows, "kind negative", , h, -1, R, 8);
    REFUSE(covo_set_episode_rows, "kind = COVO_EPLOG_KINDS", , h, COVO_EPLOG_KINDS, R, 8);
    REFUSE(covo_set_episode_rows, "stride = 0", h->ess_min = 4.0f, h, COVO_EPLOG_LAM, R, 0);
    for (int kind = 0; kind < COVO_EPLOG_KINDS; ++kind) {
        const std::string tag = "kind " + std::to_string(kind) + " without its attachment";
        REFUSE(covo_set_episode_rows, tag.c_str(), , h, kind, R, 8);
    }
    REFUSE(covo_set_step_riccati_box, "n_inst = 0", h->riccati_out = R; h->riccati_n = 3, h, I, 0);
    REFUSE(covo_set_step_riccati_box, "without Riccati", , h, I, 3);
    REFUSE(covo_set_step_riccati_box, "n_inst above the Riccati rows", h->riccati_out = R; h->riccati_n = 2, h, I, 3);
    REFUSE(covo_set_step_ilqr, "n_inst = 0", , h, R, nullptr, nullptr, 0);
    REFUSE(covo_set_step_ilqr_box, "n_inst = 0", , h, I, 0);
    REFUSE(covo_debug_ilqr_costs, "n_inst above COVO_MAX_ENVS", , h, R, COVO_MAX_ENVS + 1);
    REFUSE(covo_set_episode_hold_log, "no plan hold", , h, R, 8);
    REFUSE(covo_set_episode_hold_log, "no plan hold, stride = 0", , h, R, 0);
    REFUSE(covo_set_episode_hold_log, "stride = 0", h->plan_hold = 2; h->hold_rows = R, h, R, 0);

    // the three readers
    covo_ctx h = bare_handle();
    h.sigma_period = 4, h.sigma_age = 2, h.sigma_last_age = 1;
    h.plan_hold = 2, h.hold_rows = R, h.plan_age = 1, h.plan_last_age = 0;
    h.nodes_passes = 3, h.nodes_M = 8;
    int rc = covo_step_sigma_age(&h, &x, &y);
    std::printf("covo_step_sigma_age | period 4 at age 2 | %d | next=%d last=%d\n", rc, x, y);
    rc = covo_step_plan_age(&h, &x, &y);
    std::printf("covo_step_plan_age | hold 2 at age 1 | %d | next=%d last=%d\n", rc, x, y);
    rc = covo_step_nodes(&h, &x, &y);
    std::printf("covo_step_nodes | 3 passes of 8 nodes | %d | n_pass=%d n_nodes=%d\n", rc, x, y);
    h.sigma_period = 1, h.plan_hold = 1;
    rc = covo_step_sigma_age(&h, &x, nullptr) | covo_step_plan_age(&h, nullptr, &y);
    std::printf("covo_step_sigma_age, covo_step_plan_age | both off | %d | next=%d last=%d\n", rc, x, y);
}

int main()
{
    alignas(16) float rows[32];
    int32_t ints[8];
    R = rows;
    I = ints;
    walk(MODEL, "check_model", 1, model_cases);
    walk(ATTACH, "check_step_attachments", 3, attach_cases);
    walk(ILQR, "check_ilqr_step", 3, ilqr_cases);
    walk(EPLOGS, "check_episode_logs", 3, eplog_cases);
    walk(EPLOGS, "check_episode_logs", 3, eplog_extra, false);
    walk(SINGLE, "check_single_step", 1, single_cases);
    walk(BMODELS, "check_batch_models", 3, bmodels_cases);
    walk(BMODELS, "check_batch_models", 3, bmodels_extra, false);
    walk(BATCH, "check_batch_step", 3, batch_cases);
    walk(BATCH, "check_batch_step", 3, batch_staged_cases);
    walk(BATCH, "check_batch_step", 3, batch_ilqr_cases);
    std::printf("order | %d refusals, %d neighbour pairs, %d of them cannot coexist\n", g_refusals, g_pairs, g_apart);
    EXPECT(10 * g_apart <= g_pairs, "%d of %d pairs left out", g_apart, g_pairs);
    clean_cases();
    setter_cases();
    std::printf("%s\n", g_failed ? "step_attach_check: FAILED" : "step_attach_check: ok");
    return g_failed ? 1 : 0;
}
