// step_graph_check.cpp -- the host-only state machines of covo_mpc_amd/csrc/step_graph.hpp without a device: the HIP entry points they
// call are stubs that record what happened, the pass / between callables record what was enqueued where.  Built with
// -fsanitize=address,undefined and run by tests/test_host.py::test_step_graph_state_machines_under_a_sanitizer.
//   hipcc --offload-host-only -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all -O1 -g -std=c++17 step_graph_check.cpp
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../covo_mpc_amd/csrc/step_graph.hpp"

static std::string g_log;  // one letter per event: b/e capture begin/end, i instantiate, L graph launch, d graph destroyed,
                           // 0..9 pass j on the caller's stream, a..  pass j on the capture stream, ^ between (caller's stream)
static int g_live_graphs = 0;
static hipStream_t const CALLER = (hipStream_t)0x10, SIDE = (hipStream_t)0x20;

hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode) { g_log += (s == SIDE) ? 'b' : '?'; return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *g) { g_log += 'e'; *g = (hipGraph_t) new int(1); return hipSuccess; }
hipError_t hipGraphInstantiate(hipGraphExec_t *x, hipGraph_t, hipGraphNode_t *, char *, size_t)
{
    g_log += 'i';
    *x = (hipGraphExec_t) new int(2);
    ++g_live_graphs;
    return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t s) { g_log += (s == CALLER) ? 'L' : '?'; return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t x) { delete (int *)x; --g_live_graphs; g_log += 'd'; return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t g) { delete (int *)g; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
void covo_set_error(const char *, ...) {}
static bool g_eligible = false;
bool step_small_eligible(const covo_ctx *, const covo_env_params &, const covo_step_args &) { return g_eligible; }

static int g_failed = 0;
#define EXPECT(cond, ...)                                                      \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond);       \
            std::printf(__VA_ARGS__);                                          \
            std::printf("\n");                                                 \
            ++g_failed;                                                        \
        }                                                                      \
    } while (0)

// an owner like StepState: two caches, a key each, recorded as step_enqueue_all records it
struct Owner {
    GraphCache cache[2] = {};
    int key[2] = {0, 0};
};
static std::string step(covo_ctx *h, Owner &o, bool reuse, int key)
{
    g_log.clear();
    GraphCache &c = o.cache[reuse];
    const bool same = graph_cache_seen(c, o.key[reuse] == key);
    if (!same) o.key[reuse] = key;
    const int rc = step_run_passes(
        h, o.cache, reuse, same, CALLER, "check",
        [&](hipStream_t on, int j) { g_log += (char)((on == CALLER ? '0' : 'a') + j); return 0; },
        [&](hipStream_t on, int) { g_log += (on == CALLER) ? '^' : '?'; return 0; });
    EXPECT(rc == 0, "rc=%d", rc);
    return g_log;
}

static void drive(int K, bool arbiter, bool no_graph)
{
    covo_ctx h{};
    float log_buf[16], arb_buf[8];
    h.cfg.flags = no_graph ? COVO_FLAG_NO_GRAPH : 0;
    h.side_stream = SIDE;
    h.iters = K;
    h.iter_log = K > 1 ? log_buf : nullptr;
    h.arb_out = arbiter ? arb_buf : nullptr;
    const bool eager_only = no_graph || (K > 1 && arbiter);
    const std::string eager = K == 1 ? "0" : (arbiter ? "0^1^2" : "012");
    const std::string capture = eager_only ? eager : (K == 1 ? "baeiL" : "babceiL");
    const std::string replay = eager_only ? eager : "L";
    Owner o;
    char tag[64];
    std::snprintf(tag, sizeof(tag), "K=%d arbiter=%d no_graph=%d", K, (int)arbiter, (int)no_graph);
    // eager -> capture -> replay, for the refresh graph ...
    EXPECT(step(&h, o, false, 7) == eager, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, false, 7) == capture, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, false, 7) == replay, "%s: %s", tag, g_log.c_str());
    // ... and independently for the reuse graph, which starts with an eager call of its own and leaves the other alone
    EXPECT(step(&h, o, true, 7) == eager, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, false, 7) == replay, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, true, 7) == capture, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, true, 7) == replay, "%s: %s", tag, g_log.c_str());
    EXPECT(g_live_graphs == (eager_only ? 0 : 2), "%s: %d graphs", tag, g_live_graphs);
    // a changed key: the stale graph goes before anything is enqueued, the sequence starts again -- for that graph only
    EXPECT(step(&h, o, false, 8) == (eager_only ? eager : "d" + eager), "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, true, 7) == replay, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, false, 8) == capture, "%s: %s", tag, g_log.c_str());
    EXPECT(step(&h, o, false, 8) == replay, "%s: %s", tag, g_log.c_str());
    // step_graphs_drop: both forgotten, both start again
    o.cache[0].forget(), o.cache[1].forget();
    EXPECT(g_live_graphs == 0, "%s: %d graphs", tag, g_live_graphs);
    for (int reuse = 0; reuse < 2; ++reuse) {
        EXPECT(step(&h, o, reuse, reuse ? 7 : 8) == eager, "%s: %s", tag, g_log.c_str());
        EXPECT(step(&h, o, reuse, reuse ? 7 : 8) == capture, "%s: %s", tag, g_log.c_str());
        EXPECT(step(&h, o, reuse, reuse ? 7 : 8) == replay, "%s: %s", tag, g_log.c_str());
    }
    // the arbiter attached to an iterated step whose graphs exist: both go, the passes run eagerly with the arbiter between them;
    // detached again, the sequence starts again
    if (!no_graph && K > 1 && !arbiter) {
        h.arb_out = arb_buf;
        EXPECT(step(&h, o, false, 8) == "dd0^1^2", "%s: %s", tag, g_log.c_str());
        EXPECT(g_live_graphs == 0, "%s: %d graphs", tag, g_live_graphs);
        h.arb_out = nullptr;
        EXPECT(step(&h, o, false, 8) == eager, "%s: %s", tag, g_log.c_str());
        EXPECT(step(&h, o, false, 8) == capture, "%s: %s", tag, g_log.c_str());
    }
    o.cache[0].forget(), o.cache[1].forget();
    EXPECT(g_live_graphs == 0, "%s: %d graphs left", tag, g_live_graphs);
}

static void forms()
{
    covo_env_params p{};
    covo_step_args a{};
    for (int no_graph = 0; no_graph < 2; ++no_graph)
        for (int mode : {COVO_MODE_COVO_ONLINE, COVO_MODE_COVO_OFFLINE, COVO_MODE_MPPI})
            for (int eligible = 0; eligible < 2; ++eligible)
                for (int staged = 0; staged < 2; ++staged)
                    for (int fold = 0; fold < 2; ++fold)
                        for (int tables = 0; tables < 2; ++tables)
                            for (int reuse = 0; reuse < 2; ++reuse) {
                                covo_ctx h{};
                                h.cfg.flags = no_graph ? COVO_FLAG_NO_GRAPH : 0;
                                h.opt.fuse_small = 1;
                                h.opt.fold_begin = fold;
                                h.elite_K = staged ? 4 : 0;
                                float rows[COVO_ELITE_FLOATS];
                                h.elite_own = rows;
                                g_eligible = eligible && mode != COVO_MODE_COVO_ONLINE;
                                a.mode = mode;
                                p.disturb_kind = tables ? COVO_DISTURB_PERIODIC : COVO_DISTURB_GAUSSIAN;
                                const bool small = step_takes_small(&h, p, a);
                                EXPECT(small == (g_eligible && !staged), "small");
                                StepForm want = STEP_BEGIN_PASSES;
                                if (no_graph && small) want = STEP_ONE_LAUNCH;
                                else if (no_graph && fold && mode == COVO_MODE_COVO_ONLINE && !tables && !reuse) want = STEP_FOLDED_ONLINE;
                                EXPECT(step_form(&h, small, p, a, reuse) == want, "no_graph=%d mode=%d eligible=%d staged=%d fold=%d tables=%d reuse=%d",
                                       no_graph, mode, eligible, staged, fold, tables, reuse);
                            }
}

int main()
{
    for (int K : {1, 3})
        for (int arbiter = 0; arbiter < 2; ++arbiter)
            for (int no_graph = 0; no_graph < 2; ++no_graph) drive(K, arbiter, no_graph);
    forms();
    std::printf("%s\n", g_failed ? "step_graph_check: FAILED" : "step_graph_check: ok");
    return g_failed ? 1 : 0;
}
