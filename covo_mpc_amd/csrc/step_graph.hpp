// step_graph.hpp -- the host-only state machines of the step layer (step.hip): the capture-once / replay graph
// cache, the pass driver every iterated step runs through, and the one answer to "which form does this single step take".  No
// kernel and no device memory in here: tests/host/step_graph_check.cpp compiles this file against stubbed HIP entry points and
// walks the three under a sanitizer.
#pragma once
#include "covo_common.hpp"
#include "step_small.hpp"

// ---- the capture-once / replay cache every step path embeds (StepState and BatchState: two, the step and the reuse step of a Sigma
// period; BatchSmall: one).  The owner compares and records its key itself (the keys differ) and tells graph_cache_run whether it is
// unchanged:
//   unchanged, graph present                    hipGraphLaunch on the caller's stream, nothing else
//   unchanged, no graph, COVO_FLAG_NO_GRAPH clear   capture the step on h->side_stream, instantiate, launch on the caller's stream
//   otherwise                                   a changed key drops the graph before anything is enqueued; eager on the caller's stream
// so the first call with new buffers runs eagerly (all one-time attribute calls / allocations happen there), the second captures,
// later ones replay.
struct GraphCache {
    bool have_key, have_graph;  // have_key: an eager call with the owner's current key has run
    hipGraph_t graph;
    hipGraphExec_t exec;
    void drop()
    {
        if (!have_graph) return;
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        have_graph = false;
    }
    void forget()  // the next call runs eagerly, the one after captures again
    {
        drop();
        have_key = false;
    }
};

// key bookkeeping of an owner for one of its caches.  key_same: the owner's key equals the one it recorded (which it then overwrites
// if not); the cache adds whether it has run with it -- two caches on one key (BatchState) each start with an eager call
static inline bool graph_cache_seen(GraphCache &c, bool key_same)
{
    const bool same = key_same && c.have_key;
    c.have_key = true;
    return same;
}

// enqueue(stream) enqueues the step.  Capture is on the library's own stream (the caller's may be the legacy default stream, which
// cannot capture); nothing executes during capture, the graph is then launched on the caller's stream.  A failed capture leaves
// the cache without a graph.
template <class Enqueue>
static int graph_cache_run(covo_ctx *h, GraphCache &c, hipStream_t s, bool same, const char *name, Enqueue enqueue)
{
    if (!same) c.drop();
    if (c.have_graph) {
        COVO_CHECK_HIP(hipGraphLaunch(c.exec, s));
        return 0;
    }
    if (!same || (h->cfg.flags & COVO_FLAG_NO_GRAPH) != 0) return enqueue(s);
    hipStream_t cs = h->side_stream;
    COVO_CHECK_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue(cs);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc == 0 && e != hipSuccess) covo_set_error("%s: stream capture failed: %s", name, hipGetErrorString(e));
    if (rc == 0 && e == hipSuccess && (e = hipGraphInstantiate(&c.exec, g, nullptr, nullptr, 0)) != hipSuccess)
        covo_set_error("%s: hipGraphInstantiate failed: %s", name, hipGetErrorString(e));
    if (rc != 0 || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        return rc ? rc : (int)e;
    }
    c.graph = g;
    c.have_graph = true;
    COVO_CHECK_HIP(hipGraphLaunch(c.exec, s));
    return 0;
}

// ---- the pass driver of the single and the env-batched covo-online step.  covo_set_step_iters: K passes on one state, all in the
// step's graph -- cache[0], or cache[1] for the reuse step of a Sigma period (another launch set).  pass(stream, j) enqueues pass j.
// With the update arbiter, the Newton refinement or the Riccati refinement attached their launches sit between the passes: between(stream, j) enqueues them
// behind pass j < K - 1; they are eager by nature (their arguments are the step's), so the passes are then enqueued eagerly too and
// both graphs are forgotten.
// same: graph_cache_seen(cache[reuse], ...) of this call.
template <class Pass, class Between>
static int step_run_passes(covo_ctx *h, GraphCache (&cache)[2], bool reuse, bool same, hipStream_t s, const char *name, Pass pass,
                           Between between)
{
    const int K = covo_step_iters(h);
    auto passes = [&](hipStream_t on, bool with_between) -> int {
        for (int j = 0; j < K; ++j) {
            int rc = pass(on, j);
            if (rc == 0 && with_between && j + 1 < K) rc = between(on, j);
            if (rc) return rc;
        }
        return 0;
    };
    if (K > 1 && (covo_arb_on(h) || covo_refine_on(h) || covo_riccati_on(h))) {
        cache[0].forget(), cache[1].forget();
        return passes(s, true);
    }
    return graph_cache_run(h, cache[reuse ? 1 : 0], s, same, name, [&](hipStream_t on) { return passes(on, false); });
}

// ---- which form a single step takes.  The two shortcuts exist on an eager handle (COVO_FLAG_NO_GRAPH) only; neither runs the begin
// launch, so neither leaves the state copy / shifted mean / keys in the scratch a captured or replayed launch reads.
enum StepForm {
    STEP_ONE_LAUNCH,     // covo-offline / MPPI at small N: the whole step is the one launch of step_small.hip
    STEP_FOLDED_ONLINE,  // covo-online: the begin work rides in the Hessian's first launch (COVO_FOLD_BEGIN=0: off)
    STEP_BEGIN_PASSES,   // the begin launch, then the passes (graph or eager)
};
// covo-offline / MPPI: noise -> rollout -> records -> merge fit ONE launch (a staged update -- ESS floor, standardised temperature, elite
// set -- does not; nor does a step under the annealed schedule: that launch shifts and factors a_cov itself)
static inline bool step_takes_small(const covo_ctx *h, const covo_env_params &p, const covo_step_args &a)
{
    return h->opt.fuse_small && step_small_eligible(h, p, a) && !covo_update_staged(h) && !covo_anneal_sched_on(h);
}
// small: step_takes_small; reuse: a reuse step of a Sigma period has no Hessian launch to fold into; per-step force tables: their launch precedes the Hessian
// and reads the scalars the begin launch leaves
static inline StepForm step_form(const covo_ctx *h, bool small, const covo_env_params &p, const covo_step_args &a, bool reuse)
{
    if ((h->cfg.flags & COVO_FLAG_NO_GRAPH) == 0) return STEP_BEGIN_PASSES;
    if (small) return STEP_ONE_LAUNCH;
    if (h->opt.fold_begin && a.mode == COVO_MODE_COVO_ONLINE && !covo_needs_tables(p) && !reuse) return STEP_FOLDED_ONLINE;
    return STEP_BEGIN_PASSES;
}
