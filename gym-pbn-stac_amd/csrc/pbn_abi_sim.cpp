// pbn_abi_sim.cpp -- everything that advances a plain batch: step mode and its HIP graphs, rollout,
// replay / forced updates, MT mode, the synchronous step and the SSD histogram.
// step_launch stays next to pbn_step and the graph capture: single-env and small-batch stepping are
// launch-bound on the host.
#include "pbn_host.hpp"

// The envs one step launch covers and the stream it goes to: the whole batch on the batch's stream, or one
// launch chain's slice (pbn_batch::Chains) on a stream of the caller's choice.
struct StepRange {
    uint64_t off, len;
    hipStream_t stream;
};
static StepRange whole_batch(const pbn_batch* b) { return {0, b->B, b->stream}; }
static StepRange chain_range(const pbn_batch* b, int c, hipStream_t stream) {
    return {b->step.sl[c].off, b->step.sl[c].len, stream};
}

// What one launch of the step kernels runs: T updates from update_base, drawn from Philox -- or, with `node`,
// along given node indices (replay: with their k53 draws; forced: without).
struct StepWork {
    uint32_t T = 1;
    uint64_t update_base = 0;
    bool timed = true;                    // ev_begin / ev_end around the launch
    const uint64_t* ubase_dev = nullptr;  // inside a step graph: the update counter is *ubase_dev + update_base
    const void* node = nullptr;
    const void* k53 = nullptr;
};
static StepWork updates(uint32_t T, uint64_t update_base, bool timed = true) { return {T, update_base, timed}; }
static StepWork graph_update(uint32_t k, const uint64_t* counter) { return {1, k, false, counter}; }
static StepWork given_updates(uint32_t T, uint64_t update_base, const void* node, const void* k53) {
    return {T, update_base, true, nullptr, node, k53};
}

static int step_launch(pbn_batch* b, const StepRange& r, const StepWork& w) {
    const uint32_t T = w.T;
    const bool replay = w.node != nullptr, timed = w.timed;
    StepArgs a{};
    a.ubase_dev = w.ubase_dev;
    a.state = b->d_state + r.off * (uint64_t)b->W;
    a.img = b->d_image;
    a.L = b->net->L;
    a.B = r.len;
    a.env_base = b->env_base + r.off;
    a.seed = b->seed;
    a.update_base = w.update_base;
    a.T = T;
    a.replay_node = (const uint32_t*)w.node;
    a.replay_k53 = (const uint64_t*)w.k53;
    hipEvent_t stop = nullptr;
    if (timed)
        if (int rc = b->ev_begin(&stop)) return rc;
    int store = STORE_FULL;
    if (T == 1 && !replay) {  // PBNSIM_STORE_MODE forces the write-back; by size otherwise (step_half_store)
        store = step_half_store(b->B, b->n_cu, b->step.block) ? STORE_HALF : STORE_DIRTY;
        if (b->knob.store_mode >= 0) store = b->knob.store_mode;
    }
    // step mode: K envs per thread (their loads overlap); rollout: one env per lane up to the
    // resident grid -- its T updates are the work, and more lanes hide more LDS latency
    // (Bittner-28 @65,536 envs, T = 256: 115 vs 62 G updates/s with K = 2)
    const bool rollout = T > 1 && !replay;  // k_rollout (or k_rollout_grp), 256-thread groups
    a.grp = rollout ? b->roll_group : 1;
    const uint64_t K = rollout ? 1u : (uint64_t)b->knob.envs_per_thread;
    const uint64_t lanes = rollout ? r.len * (uint64_t)a.grp : (r.len + K - 1) / K;
    const int sb = (replay || rollout) ? BLOCK : b->step.block;
    const int grid = replay    ? b->grid_for(lanes, b->bpc_base)
                     : rollout ? b->grid_for(lanes, b->bpc_roll, sb)
                               : b->grid_for(lanes, b->bpc_step, sb);
    int e = launch_step(b->W, a, store, replay, sb, grid, r.stream);
    if (e) return fail(PBN_E_HIP, "k_step launch: %s", hipGetErrorString((hipError_t)e));
    return timed ? b->ev_end(stop) : 0;
}

// Step mode is launch-bound between kernels (one HBM pass each): runs of step launches go out
// as captured HIP graphs -- the same kernels with the same arguments, except that the update
// counter comes from device memory (*ubase + k for launch k), so one instantiated graph per length
// serves every replay. Which calls use them, and how a call is cut into replays: pbn_step_plan.hpp.
//
// Captures n step launches of chain c's envs -- and, with `bump`, a k_bump of the chain's counter by n behind
// them -- into an instantiated exec, uploaded on `upload_on` if given. Captured on the batch's stream (a
// captured launch keeps no stream); the launches read chain c's own counter, so one chain's k_bump never
// races another chain's reads. A graph holds one chain only: it is a linear run of kernels.
static bool capture_steps(pbn_batch* b, int c, uint32_t n, bool bump, hipStream_t upload_on, hipGraphExec_t* out) {
    uint64_t* counter = (uint64_t*)b->sg.ubase.p + c;
    const StepRange r = chain_range(b, c, b->stream);
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    bool launched = ok;
    for (uint32_t k = 0; launched && k < n; ++k) launched = step_launch(b, r, graph_update(k, counter)) == 0;
    if (launched && bump) launched = launch_bump(counter, n, b->stream) == 0;
    if (ok) ok = hipStreamEndCapture(b->stream, &g) == hipSuccess && launched && g;
    if (ok) ok = hipGraphInstantiate(out, g, nullptr, nullptr, 0) == hipSuccess;
    if (ok && upload_on) ok = hipGraphUpload(*out, upload_on) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    return ok;
}

// A failed capture is not the caller's error: the call goes on with the graphs it has, or plain launches. The
// family is marked, so later calls do not capture n launches to fail again.
static void capture_failed(bool& family_broken) {
    family_broken = true;
    (void)hipGetLastError();
    g_err.clear();
}

// The power-of-two graphs: lengths 64, 32, ..., 2 of every chain, with the k_bump that moves the chain's counter
// on for the next replay of the call; all captured at the first call that replays one.
static bool step_graph_ready(pbn_batch* b, bool may_capture) {
    if (b->sg.built) return true;
    if (b->sg.broken || !may_capture) return false;
    if (b->sg.ubase.ensure(64)) return false;
    bool ok = true;
    for (int c = 0; ok && c < b->step.chains; ++c)
        for (int j = 0; ok && j < STEP_GRAPH_SIZES; ++j)
            ok = capture_steps(b, c, STEP_GRAPH_K >> j, true, nullptr, &b->sg.graph[c][j]);
    if (!ok) {
        for (auto& chain : b->sg.graph) destroy_graph_execs(chain);
        capture_failed(b->sg.broken);
        return false;
    }
    b->sg.built = true;
    return true;
}

// Captures n step launches as one graph per launch chain in a free (or the least recently used) exact-length
// slot. Returns the slot, or -1 (plain launches / power-of-two graphs then).
static int exact_graph_build(pbn_batch* b, uint32_t n) {
    if (!step_exact_fits(n) || b->sg.broken || b->sg.exact_broken) return -1;
    if (b->sg.ubase.ensure(64)) return -1;
    // capture and instantiate into fresh execs first: a failed capture leaves the cached graphs as they were
    // no k_bump: pbn_step writes the device counter before every replay of an exact graph
    // upload now, on the stream that will replay it, so the first replay (e.g. a timed one) does not pay for it
    hipGraphExec_t x[STEP_CHAINS_MAX] = {};
    bool ok = true;
    for (int c = 0; ok && c < b->step.chains; ++c) ok = capture_steps(b, c, n, false, b->chain_stream(c), &x[c]);
    // the extra chains' uploads are done before anything below may destroy an exec (setup, not a replay loop)
    for (int c = 1; c < b->step.chains; ++c) (void)hipStreamSynchronize(b->ch.stream[c]);
    if (!ok) {
        destroy_graph_execs(x);
        capture_failed(b->sg.exact_broken);
        return -1;
    }
    int slot = 0;
    for (int j = 1; j < pbn_batch::StepGraphs::EXACT_GRAPHS; ++j)
        if (b->sg.exact_used[j] < b->sg.exact_used[slot]) slot = j;
    if (b->sg.exact_graph[slot][0]) {
        // the evicted execs may still be queued or running from an earlier asynchronous pbn_step
        // (HIP documents no deferred free): drain the stream first -- every call joined its chains
        // into it. Eviction happens only at capture time, never in a steady replay loop.
        if (hipStreamSynchronize(b->stream) != hipSuccess) {
            destroy_graph_execs(x);
            (void)fail(PBN_E_HIP, "stream sync before graph eviction failed");
            return -1;
        }
        destroy_graph_execs(b->sg.exact_graph[slot]);
    }
    for (int c = 0; c < STEP_CHAINS_MAX; ++c) b->sg.exact_graph[slot][c] = x[c];
    b->sg.exact_n[slot] = n;
    b->sg.exact_used[slot] = ++b->sg.exact_clock;
    return slot;
}

static int exact_graph_find(pbn_batch* b, uint32_t n) {
    for (int j = 0; j < pbn_batch::StepGraphs::EXACT_GRAPHS; ++j)
        if (b->sg.exact_graph[j][0] && b->sg.exact_n[j] == n) return j;
    return -1;
}

static bool stream_capturing(pbn_batch* b) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (b->stream && hipStreamIsCapturing(b->stream, &cap) != hipSuccess) return true;
    return cap != hipStreamCaptureStatusNone;
}

// every chain's device counter <- update_count (one tiny kernel on the batch's stream, ahead of the fork)
static int upload_update_count(pbn_batch* b) {
    if (int e = launch_set_counters((uint64_t*)b->sg.ubase.p, b->update_count, (uint32_t)b->step.chains, b->stream))
        return fail(PBN_E_HIP, "k_set_counters launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

// A chained call's fork: the extra chains' streams wait for everything queued on the batch's stream so far.
static int chains_fork(pbn_batch* b) {
    HIP_TRY(hipEventRecord(b->ch.fork, b->stream));
    for (int c = 1; c < b->step.chains; ++c) HIP_TRY(hipStreamWaitEvent(b->ch.stream[c], b->ch.fork, 0));
    return 0;
}

// ... and its join: whatever is queued on the batch's stream next waits for every chain's launches.
static int chains_join(pbn_batch* b) {
    for (int c = 1; c < b->step.chains; ++c) {
        HIP_TRY(hipEventRecord(b->ch.done[c], b->ch.stream[c]));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->ch.done[c], 0));
    }
    return 0;
}

// Queues the launches of one pbn_step call: one exact graph, or the power-of-two graphs and the plain rest, or
// plain launches only. A chained call queues each replay and each launch once per chain, alternating chains:
// each chain's stream holds its own launches in update order.
static int step_issue(pbn_batch* b, uint32_t n_updates, const StepCall& plan, int exact, bool pow2) {
    const int S = plan.chained ? b->step.chains : 1;
    if (exact >= 0) {
        for (int c = 0; c < S; ++c) HIP_TRY(hipGraphLaunch(b->sg.exact_graph[exact][c], b->chain_stream(c)));
        b->sg.exact_used[exact] = ++b->sg.exact_clock;
        b->update_count += n_updates;
        return 0;
    }
    StepPow2 d;
    if (pow2) d = step_pow2(n_updates);
    else d.plain = n_updates;
    for (int j = 0; j < STEP_GRAPH_SIZES; ++j)
        for (uint32_t q = 0; q < d.replays[j]; ++q) {
            for (int c = 0; c < S; ++c) HIP_TRY(hipGraphLaunch(b->sg.graph[c][j], b->chain_stream(c)));
            b->update_count += STEP_GRAPH_K >> j;
        }
    // a run's launches were accounted by pbn_step; any other call's launch takes its own event pair
    for (uint32_t q = 0; q < d.plain; ++q, ++b->update_count)
        for (int c = 0; c < S; ++c) {
            const StepRange r = plan.chained ? chain_range(b, c, b->chain_stream(c)) : whole_batch(b);
            if (int rc = step_launch(b, r, updates(1, b->update_count, !plan.run))) return rc;
        }
    return 0;
}

// Replay / forced node indices name an updatable node (truth-table networks never update node 0); k53, if given, < 2^53.
static int check_replay_nodes(const pbn_batch* b, const char* what, const uint32_t* node_idx, const uint64_t* k53,
                              uint64_t n) {
    const uint32_t lo = (uint32_t)b->net->kind == PBN_KIND_PROB_TABLE ? 1u : 0u;
    for (uint64_t q = 0; q < n; q++) {
        if (node_idx[q] >= (uint32_t)b->N || node_idx[q] < lo)
            return fail(PBN_E_RANGE, "%s node index %u outside [%u, %d)", what, node_idx[q], lo, b->N);
        if (k53 && k53[q] >> 53) return fail(PBN_E_RANGE, "replay k53 must be < 2^53");
    }
    return 0;
}

extern "C" {

int pbn_step_prepare(pbn_batch* b, uint32_t n_updates) {
    CHECK_NN(b, "batch");
    if (n_updates > PBN_STEP_PREPARE_MAX)
        return fail(PBN_E_INVALID, "n_updates=%u above PBN_STEP_PREPARE_MAX", n_updates);
    SET_DEV(b);
    // the call this prepares comes later, in a timing mode of its own: planned as an untimed one. On a failed
    // capture pbn_step falls back to plain launches
    if (!step_call(b->step, n_updates, 0, stream_capturing(b), !b->stream).capture) return 0;
    if (!step_exact_fits(n_updates)) (void)step_graph_ready(b, true);
    else if (exact_graph_find(b, n_updates) < 0) (void)exact_graph_build(b, n_updates);
    return 0;
}

int pbn_step(pbn_batch* b, uint32_t n_updates) {
    CHECK_NN(b, "batch");
    SET_DEV(b);
    const StepCall plan = step_call(b->step, n_updates, b->tm.mode, stream_capturing(b), !b->stream);
    int exact = -1;
    if (plan.graphs) {
        exact = exact_graph_find(b, n_updates);
        // a length seen twice in a row gets its own graph (an RL loop's fixed step count)
        if (exact < 0 && plan.capture && n_updates == b->sg.last_n) exact = exact_graph_build(b, n_updates);
    }
    b->sg.last_n = n_updates;
    const bool pow2 = plan.graphs && exact < 0 && step_graph_ready(b, plan.capture);
    if (exact >= 0 || pow2)
        if (int rc = upload_update_count(b)) return rc;
    // a run counts as n_updates launches (one per step, not per replay or per chain), all accounted here; the
    // region's start, like its stop, is recorded on the batch's stream: ahead of the fork, behind the join
    if (plan.run && b->tm.mode == 2) {
        hipEvent_t stop;  // stays null: a region's stop is recorded when it closes
        if (int rc = b->ev_begin(&stop)) return rc;
        b->tm.region_launches += n_updates - 1;  // ev_begin counted one
    }
    if (plan.chained)
        if (int rc = chains_fork(b)) return rc;
    int rc = step_issue(b, n_updates, plan, exact, pow2);
    if (plan.chained) {  // also after a failed launch: what was queued on the chains stays ordered
        const int jrc = chains_join(b);
        if (!rc) rc = jrc;
    }
    return rc;
}

int pbn_rollout(pbn_batch* b, uint32_t n_updates) {
    CHECK_NN(b, "batch");
    if (!n_updates) return 0;
    SET_DEV(b);
    if (int rc = step_launch(b, whole_batch(b), updates(n_updates, b->update_count))) return rc;
    b->update_count += n_updates;
    return 0;
}

int pbn_step_replay(pbn_batch* b, const uint32_t* node_idx, const uint64_t* k53, uint32_t n_updates) {
    CHECK_NN(b, "batch");
    if (!n_updates) return 0;
    CHECK_NN(node_idx, "node_idx");
    CHECK_NN(k53, "k53");
    const uint64_t n = (uint64_t)n_updates * b->B;
    if (int rc = check_replay_nodes(b, "replay", node_idx, k53, n)) return rc;
    SET_DEV(b);
    if (int rc = b->s_replay_i.ensure(4 * n)) return rc;
    if (int rc = b->s_replay_k.ensure(8 * n)) return rc;
    HIP_TRY(hipMemcpyAsync(b->s_replay_i.p, node_idx, 4 * n, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->s_replay_k.p, k53, 8 * n, hipMemcpyHostToDevice, b->stream));
    if (int rc = step_launch(b, whole_batch(b), given_updates(n_updates, 0, b->s_replay_i.p, b->s_replay_k.p))) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_step_forced(pbn_batch* b, const uint32_t* node_idx, uint32_t n_updates) {
    CHECK_NN(b, "batch");
    if (!n_updates) return 0;
    CHECK_NN(node_idx, "node_idx");
    const uint64_t n = (uint64_t)n_updates * b->B;
    if (int rc = check_replay_nodes(b, "forced", node_idx, nullptr, n)) return rc;
    SET_DEV(b);
    if (int rc = b->s_replay_i.ensure(4 * n)) return rc;
    HIP_TRY(hipMemcpyAsync(b->s_replay_i.p, node_idx, 4 * n, hipMemcpyHostToDevice, b->stream));
    // replay-mode kernel with no k53 array: update t takes the choice word of Philox step update
    // update_count + t (the draw pbn_step would use), so the stream stays in step with pbn_step
    if (int rc = step_launch(b, whole_batch(b), given_updates(n_updates, b->update_count, b->s_replay_i.p, nullptr))) return rc;
    b->update_count += n_updates;
    HIP_TRY(hipStreamSynchronize(b->stream));  // the staging buffer is reused by the next call
    return 0;
}

static MTArgs mt_args(pbn_batch* b) {
    MTArgs a{};
    a.state = b->d_state;
    a.img = b->d_image;
    a.L = b->net->L;
    a.B = b->B;
    a.n_nodes = b->N;
    a.mt_py = (uint32_t*)b->mt.py.p;
    a.mt_np = (uint32_t*)b->mt.np.p;
    a.pos_py = (uint32_t*)b->mt.pos_py.p;
    a.pos_np = (uint32_t*)b->mt.pos_np.p;
    a.lane_walk = b->knob.mt_lane_walk ? 1 : 0;
    return a;
}

int pbn_mt_seed(pbn_batch* b, const uint64_t* seeds, int init_state) {
    CHECK_NN(b, "batch");
    CHECK_NN(seeds, "seeds");
    const bool table = b->net->kind == PBN_KIND_PROB_TABLE;
    if (table)  // np.random.seed(s) accepts 0 <= s < 2^32 only
        for (uint64_t e = 0; e < b->B; e++)
            if (seeds[e] >> 32) return fail(PBN_E_RANGE, "Seed must be between 0 and 2**32 - 1 (env %llu)",
                                            (unsigned long long)e);
    SET_DEV(b);
    const size_t row = 4 * ((size_t)MT_ROW * b->B + MT_TAIL_PAD);
    if (int rc = b->mt.py.ensure(row)) return rc;
    if (int rc = b->mt.pos_py.ensure(4 * b->B)) return rc;
    if (table) {
        if (int rc = b->mt.np.ensure(row)) return rc;
        if (int rc = b->mt.pos_np.ensure(4 * b->B)) return rc;
    }
    if (int rc = b->mt.seeds.ensure(8 * b->B)) return rc;
    HIP_TRY(hipMemcpyAsync(b->mt.seeds.p, seeds, 8 * b->B, hipMemcpyHostToDevice, b->stream));
    MTArgs a = mt_args(b);
    a.seeds = (const uint64_t*)b->mt.seeds.p;
    if (int rc = timed_launch(b, "k_mt_seed", [&] { return launch_mt_seed(b->W, a, b->grid_all(b->B), b->stream); }))
        return rc;
    if (init_state) {  // genRandState / PBN.reset(None): the step kernel's init draws
        a.init_state = 1;
        if (int rc = timed_launch(b, "k_mt_step (init)", [&] { return launch_mt_step(b->W, a, b->n_cu, b->stream); }))
            return rc;
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->mt.ready = 1;
    return 0;
}

int pbn_mt_step(pbn_batch* b, uint32_t n_updates) {
    CHECK_NN(b, "batch");
    if (!b->mt.ready) return fail(PBN_E_STATE, "pbn_mt_seed has not been called");
    if (!n_updates) return 0;
    SET_DEV(b);
    MTArgs a = mt_args(b);
    a.T = n_updates;
    return timed_launch(b, "k_mt_step", [&] { return launch_mt_step(b->W, a, b->n_cu, b->stream); });
}

// ------------------------------------------------------------------ synchronous update
int pbn_synch_step(pbn_batch* b, uint32_t n_steps, const uint32_t* perturb_gap_thr) {
    CHECK_NN(b, "batch");
    if (!n_steps) return 0;
    if (perturb_gap_thr)
        for (int k = 1; k < b->N; k++)
            if (perturb_gap_thr[k] > perturb_gap_thr[k - 1])
                return fail(PBN_E_INVALID, "perturb_gap_thr must be non-increasing");
    SET_DEV(b);
    SyncArgs a{};
    a.state = b->d_state;
    a.img = b->d_image;
    a.L = b->net->L;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.step_base = b->aux.sync_steps;
    a.T = n_steps;
    if (perturb_gap_thr) {
        if (int rc = b->aux.sync_tab.ensure(4 * (size_t)b->N)) return rc;
        HIP_TRY(hipMemcpyAsync(b->aux.sync_tab.p, perturb_gap_thr, 4 * (size_t)b->N, hipMemcpyHostToDevice,
                               b->stream));
        a.gap_thr = (const uint32_t*)b->aux.sync_tab.p;
        a.gap_inv_log2 = gap_inv_log2(perturb_gap_thr, b->N);
    }
    a.lds_bytes = sync_layout(b->W, b->net->L.bytes, b->N, &a);
    if (a.lds_bytes > 160u * 1024u) return fail(PBN_E_UNSUPPORTED, "sync LDS footprint %u B too large", a.lds_bytes);
    const int grid = b->grid_for(b->B, b->bpc_base);
    if (int rc = timed_launch(b, "k_sync", [&] { return launch_sync(b->W, a, grid, b->stream); })) return rc;
    b->aux.sync_steps += n_steps;
    if (perturb_gap_thr) HIP_TRY(hipStreamSynchronize(b->stream));  // table buffer is reused by later calls
    return 0;
}

// ------------------------------------------------------------------ SSD histogram
int pbn_ssd_run(pbn_batch* b, const int32_t* target_nodes, int n_targets, const uint32_t* flip_gap_thr,
                uint32_t iters, uint64_t* hist) {
    CHECK_NN(b, "batch");
    CHECK_NN(target_nodes, "target_nodes");
    CHECK_NN(hist, "hist");
    if (n_targets < 1 || n_targets > 12) return fail(PBN_E_UNSUPPORTED, "n_targets=%d outside [1, 12]", n_targets);
    for (int j = 0; j < n_targets; j++) {
        if (target_nodes[j] < 0 || target_nodes[j] >= b->N)
            return fail(PBN_E_RANGE, "target node %d out of range [0, %d)", target_nodes[j], b->N);
        for (int q = 0; q < j; q++)
            if (target_nodes[q] == target_nodes[j]) return fail(PBN_E_INVALID, "duplicate target node %d", target_nodes[j]);
    }
    if (flip_gap_thr)
        for (int k = 1; k < b->N; k++)
            if (flip_gap_thr[k] > flip_gap_thr[k - 1]) return fail(PBN_E_INVALID, "flip_gap_thr must be non-increasing");
    SET_DEV(b);
    const size_t nb = (size_t)1 << n_targets;
    if (int rc = b->aux.ssd_hist.ensure(8 * nb)) return rc;
    if (int rc = b->aux.ssd_tab.ensure(4 * (size_t)b->N + 4 * (size_t)n_targets)) return rc;
    uint32_t* d_gap = (uint32_t*)b->aux.ssd_tab.p;
    int32_t* d_tgt = (int32_t*)(d_gap + b->N);
    if (flip_gap_thr) HIP_TRY(hipMemcpyAsync(d_gap, flip_gap_thr, 4 * (size_t)b->N, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(d_tgt, target_nodes, 4 * (size_t)n_targets, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemsetAsync(b->aux.ssd_hist.p, 0, 8 * nb, b->stream));
    SSDArgs a{};
    a.state = b->d_state;
    a.img = b->d_image;
    a.L = b->net->L;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.iter_base = b->aux.ssd_iters;
    a.iters = iters;
    a.n_targets = n_targets;
    a.targets = d_tgt;
    a.gap_thr = flip_gap_thr ? d_gap : nullptr;
    a.gap_inv_log2 = flip_gap_thr ? gap_inv_log2(flip_gap_thr, b->N) : 0.0f;
    a.hist = (uint64_t*)b->aux.ssd_hist.p;
    a.error = b->d_error;
    HIP_TRY(hipMemsetAsync(b->d_error, 0, 4, b->stream));
    // one wave per env while the batch is small against the chip (the reference's 300 resets).
    // Crossovers measured on MI355X (tools/ssd_mode_sweep.py, Bittner-200, p = 0.01, G transitions/s):
    // 4,096 envs shared 19.4 / wave 16.4 / lane 0.9; 16,384: 18.4 / 19.8 / 3.8; 65,536: - / 20.1 / 14.7;
    // 262,144: - / 19.8 / 39.4
    a.wave = b->knob.ssd_wave >= 0 ? b->knob.ssd_wave : (b->B <= (uint64_t)b->n_cu * 256u ? 1 : 0);
    a.dag = a.wave && !b->knob.ssd_serial && (b->net->kind == PBN_KIND_PREDICTOR_MIX || b->net->kmax <= SSD_DAG_KMAX) ? 1 : 0;
    // chunk resolution with the workgroup's 4 waves on one env while even that leaves SIMDs free
    if (a.dag && (b->knob.ssd_shared >= 0 ? b->knob.ssd_shared > 0 : b->B <= (uint64_t)b->n_cu * 8u))
        a.dag = b->knob.ssd_shared > 1 ? b->knob.ssd_shared : SSD_SHARED_WAVES;
    a.lds_bytes = ssd_layout(b->W, b->net->L.bytes, b->N, n_targets, &a);
    if (a.lds_bytes > 160u * 1024u) return fail(PBN_E_UNSUPPORTED, "SSD LDS footprint %u B too large", a.lds_bytes);
    const uint64_t envs_per_block = a.dag > 1 ? 1u : BLOCK / 64;
    const int grid = a.wave ? (int)std::min<uint64_t>((b->B + envs_per_block - 1) / envs_per_block, (uint64_t)b->n_cu * 8u)
                            : b->grid_for(b->B, b->bpc_base);
    if (int rc = timed_launch(b, "k_ssd", [&] { return launch_ssd(b->W, a, grid, b->stream); })) return rc;
    std::vector<uint64_t> h(nb);
    int32_t err = 0;
    HIP_TRY(hipMemcpyAsync(h.data(), b->aux.ssd_hist.p, 8 * nb, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(&err, b->d_error, 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (err) return fail(PBN_E_HIP, "k_ssd_wave: a wave timed out waiting for its turn (internal error)");
    for (size_t k = 0; k < nb; k++) hist[k] += h[k];
    b->aux.ssd_iters += iters;
    return 0;
}

}  // extern "C"
