// pbn_abi_reach.cpp -- attractor discovery (pbn_reach.hip): the pbn_reach_* entry points.
#include "pbn_host.hpp"

// The set of one network on one device; graph: TABLE_GRAPH_NONE for predictor mix, else the table graph.
static int reach_create(pbn_net* net, int device, uint64_t max_states, int graph, pbn_reach** out) {
    if (max_states < 1 || max_states > PBN_REACH_MAX_STATES)
        return fail(PBN_E_INVALID, "max_states=%llu outside [1, %llu]", (unsigned long long)max_states,
                    (unsigned long long)PBN_REACH_MAX_STATES);
    // the edge-rule kernels stage the whole image: one that does not fit is refused here, never launched
    if (net->L.bytes > REACH_LDS_MAX)
        return fail(PBN_E_UNSUPPORTED, "network image (%u B) exceeds the %u B of LDS the attractor kernels stage it in",
                    net->L.bytes, REACH_LDS_MAX);
    if (int rc = open_device(device)) return rc;
    pbn_reach* r = new pbn_reach;
    r->net = net;
    r->graph = graph;
    r->device = device;
    r->W = net->W;
    r->max_states = (uint32_t)max_states;
    // entries lost to publish races are dead until the next level hands them out again: room for one level's
    // worth (measured: up to ~1.3 per new state on a 2^19-state cube), and a floor for small sets
    r->key_cap = r->max_states + r->max_states / 2u + 65536u;
    r->fcap = keytable_pow2(r->key_cap);
    r->tcap = keytable_pow2(2ull * r->max_states);  // load factor <= 1/2 at max_states
    auto bail = [&](int code) {
        pbn_reach_destroy(r);
        return code;
    };
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(PBN_E_HIP, "hipStreamCreate"));
    if (hipHostMalloc((void**)&r->h_ctl, 4 * (REACH_CTL_WORDS + 1), hipHostMallocDefault) != hipSuccess)
        return bail(fail(PBN_E_NOMEM, "pinned control words"));
    int rc = 0;
    if ((rc = r->keys.ensure(8 * (size_t)r->W * r->key_cap)) || (rc = r->mark.ensure(4 * (size_t)r->key_cap)) ||
        (rc = r->queue.ensure(4 * (size_t)r->key_cap)) || (rc = r->free_ring.ensure(4 * (size_t)r->fcap)) ||
        (rc = r->table.ensure(8 * (size_t)r->tcap)) ||
        (rc = r->ctl.ensure(4 * REACH_CTL_WORDS)) || (rc = r->hull.ensure(16 * (size_t)r->W)))
        return bail(rc);
    if (hipMemsetAsync(r->table.p, 0, 8 * (size_t)r->tcap, r->stream) != hipSuccess ||
        hipMemsetAsync(r->ctl.p, 0, 4 * REACH_CTL_WORDS, r->stream) != hipSuccess ||
        hipStreamSynchronize(r->stream) != hipSuccess)
        return bail(fail(PBN_E_HIP, "hipMemset"));
    r->d_image = net->image_on(device);
    if (!r->d_image) return bail(fail(PBN_E_NOMEM, "network image upload failed"));
    r->complete = true;  // the empty set
    *out = r;
    return 0;
}

extern "C" {

int pbn_reach_create(const pbn_net* net_c, int device, uint64_t max_states, pbn_reach** out) {
    CHECK_NN(net_c, "net");
    CHECK_NN(out, "out");
    *out = nullptr;
    pbn_net* net = const_cast<pbn_net*>(net_c);
    if (net->kind != PBN_KIND_PREDICTOR_MIX)
        return fail(PBN_E_UNSUPPORTED, "attractor discovery covers predictor-mix networks here (truth-table networks "
                                       "have two support graphs: pbn_reach_create_table takes the choice)");
    return reach_create(net, device, max_states, TABLE_GRAPH_NONE, out);
}

int pbn_reach_create_table(const pbn_net* net_c, int device, uint64_t max_states, int32_t graph, pbn_reach** out) {
    CHECK_NN(net_c, "net");
    CHECK_NN(out, "out");
    *out = nullptr;
    pbn_net* net = const_cast<pbn_net*>(net_c);
    if (net->kind != PBN_KIND_PROB_TABLE)
        return fail(PBN_E_INVALID, "pbn_reach_create_table takes a truth-table network (predictor mix: pbn_reach_create)");
    if (graph != PBN_TABLE_GRAPH_STG && graph != PBN_TABLE_GRAPH_STEP)
        return fail(PBN_E_INVALID, "graph=%d is neither PBN_TABLE_GRAPH_STG nor PBN_TABLE_GRAPH_STEP", (int)graph);
    return reach_create(net, device, max_states, graph, out);
}

void pbn_reach_destroy(pbn_reach* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    delete r;
}

int pbn_reach_get_info(const pbn_reach* r, pbn_reach_info* info) {
    CHECK_NN(r, "reach");
    CHECK_NN(info, "info");
    info->n_nodes = r->net->N;
    info->n_words = r->W;
    info->device = r->device;
    info->complete = r->complete ? 1 : 0;
    info->max_states = r->max_states;
    info->table_slots = r->tcap;
    info->key_capacity = r->key_cap;
    info->n_states = r->count;
    info->n_entries = r->n_keys;
    info->kind = r->net->kind;
    info->table_graph = r->graph;
    return 0;
}

int pbn_reach_unstable(pbn_reach* r, const uint64_t* states, uint64_t n_states, uint64_t* masks) {
    CHECK_NN(r, "reach");
    CHECK_NN(states, "states");
    CHECK_NN(masks, "masks");
    if (n_states < 1 || n_states > (1ull << 28)) return fail(PBN_E_INVALID, "n_states outside [1, 2^28]");
    SET_DEV(r);
    const size_t bytes = 8 * (size_t)r->W * n_states;
    if (int rc = r->upload(states, n_states)) return rc;
    if (int rc = r->out.ensure(bytes)) return rc;
    ReachArgs a = r->args();
    a.in = (const uint64_t*)r->in.p;
    a.out = (uint64_t*)r->out.p;
    a.n_in = n_states;
    const int grid = (int)std::min<uint64_t>(REACH_MAX_GRID, (n_states + 3) / 4);
    if (int e = launch_reach(r->W, REACH_K_UNSTABLE, a, grid, r->stream))
        return fail(PBN_E_HIP, "k_unstable launch: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(hipMemcpyAsync(masks, r->out.p, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return 0;
}

int pbn_reach_closure(pbn_reach* r, const uint64_t* seeds, uint64_t n_seeds, uint64_t* count, int32_t* complete) {
    CHECK_NN(r, "reach");
    CHECK_NN(seeds, "seeds");
    if (n_seeds < 1 || n_seeds > (1ull << 28)) return fail(PBN_E_INVALID, "n_seeds outside [1, 2^28]");
    const uint64_t top = r->net->N % 64 ? ~0ull << (r->net->N % 64) : 0;
    for (uint64_t e = 0; e < n_seeds; e++)
        if (seeds[e * r->W + r->W - 1] & top) return fail(PBN_E_RANGE, "seed %llu has bits set past node %d",
                                                          (unsigned long long)e, r->net->N - 1);
    SET_DEV(r);
    r->n_keys = r->count = r->epoch = r->free_limit = 0;
    r->free_any = false;
    r->complete = false;
    HIP_TRY(hipMemsetAsync(r->table.p, 0, 8 * (size_t)r->tcap, r->stream));
    HIP_TRY(hipMemsetAsync(r->ctl.p, 0, 4 * REACH_CTL_WORDS, r->stream));
    if (int rc = r->upload(seeds, n_seeds)) return rc;
    ReachArgs a = r->args();
    a.in = (const uint64_t*)r->in.p;
    a.n_in = n_seeds;
    if (int e = launch_reach(r->W, REACH_K_SEED, a, (int)((n_seeds + BLOCK - 1) / BLOCK), r->stream))
        return fail(PBN_E_HIP, "k_reach_seed launch: %s", hipGetErrorString((hipError_t)e));
    // level-synchronous: the entries a level publishes are the next frontier; the fixed point is an empty one
    uint32_t lo = 0;
    for (;;) {
        if (int rc = r->read_ctl()) return rc;
        const uint32_t hi = std::min(r->h_ctl[REACH_QTAIL], r->key_cap);
        r->n_keys = std::min(r->h_ctl[REACH_KEYS], r->key_cap);
        r->count = r->h_ctl[REACH_COUNT];
        if (r->h_ctl[REACH_OVERFLOW] || lo >= hi) break;
        // free ring: takers that ran past the last level's limit took nothing; what the last level pushed is
        // complete now and may be taken
        if ((int32_t)(r->h_ctl[REACH_FREE_HEAD] - r->free_limit) > 0) {
            r->h_ctl[REACH_CTL_WORDS] = r->free_limit;
            HIP_TRY(hipMemcpyAsync((uint32_t*)r->ctl.p + REACH_FREE_HEAD, r->h_ctl + REACH_CTL_WORDS, 4,
                                   hipMemcpyHostToDevice, r->stream));
            r->h_ctl[REACH_FREE_HEAD] = r->free_limit;
        }
        r->free_limit = r->h_ctl[REACH_FREE_TAIL];
        r->free_any = r->free_limit != r->h_ctl[REACH_FREE_HEAD];
        if (int rc = r->sweep(REACH_K_EXPAND, lo, hi)) return rc;
        lo = hi;
    }
    // lanes that passed the count test together can publish past max_states: that is over capacity too
    r->complete = r->h_ctl[REACH_OVERFLOW] == 0 && r->count <= r->max_states;
    if (count) *count = r->count;
    if (complete) *complete = r->complete ? 1 : 0;
    return 0;
}

int pbn_reach_mark_backward(pbn_reach* r, const uint64_t* state, uint64_t* n_marked) {
    CHECK_NN(r, "reach");
    CHECK_NN(state, "state");
    if (!r->count) return fail(PBN_E_STATE, "the set is empty: call pbn_reach_closure first");
    if (r->epoch >= REACH_DEAD - 1u) return fail(PBN_E_STATE, "mark epochs exhausted: run the closure again");
    SET_DEV(r);
    r->epoch++;
    HIP_TRY(hipMemsetAsync((uint32_t*)r->ctl.p + REACH_QTAIL, 0, 8, r->stream));  // QTAIL and MISSING
    if (int rc = r->upload(state, 1)) return rc;
    ReachArgs a = r->args();
    a.in = (const uint64_t*)r->in.p;
    a.n_in = 1;
    if (int e = launch_reach(r->W, REACH_K_BACK_START, a, 1, r->stream))
        return fail(PBN_E_HIP, "k_reach_back_start launch: %s", hipGetErrorString((hipError_t)e));
    uint32_t lo = 0;
    for (;;) {
        if (int rc = r->read_ctl()) return rc;
        if (r->h_ctl[REACH_MISSING]) {
            r->epoch--;
            return fail(PBN_E_INVALID, "the state is not in the set");
        }
        const uint32_t hi = std::min(r->h_ctl[REACH_QTAIL], r->key_cap);
        if (lo >= hi) break;
        if (int rc = r->sweep(REACH_K_BACK, lo, hi)) return rc;
        lo = hi;
    }
    if (n_marked) *n_marked = lo;
    return 0;
}

int pbn_reach_read(pbn_reach* r, uint64_t* states, uint32_t* marks, uint64_t capacity, uint64_t* n_states) {
    CHECK_NN(r, "reach");
    CHECK_NN(n_states, "n_states");
    *n_states = r->count;
    if (!states && !marks) return 0;
    if (capacity < r->count)
        return fail(PBN_E_INVALID, "capacity %llu below the %u states of the set", (unsigned long long)capacity, r->count);
    SET_DEV(r);
    const size_t W = (size_t)r->W;
    std::vector<uint64_t> k((size_t)r->n_keys * W);
    std::vector<uint32_t> m(r->n_keys);
    if (r->n_keys) {
        HIP_TRY(hipMemcpyAsync(k.data(), r->keys.p, 8 * k.size(), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipMemcpyAsync(m.data(), r->mark.p, 4 * m.size(), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    uint64_t n = 0;
    for (uint32_t e = 0; e < r->n_keys; e++) {
        if (m[e] == REACH_DEAD) continue;
        if (n >= capacity) return fail(PBN_E_HIP, "the set holds more live entries than it counted");
        if (states) memcpy(states + n * W, k.data() + (size_t)e * W, 8 * W);
        if (marks) marks[n] = r->epoch && m[e] == r->epoch ? 1u : 0u;
        n++;
    }
    *n_states = n;
    return 0;
}

int pbn_reach_hull(pbn_reach* r, uint64_t* all_words, uint64_t* any_words) {
    CHECK_NN(r, "reach");
    CHECK_NN(all_words, "all_words");
    CHECK_NN(any_words, "any_words");
    if (!r->count) return fail(PBN_E_STATE, "the set is empty: call pbn_reach_closure first");
    SET_DEV(r);
    const size_t wb = 8 * (size_t)r->W;
    HIP_TRY(hipMemsetAsync(r->hull.p, 0xFF, wb, r->stream));
    HIP_TRY(hipMemsetAsync((uint8_t*)r->hull.p + wb, 0, wb, r->stream));
    ReachArgs a = r->args();
    a.hi = r->n_keys;
    const int grid = (int)std::min<uint32_t>(1024u, (r->n_keys + BLOCK - 1) / BLOCK);
    if (int e = launch_reach(r->W, REACH_K_HULL, a, grid, r->stream))
        return fail(PBN_E_HIP, "k_reach_hull launch: %s", hipGetErrorString((hipError_t)e));
    uint64_t h[2 * MAX_WORDS];
    HIP_TRY(hipMemcpyAsync(h, r->hull.p, 2 * wb, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    memcpy(all_words, h, wb);
    memcpy(any_words, h + r->W, wb);
    return 0;
}

}  // extern "C"
