// pbn_abi_census.cpp -- the state census (pbn_census_*): the entry points over the counting table of pbn_census.hpp and
// the kernel of pbn_census.hip. DESIGN.md §15.
#include "pbn_host.hpp"
#include "pbn_census.hpp"

static_assert(PBN_CENSUS_MAX_STATES == CENSUS_MAX_STATES && PBN_CENSUS_MAX_UPDATES == CENSUS_MAX_UPDATES,
              "pbn_abi.h and pbn_census.hpp name the same caps");

// The table of one census. Host-only (device -1): the shape and the argument checks, no device memory.
struct pbn_census {
    int n_nodes = 0, W = 0, device = -1;
    uint64_t max_states = 0;
    uint32_t slots = 0, key_cap = 0, ring_cap = 0;
    uint64_t visits = 0;    // sample points of every launch so far: known on the host, no device counter
    uint32_t launches = 0;  // the next launch's ring parity is launches & 1
    DevBuf table, keys, counts, ring, ctl;
    hipEvent_t done = nullptr;  // the end of the last launch, on whatever stream it went to
    bool pending = false;       // a launch since the last wait
    // k_census' resident workgroups per CU, asked once per kernel and image size (a census does not own the network)
    int bpc = 0;
    const void* bpc_kernel = nullptr;
    uint32_t bpc_image = 0;

    ~pbn_census() {
        if (done) (void)hipEventDestroy(done);
    }
    int wait() {
        if (pending) HIP_TRY(hipEventSynchronize(done));
        pending = false;
        return 0;
    }
    uint64_t mask_top() const { return n_nodes % 64 ? (1ull << (n_nodes % 64)) - 1ull : ~0ull; }
};

extern "C" {

int pbn_census_create(int32_t n_nodes, int device, uint64_t max_states, pbn_census** out) {
    CHECK_NN(out, "out");
    *out = nullptr;
    if (n_nodes < 1 || n_nodes > 64 * MAX_WORDS)
        return fail(PBN_E_INVALID, "n_nodes=%d outside [1, %d]", (int)n_nodes, 64 * MAX_WORDS);
    if (max_states < 1 || max_states > PBN_CENSUS_MAX_STATES)
        return fail(PBN_E_INVALID, "max_states=%llu outside [1, PBN_CENSUS_MAX_STATES = %llu]",
                    (unsigned long long)max_states, (unsigned long long)PBN_CENSUS_MAX_STATES);
    if (device < -1) return fail(PBN_E_RANGE, "device %d: a device index, or -1 for a host-only handle", device);
    if (device >= 0)
        if (int rc = open_device(device)) return rc;
    pbn_census* c = new pbn_census;
    c->n_nodes = n_nodes;
    c->W = (n_nodes + 63) / 64;
    c->max_states = max_states;
    c->slots = census_slots(max_states);
    c->key_cap = census_key_cap(max_states);
    c->ring_cap = census_ring_cap(c->key_cap);
    if (device >= 0) {
        c->device = device;
        auto bail = [&](int code) {
            pbn_census_destroy(c);
            return code;
        };
        int rc = 0;
        if ((rc = c->table.ensure(8 * (size_t)c->slots)) || (rc = c->keys.ensure(8 * (size_t)c->W * c->key_cap)) ||
            (rc = c->counts.ensure(8 * (size_t)c->key_cap)) || (rc = c->ring.ensure(4 * 2 * (size_t)c->ring_cap)) ||
            (rc = c->ctl.ensure(CENSUS_CTL_BYTES)))
            return bail(rc);
        if (hipEventCreateWithFlags(&c->done, hipEventDisableTiming) != hipSuccess)
            return bail(fail(PBN_E_HIP, "hipEventCreate"));
        if (int rc2 = pbn_census_clear(c)) return bail(rc2);
    }
    *out = c;
    return 0;
}

void pbn_census_destroy(pbn_census* c) {
    if (!c) return;
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        if (c->pending) (void)hipEventSynchronize(c->done);
    }
    delete c;  // the DevBufs give back the table
}

int pbn_census_clear(pbn_census* c) {
    CHECK_NN(c, "census");
    c->visits = 0;
    c->launches = 0;
    if (c->device < 0) return 0;
    SET_DEV(c);
    if (int rc = c->wait()) return rc;
    // the key words need no clearing: an entry's words are written before a slot names it. The rings are empty
    // once their heads and tails are 0.
    HIP_TRY(hipMemset(c->table.p, 0, 8 * (size_t)c->slots));
    HIP_TRY(hipMemset(c->counts.p, 0, 8 * (size_t)c->key_cap));
    HIP_TRY(hipMemset(c->ctl.p, 0, CENSUS_CTL_BYTES));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

// The control block as the host reads it: the u32 words, then dropped and adds.
struct CensusCtl {
    uint32_t w[CENSUS_CTL_WORDS];
    uint64_t dropped, adds;
};
static_assert(sizeof(CensusCtl) == CENSUS_CTL_BYTES, "the control block's layout");

static int read_ctl(pbn_census* c, CensusCtl* h) {
    memset(h, 0, sizeof *h);
    if (c->device < 0) return 0;
    SET_DEV(c);
    if (int rc = c->wait()) return rc;
    HIP_TRY(hipMemcpy(h, c->ctl.p, CENSUS_CTL_BYTES, hipMemcpyDeviceToHost));
    return 0;
}

// The read-out: the reported entries compacted into states / counts (either may be NULL, at most cap rows), their
// number, and the visits dropped in all -- on the device, plus those counted on entries published past max_states.
// The entry arrays are copied only when somebody needs them: for rows, or for the visits of entries past max_states.
static int read_out(pbn_census* c, uint64_t* states, uint64_t* counts, uint64_t cap, uint64_t* n_states,
                    uint64_t* dropped) {
    CensusCtl h;
    if (int rc = read_ctl(c, &h)) return rc;
    const uint64_t live = h.w[CENSUS_COUNT];
    *n_states = std::min<uint64_t>(live, c->max_states);
    *dropped = h.dropped;
    const uint64_t n_entries = std::min<uint64_t>(h.w[CENSUS_KEYS], c->key_cap);
    if (!n_entries || (!states && !counts && live <= c->max_states)) return 0;
    std::vector<uint64_t> k, n((size_t)n_entries);
    if (states) {
        k.resize((size_t)n_entries * c->W);
        HIP_TRY(hipMemcpy(k.data(), c->keys.p, 8 * k.size(), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(n.data(), c->counts.p, 8 * n.size(), hipMemcpyDeviceToHost));
    uint64_t over = 0;
    const uint64_t rows = census_compact(k.data(), n.data(), n_entries, c->W, states, counts, cap, &over);
    if (rows != *n_states)
        return fail(PBN_E_HIP, "the census holds %llu counted entries within max_states and %llu published ones",
                    (unsigned long long)rows, (unsigned long long)*n_states);
    *dropped += over;
    return 0;
}

int pbn_census_get_info(pbn_census* c, pbn_census_info* info) {
    CHECK_NN(c, "census");
    CHECK_NN(info, "info");
    uint64_t n_states = 0, dropped = 0;
    if (int rc = read_out(c, nullptr, nullptr, 0, &n_states, &dropped)) return rc;
    info->n_nodes = c->n_nodes;
    info->n_words = c->W;
    info->device = c->device;
    info->max_states = c->max_states;
    info->table_slots = c->slots;
    info->n_states = n_states;
    info->visits = c->visits;
    info->dropped = dropped;
    return 0;
}

int pbn_census_get_stats(pbn_census* c, uint64_t* adds, uint64_t* entries) {
    CHECK_NN(c, "census");
    if (!adds && !entries) return fail(PBN_E_INVALID, "adds and entries are both NULL");
    CensusCtl h;
    if (int rc = read_ctl(c, &h)) return rc;
    if (adds) *adds = h.adds;
    if (entries) *entries = std::min<uint64_t>(h.w[CENSUS_KEYS], c->key_cap);
    return 0;
}

int pbn_census_run_device(pbn_batch* b, pbn_census* c, uint32_t n_updates, uint32_t first, uint32_t stride,
                          const uint64_t* mask_words) {
    CHECK_NN(c, "census");
    // what the census alone decides comes first, so that it is decided the same way with and without a device
    if (n_updates > PBN_CENSUS_MAX_UPDATES)
        return fail(PBN_E_INVALID, "n_updates=%u outside [0, PBN_CENSUS_MAX_UPDATES = %u]", (unsigned)n_updates,
                    (unsigned)PBN_CENSUS_MAX_UPDATES);
    if (stride == 0) return fail(PBN_E_INVALID, "stride is 0: the sample points are first, first + stride, ...");
    if (first > n_updates)
        return fail(PBN_E_INVALID, "first=%u above n_updates=%u: no sample point", (unsigned)first, (unsigned)n_updates);
    if (mask_words && (mask_words[c->W - 1] & ~c->mask_top()))
        return fail(PBN_E_INVALID, "the mask has bits set past node %d", c->n_nodes - 1);
    if (c->device < 0) return fail(PBN_E_STATE, "the census is a host-only handle (created with device -1)");
    CHECK_NN(b, "batch");
    if (c->device != b->device)
        return fail(PBN_E_INVALID, "the census lives on device %d, the batch on device %d", c->device, b->device);
    if (c->n_nodes != b->N)
        return fail(PBN_E_INVALID, "the census counts states of %d nodes, the batch has %d", c->n_nodes, b->N);
    if (b->net->kind == PBN_KIND_PROB_TABLE && n_updates)
        if (int rc = check_two_nodes(b)) return rc;
    SET_DEV(b);
    void* kernel = census_kernel(b->W, b->net->kind);
    if (c->bpc_kernel != kernel || c->bpc_image != b->net->L.bytes) {
        c->bpc = 0;
        c->bpc_kernel = kernel;
        c->bpc_image = b->net->L.bytes;
    }
    if (int rc = cached_bpc(c->bpc, kernel, b->W, b->net->L.bytes)) return rc;
    CensusArgs a{};
    fill_lane_env(b, a);
    a.update = b->update_count;
    a.n_updates = n_updates;
    a.first = first;
    a.stride = stride;
    a.parity = c->launches & 1u;
    for (int k = 0; k < c->W; ++k) a.mask[k] = mask_words ? mask_words[k] : ~0ull;
    a.table = (unsigned long long*)c->table.p;
    a.keys = (uint64_t*)c->keys.p;
    a.counts = (unsigned long long*)c->counts.p;
    a.ring = (uint32_t*)c->ring.p;
    a.ctl = (uint32_t*)c->ctl.p;
    a.dropped = (unsigned long long*)((uint8_t*)c->ctl.p + 4 * CENSUS_CTL_WORDS);
    a.adds = a.dropped + 1;
    a.tmask = c->slots - 1u;
    a.key_cap = c->key_cap;
    a.max_states = (uint32_t)c->max_states;
    a.ring_mask = c->ring_cap - 1u;
    // what is resident, and no more lanes than the table has entries to spare (one dead entry per lane at most).
    // PBNSIM_ENVSET_GRID caps it further, as it caps every lane-per-env step launch (Knobs::envset_grid: k_tenv_step,
    // k_tenv_macro, k_env_set, k_census): tests make a small batch walk the grid-stride loop with it
    int grid = std::min(b->grid_for(b->B, c->bpc), CENSUS_MAX_GRID);
    if (b->knob.envset_grid > 0) grid = std::min(grid, b->knob.envset_grid);
    if (int rc = timed_launch(b, "k_census", [&] { return launch_lane_env(kernel, b->W, a.L.bytes, grid, b->stream, &a); }))
        return rc;
    HIP_TRY(hipEventRecord(c->done, b->stream));
    c->pending = true;
    c->launches++;
    c->visits += b->B * census_samples(n_updates, first, stride);
    b->update_count += n_updates;
    return 0;
}

int pbn_census_read(pbn_census* c, uint64_t* states, uint64_t* counts, uint64_t cap, uint64_t* n_states) {
    CHECK_NN(c, "census");
    CHECK_NN(n_states, "n_states");
    CensusCtl h;
    if (int rc = read_ctl(c, &h)) return rc;
    *n_states = std::min<uint64_t>(h.w[CENSUS_COUNT], c->max_states);
    if (!states && !counts) return 0;
    if (cap < *n_states)
        return fail(PBN_E_INVALID, "capacity %llu below the %llu states of the census", (unsigned long long)cap,
                    (unsigned long long)*n_states);
    uint64_t dropped = 0;
    return read_out(c, states, counts, cap, n_states, &dropped);
}

}  // extern "C"
