// pbn_abi.cpp -- host side of libpbnsim.so: the core of the C ABI declared in include/pbn_abi.h.
//
// Owns device memory and validates descriptors: version / error / device count, the lifecycle of
// networks, batches and env configs, stream / info / sync, state I/O and timing. The packers live in
// pbn_image.cpp, the calls that advance a batch in pbn_abi_sim.cpp, R6 in pbn_abi_env.cpp, attractor
// discovery in pbn_abi_reach.cpp (shared objects and helpers: pbn_host.hpp).
// There is no host compute path: every state transition runs on the GPU, and a
// missing/unsupported device is reported as an error, never silently emulated.
#include "pbn_host.hpp"

#include <cstdlib>

const void* DevCache::on(int device, const void* host, size_t bytes) {
    std::lock_guard<std::mutex> g(mu);
    auto it = dev.find(device);
    if (it != dev.end()) return it->second;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    if (hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    dev[device] = p;
    return p;
}

void DevCache::release() {
    for (auto& kv : dev) {
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second);
    }
    dev.clear();
}

// The PBNSIM_* launch knobs (measurement / tests), read once per batch.
static Knobs read_knobs() {
    Knobs k;
    if (const char* sm = getenv("PBNSIM_STORE_MODE")) k.store_mode = std::max(0, std::min(2, atoi(sm)));
    if (const char* r = getenv("PBNSIM_ENVS_PER_THREAD")) k.envs_per_thread = std::max(1, std::min(64, atoi(r)));
    if (const char* v = getenv("PBNSIM_STEP_BLOCK")) k.step_block = atoi(v) == 256 ? 256 : 1024;
    k.env.no_gen = getenv("PBNSIM_ENV_NO_GEN") != nullptr;
    if (const char* v = getenv("PBNSIM_ENV_GROUP")) k.env.group = std::max(1, atoi(v));
    if (const char* v = getenv("PBNSIM_ENV_BPC")) k.env.bpc = std::max(1, atoi(v));
    if (const char* v = getenv("PBNSIM_ENV_CHUNK")) k.env.chunk = atoi(v);
    if (const char* v = getenv("PBNSIM_ENV_GRID")) k.env.grid_cap = std::max(1, atoi(v));
    if (const char* v = getenv("PBNSIM_ENV_TAIL")) k.env.tail = std::max(0, std::min(64, atoi(v)));
    if (const char* v = getenv("PBNSIM_ENV_LANES")) k.env.lane_limit = std::max(0, std::min(64, atoi(v)));
    if (const char* v = getenv("PBNSIM_ENV_STEAL")) k.env.steal = atoi(v) != 0;
    if (const char* v = getenv("PBNSIM_ENV_KERNEL_IMAGE")) k.env.kernel_image = atoi(v) != 0;
    if (const char* v = getenv("PBNSIM_ENV_HELPERS")) k.env_helpers = std::max(0, std::min(3, atoi(v)));
    if (const char* v = getenv("PBNSIM_ENV_GRID_STEAL")) k.env_grid_steal = atoi(v) != 0 ? 1 : 0;
#ifdef PBN_MEASURE_KNOBS  // A/B-only knobs: tools/build_exp.sh -DPBN_MEASURE_KNOBS
    if (const char* v = getenv("PBNSIM_ENV_POOL_CU_IDLE")) k.env_pool_cu_idle = atoi(v) != 0 ? 1 : 0;
    if (const char* v = getenv("PBNSIM_ENV_GRID_SLOTS")) k.env_grid_slots = std::max(1, std::min((int)GPOOL_CAP, atoi(v)));
#endif
    if (const char* v = getenv("PBNSIM_SSD_WAVE")) k.ssd_wave = atoi(v) ? 1 : 0;
    if (const char* v = getenv("PBNSIM_SSD_SERIAL")) k.ssd_serial = atoi(v) != 0;
    if (const char* v = getenv("PBNSIM_SSD_SHARED")) {
        const int w = atoi(v);
        k.ssd_shared = w == 0 ? 0 : (w == 4 || w == 8) ? w : 1;
    }
    if (const char* v = getenv("PBNSIM_STEP_GRAPH")) k.step_graph = atoi(v) != 0 ? 1 : 0;
    if (const char* v = getenv("PBNSIM_STEP_CHAINS")) {
        const int s = atoi(v);
        k.step_chains = s >= 4 ? 4 : s >= 2 ? 2 : 1;
    }
    if (const char* v = getenv("PBNSIM_MT_LANES")) k.mt_lane_walk = atoi(v) != 0;
    if (const char* v = getenv("PBNSIM_ROLL_GROUP")) k.roll_group = std::max(0, atoi(v));
    if (const char* v = getenv("PBNSIM_ENVSET_GRID")) k.envset_grid = std::max(1, atoi(v));
    if (const char* v = getenv("PBNSIM_ENVSET_NO_HULL")) k.envset_no_hull = atoi(v) != 0;
    if (const char* v = getenv("PBNSIM_ENVSET_NO_SKIP")) k.envset_no_skip = atoi(v) != 0;
    return k;
}

// k_rollout_grp: predictor mix, N <= 256 (byte-packed node lists of a group)
static bool roll_group_ok(const pbn_net* net) { return net->kind == PBN_KIND_PREDICTOR_MIX && net->N <= 256; }

// Lanes per env of the rollout kernel by batch size: the largest G with B x G <= 512 lanes per CU
// (8 waves per CU). Measured on MI355X (tools/rollout_group_sweep.py, node-updates/s): Bittner-28
// 65,536 envs 114 G (lane) -> 145 G (G = 2); 16,384 envs 31 -> 74 G (G = 8); Bittner-200
// 65,536 envs 164 -> 183 G (G = 2); from 131,072 envs on lane mode is as fast or faster (the
// group kernel spends ~1.1x (G = 2) to ~2x (G = 4, 8) the VALU work per update).
static int roll_group_size(const pbn_batch* b, const pbn_net* net) {
    if (!roll_group_ok(net)) return 1;
    const uint64_t lanes = (uint64_t)b->n_cu * 512u;
    for (int g = 8; g >= 2; g /= 2)
        if (b->B * (uint64_t)g <= lanes) return g;
    return 1;
}

static int check_state_words(const pbn_batch* b, const uint64_t* w) {
    const int r = b->N & 63;
    if (!r) return 0;
    const uint64_t bad = ~(((uint64_t)1 << r) - 1);
    for (uint64_t e = 0; e < b->B; e++)
        if (w[e * b->W + b->W - 1] & bad) return fail(PBN_E_RANGE, "env %llu has bits set beyond node %d",
                                                       (unsigned long long)e, b->N - 1);
    return 0;
}

// host -> device through the pinned staging buffer when small (the caller syncs before reuse)
int h2d(pbn_batch* b, void* dst, const void* src, size_t bytes) {
    if (bytes <= PinBuf::CAP && b->pin.ready()) {
        HIP_TRY(hipStreamSynchronize(b->stream));  // the staging buffer may still feed an earlier copy
        memcpy(b->pin.p, src, bytes);
        HIP_TRY(hipMemcpyAsync(dst, b->pin.p, bytes, hipMemcpyHostToDevice, b->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->stream));
    }
    return 0;
}

int run_init(pbn_batch* b, const pbn_envcfg* cfg, const void* d_mask, const void* care, const void* value) {
    InitArgs a{};
    a.state = b->d_state;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.reset_count = b->reset_count;
    a.n_nodes = b->N;
    a.kind = b->net->kind;
    a.cube_care = (const uint64_t*)care;
    a.cube_value = (const uint64_t*)value;
    a.n_cubes = cfg ? cfg->H_reset : 0;
    a.mask = (const uint8_t*)d_mask;
    a.n_steps = cfg ? b->d_nsteps : nullptr;
    if (int rc = timed_launch(b, "k_init", [&] { return launch_init(b->W, a, b->grid_all(b->B), b->stream); })) return rc;
    b->reset_count++;
    return 0;
}

int validate_actions(const pbn_batch* b, const int32_t* actions, int A, int offset) {
    if (int rc = check_action_shape(A, offset)) return rc;
    const uint64_t n = b->B * (uint64_t)A;
    for (uint64_t k = 0; k < n; k++) {
        int32_t v = actions[k];
        if (v == 0) continue;
        int32_t idx = v - offset;
        if (idx >= b->N || idx < -b->N)
            return fail(PBN_E_RANGE, "Invalid action, no node at index %d (env %llu)", idx,
                        (unsigned long long)(k / A));  // base.py:283-284
    }
    return 0;
}

// Region timing: the stop event is recorded on the stream now, right behind the last launch.
static int close_region(pbn_batch* b) {
    b->tm.region_end = nullptr;
    if (!b->tm.region_launches) return 0;
    if (b->tm.ev_pool.empty()) return fail(PBN_E_HIP, "timing region without events");
    HIP_TRY(hipEventRecord(b->tm.ev_pool[0].second, b->stream));
    b->tm.region_end = b->tm.ev_pool[0].second;
    return 0;
}

extern "C" {

int pbn_abi_version(void) { return PBN_ABI_VERSION; }

const char* pbn_last_error(void) { return g_err.c_str(); }

int pbn_device_count(int* count) {
    CHECK_NN(count, "count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(PBN_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return 0;
}

int pbn_net_create(const pbn_net_desc* d, pbn_net** out) {
    CHECK_NN(d, "desc");
    CHECK_NN(out, "out");
    *out = nullptr;
    if (d->n_nodes < 1 || d->n_nodes > 64 * MAX_WORDS)
        return fail(PBN_E_UNSUPPORTED, "n_nodes=%d outside [1, %d]", d->n_nodes, 64 * MAX_WORDS);
    pbn_net* n = new pbn_net;
    n->kind = d->kind;
    n->N = d->n_nodes;
    n->W = (d->n_nodes + 63) / 64;
    int rc;
    if (d->kind == PBN_KIND_PREDICTOR_MIX)
        rc = build_predictor_image(d, n);
    else if (d->kind == PBN_KIND_PROB_TABLE)
        rc = build_table_image(d, n);
    else
        rc = fail(PBN_E_INVALID, "unknown network kind %d", d->kind);
    if (rc) {
        delete n;
        return rc;
    }
    *out = n;
    return 0;
}

int pbn_net_select_u32(const pbn_net* n, int32_t node, uint32_t a, uint64_t* record) {
    CHECK_NN(n, "net");
    CHECK_NN(record, "record");
    if (n->L.kind != KIND_PREDICTOR_MIX) return fail(PBN_E_INVALID, "not a predictor-mix network");
    if (node < 0 || node >= n->L.n_nodes) return fail(PBN_E_RANGE, "node %d out of range", node);
    *record = net_select_u32(n, node, a);
    return 0;
}

int pbn_net_unstable(const pbn_net* n, int32_t graph, const uint64_t* states, uint64_t n_states, uint64_t* masks) {
    CHECK_NN(n, "net");
    CHECK_NN(states, "states");
    CHECK_NN(masks, "masks");
    if (n->L.kind == KIND_PROB_TABLE && graph != PBN_TABLE_GRAPH_STG && graph != PBN_TABLE_GRAPH_STEP)
        return fail(PBN_E_INVALID, "graph=%d is neither PBN_TABLE_GRAPH_STG nor PBN_TABLE_GRAPH_STEP", (int)graph);
    if (n_states < 1 || n_states > (1ull << 28)) return fail(PBN_E_INVALID, "n_states outside [1, 2^28]");
    net_unstable(n, graph, states, n_states, masks);
    return 0;
}

int pbn_net_edge_mass(const pbn_net* n, int32_t graph, const uint64_t* states, uint64_t n_states, uint64_t* mass) {
    CHECK_NN(n, "net");
    CHECK_NN(states, "states");
    CHECK_NN(mass, "mass");
    if (n->L.kind == KIND_PROB_TABLE && graph != PBN_TABLE_GRAPH_STG && graph != PBN_TABLE_GRAPH_STEP)
        return fail(PBN_E_INVALID, "graph=%d is neither PBN_TABLE_GRAPH_STG nor PBN_TABLE_GRAPH_STEP", (int)graph);
    if (n_states < 1 || n_states > (1ull << 28)) return fail(PBN_E_INVALID, "n_states outside [1, 2^28]");
    net_edge_mass(n, graph, states, n_states, mass);
    return 0;
}

void pbn_net_destroy(pbn_net* n) {
    if (!n) return;
    n->dev_image.release();
    delete n;
}

int pbn_batch_create(const pbn_net* net_c, int device, uint64_t n_envs, uint64_t env_id_base, uint64_t seed,
                     pbn_batch** out) {
    CHECK_NN(net_c, "net");
    CHECK_NN(out, "out");
    *out = nullptr;
    pbn_net* net = const_cast<pbn_net*>(net_c);
    if (n_envs < 1) return fail(PBN_E_INVALID, "n_envs must be >= 1");
    // without the sum: env_id_base + n_envs wraps for bases near 2^64
    const uint64_t id_end = (uint64_t)1 << 56;
    if (n_envs > id_end || env_id_base > id_end - n_envs) return fail(PBN_E_RANGE, "global env ids must stay below 2^56");
    if (int rc = open_device(device)) return rc;
    pbn_batch* b = new pbn_batch;
    b->net = net;
    b->device = device;
    b->W = net->W;
    b->N = net->N;
    b->B = n_envs;
    b->env_base = env_id_base;
    b->seed = seed;
    b->knob = read_knobs();
    hipDeviceProp_t prop;
    int rc = 0;
    auto bail = [&](int code) {
        pbn_batch_destroy(b);
        return code;
    };
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(fail(PBN_E_HIP, "hipGetDeviceProperties"));
    b->n_cu = prop.multiProcessorCount;
    b->step = step_shape(n_envs, b->W, b->n_cu, b->knob.step_block, b->knob.step_chains, b->knob.step_graph,
                         b->knob.envs_per_thread);
    // rollout lanes per env: 1 = k_rollout; 2/4/8 = k_rollout_grp (predictor mix, N <= 256)
    b->roll_group = roll_group_size(b, net);
    if (b->knob.roll_group >= 0) {
        const int g = b->knob.roll_group;
        b->roll_group = (g == 2 || g == 4 || g == 8) && roll_group_ok(net) ? g : 1;
    }
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(PBN_E_HIP, "hipStreamCreate"));
    b->own_stream = b->stream;
    if (b->step.chains > 1) {  // the chains' streams right behind the batch's own
        for (int c = 1; c < b->step.chains; ++c)
            if (hipStreamCreateWithFlags(&b->ch.stream[c], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&b->ch.done[c], hipEventDisableTiming) != hipSuccess)
                return bail(fail(PBN_E_HIP, "step chain %d: stream / event create", c));
        if (hipEventCreateWithFlags(&b->ch.fork, hipEventDisableTiming) != hipSuccess)
            return bail(fail(PBN_E_HIP, "step chains: event create"));
    }
    size_t sb = 8 * (size_t)b->W * n_envs;
    if (hipMalloc(&b->d_state, sb) != hipSuccess) return bail(fail(PBN_E_NOMEM, "state alloc (%zu B)", sb));
    if (hipMalloc(&b->d_nsteps, 8 * n_envs) != hipSuccess) return bail(fail(PBN_E_NOMEM, "n_steps alloc"));
    // [0] the launch's error flags (zeroed per launch), [1] sticky grid-pool faults of device-path env
    // launches, read and cleared by pbn_sync
    if (hipMalloc(&b->d_error, 8) != hipSuccess) return bail(fail(PBN_E_NOMEM, "error flag alloc"));
    if (hipMemsetAsync(b->d_error, 0, 8, b->stream) != hipSuccess || hipMemsetAsync(b->d_state, 0, sb, b->stream) != hipSuccess ||
        hipMemsetAsync(b->d_nsteps, 0, 8 * n_envs, b->stream) != hipSuccess)
        return bail(fail(PBN_E_HIP, "hipMemset"));
    b->d_image = net->image_on(device);
    if (!b->d_image) return bail(fail(PBN_E_NOMEM, "network image upload failed"));
    if ((rc = max_blocks_step(b->W, net->kind, net->L.bytes, BLOCK, &b->bpc_base)))
        return bail(fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)rc)));
    if ((rc = max_blocks_step(b->W, net->kind, net->L.plane_off, b->step.block, &b->bpc_step)))
        return bail(fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)rc)));
    if ((rc = max_blocks_step(b->W, net->kind, net->L.plane_off, BLOCK, &b->bpc_roll, 1, b->roll_group)))
        return bail(fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)rc)));
    if (hipStreamSynchronize(b->stream) != hipSuccess) return bail(fail(PBN_E_HIP, "stream sync"));
    *out = b;
    return 0;
}
void pbn_batch_destroy(pbn_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (hipStream_t s : b->ch.stream)
        if (s) (void)hipStreamSynchronize(s);
    delete b;  // every member gives back what it holds (pbn_host.hpp)
}

int pbn_batch_set_stream(pbn_batch* b, int own, void* stream) {
    CHECK_NN(b, "batch");
    hipStream_t s = own ? b->own_stream : (hipStream_t)stream;  // NULL = the default stream
    if (s == b->stream) return 0;
    SET_DEV(b);
    HIP_TRY(hipStreamSynchronize(b->stream));  // work already queued on the old stream finishes first
    b->stream = s;
    return 0;
}

int pbn_batch_get_info(const pbn_batch* b, pbn_batch_info* info) {
    CHECK_NN(b, "batch");
    CHECK_NN(info, "info");
    info->n_nodes = b->N;
    info->n_words = b->W;
    info->kind = b->net->kind;
    info->device = b->device;
    info->n_envs = b->B;
    info->env_id_base = b->env_base;
    info->seed = b->seed;
    info->update_count = b->update_count;
    info->env_call_count = b->r6.calls;
    info->reset_count = b->reset_count;
    info->mt_ready = b->mt.ready;
    const EnvPlan& p = b->r6.last;
    info->env_lanes = p.grp;
    info->roll_lanes = b->roll_group;
    info->env_grid = p.grid;
    info->env_kernel = p.mode;
    info->env_lane_limit = (int)p.lane_limit;
    info->env_handoff = p.handoff ? 1 : 0;
    info->env_chunk = (p.mode == ENV_MODE_COOP || p.mode == ENV_MODE_TAIL) ? (int)p.chunk : 0;
    info->step_chains = b->step.chains;
    return 0;
}

int pbn_batch_get_counters(const pbn_batch* b, pbn_batch_counters* out) {
    CHECK_NN(b, "batch");
    CHECK_NN(out, "out");
    out->update_count = b->update_count;
    out->ssd_iters = b->aux.ssd_iters;
    out->sync_steps = b->aux.sync_steps;
    out->env_call_count = b->r6.calls;
    out->reset_count = b->reset_count;
    return 0;
}

// Host fields only: every launch takes its counter as an argument, and the step graphs read theirs from sg.ubase,
// which pbn_step rewrites from update_count ahead of every call that replays one (upload_update_count).
int pbn_batch_set_counters(pbn_batch* b, const pbn_batch_counters* in) {
    CHECK_NN(b, "batch");
    CHECK_NN(in, "in");
    b->update_count = in->update_count;
    b->aux.ssd_iters = in->ssd_iters;
    b->aux.sync_steps = in->sync_steps;
    b->r6.calls = in->env_call_count;
    b->reset_count = in->reset_count;
    return 0;
}

int pbn_sync(pbn_batch* b) {
    CHECK_NN(b, "batch");
    SET_DEV(b);
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->r6.fault_check) {
        // a device-path env launch ran with the grid pool: its outputs reach the caller without a host
        // read, so a dropped env (a claimed slot whose words never arrived) is reported here
        b->r6.fault_check = false;
        int32_t f = 0;
        HIP_TRY(hipMemcpy(&f, b->d_error + 1, 4, hipMemcpyDeviceToHost));
        if (f) {
            HIP_TRY(hipMemset(b->d_error + 1, 0, 4));
            return fail(PBN_E_HIP, "k_env grid pool: a wait timed out in a device-path launch (an env's outputs "
                                   "were not written)");
        }
    }
    return 0;
}

int pbn_set_state(pbn_batch* b, const uint64_t* words) {
    CHECK_NN(b, "batch");
    CHECK_NN(words, "words");
    if (int rc = check_state_words(b, words)) return rc;
    SET_DEV(b);
    if (int rc = h2d(b, b->d_state, words, 8 * (size_t)b->W * b->B)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_get_state(pbn_batch* b, uint64_t* words) {
    CHECK_NN(b, "batch");
    CHECK_NN(words, "words");
    SET_DEV(b);
    const size_t bytes = 8 * (size_t)b->W * b->B;
    if (bytes <= PinBuf::CAP && b->pin.ready()) {
        HIP_TRY(hipMemcpyAsync(b->pin.p, b->d_state, bytes, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        memcpy(words, b->pin.p, bytes);
        return 0;
    }
    HIP_TRY(hipMemcpyAsync(words, b->d_state, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_set_state_device(pbn_batch* b, const void* dev_words) {
    CHECK_NN(b, "batch");
    CHECK_NN(dev_words, "dev_words");
    SET_DEV(b);
    HIP_TRY(hipMemcpyAsync(b->d_state, dev_words, 8 * (size_t)b->W * b->B, hipMemcpyDeviceToDevice, b->stream));
    return 0;
}

int pbn_get_state_device(pbn_batch* b, void* dev_words) {
    CHECK_NN(b, "batch");
    CHECK_NN(dev_words, "dev_words");
    SET_DEV(b);
    HIP_TRY(hipMemcpyAsync(dev_words, b->d_state, 8 * (size_t)b->W * b->B, hipMemcpyDeviceToDevice, b->stream));
    return 0;
}

int pbn_unpack_bits_device(pbn_batch* b, const void* d_words, void* d_bits) {
    CHECK_NN(b, "batch");
    CHECK_NN(d_bits, "d_bits");
    SET_DEV(b);
    const uint64_t total = b->B * (uint64_t)b->N;
    const int grid = (int)std::min<uint64_t>((total + BLOCK - 1) / BLOCK, (uint64_t)b->n_cu * 32u);
    int e = launch_unpack(d_words ? (const uint64_t*)d_words : b->d_state, (uint8_t*)d_bits, b->B, (uint32_t)b->N,
                          (uint32_t)b->W, std::max(grid, 1), b->stream);
    if (e) return fail(PBN_E_HIP, "k_unpack launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

int pbn_randomize_state(pbn_batch* b) {
    CHECK_NN(b, "batch");
    SET_DEV(b);
    return run_init(b, nullptr, nullptr, nullptr, nullptr);
}

int pbn_flip(pbn_batch* b, const int32_t* actions, int A, int offset, int dedup) {
    CHECK_NN(b, "batch");
    CHECK_NN(actions, "actions");
    if (int rc = validate_actions(b, actions, A, offset)) return rc;
    SET_DEV(b);
    size_t bytes = 4 * (size_t)A * b->B;
    if (int rc = b->s_act.ensure(bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(b->s_act.p, actions, bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemsetAsync(b->d_error, 0, 4, b->stream));
    FlipArgs a{b->d_state, (const int32_t*)b->s_act.p, b->B, A, offset, dedup ? 1 : 0, b->N, b->d_error};
    int e = launch_flip(b->W, a, b->grid_all(b->B), b->stream);
    if (e) return fail(PBN_E_HIP, "k_flip launch: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_flip_device(pbn_batch* b, const int32_t* d_actions, int A, int offset, int dedup, int check) {
    CHECK_NN(b, "batch");
    CHECK_NN(d_actions, "d_actions");
    if (int rc = check_action_shape(A, offset)) return rc;
    SET_DEV(b);
    int32_t* flag = nullptr;
    if (int rc = b->s_flip_err.get(b->stream, &flag)) return rc;
    FlipArgs a{b->d_state, d_actions, b->B, A, offset, dedup ? 1 : 0, b->N, flag};
    int e = launch_flip(b->W, a, b->grid_all(b->B), b->stream);
    if (e) return fail(PBN_E_HIP, "k_flip launch: %s", hipGetErrorString((hipError_t)e));
    if (!check) return 0;
    int32_t err;
    if (int rc = b->s_flip_err.read_and_clear(b, &err)) return rc;
    if (err) return fail(PBN_E_RANGE, "Invalid action: a value names no node (rows holding one were left untouched)");
    return 0;
}

// ------------------------------------------------------------------ R6 env config
int pbn_envcfg_create(const pbn_net* net, const pbn_envcfg_desc* d, pbn_envcfg** out) {
    CHECK_NN(net, "net");
    CHECK_NN(d, "desc");
    CHECK_NN(out, "out");
    *out = nullptr;
    if (d->n_cubes < 0 || d->n_cubes > 4096) return fail(PBN_E_INVALID, "n_cubes=%d outside [0, 4096]", d->n_cubes);
    if (d->n_cubes && (!d->cube_care || !d->cube_value)) return fail(PBN_E_INVALID, "cube arrays are NULL");
    if (d->n_reset_cubes < 0 || (d->n_reset_cubes && (!d->reset_care || !d->reset_value)))
        return fail(PBN_E_INVALID, "bad reset cubes");
    CHECK_NN(d->target_care, "target_care");
    CHECK_NN(d->target_value, "target_value");
    pbn_envcfg* c = new pbn_envcfg;
    if (int rc = build_envcfg_image(*net, d, c)) {
        delete c;
        return rc;
    }
    *out = c;
    return 0;
}

void pbn_envcfg_destroy(pbn_envcfg* c) {
    if (!c) return;
    for (DevCache* d : {&c->dev_image, &c->dev_reset, &c->dev_gen}) d->release();
    delete c;
}

// ------------------------------------------------------------------ timing
int pbn_timing_enable(pbn_batch* b, int enable) {
    CHECK_NN(b, "batch");
    if (enable < 0 || enable > 2) return fail(PBN_E_INVALID, "timing mode must be 0, 1 or 2");
    if (b->tm.mode == 2 && enable != 2) {
        // close the open region right behind the last launch; pbn_timing_read reports it
        if (int rc = close_region(b)) return rc;
        b->tm.region_closed = true;
        b->tm.mode = enable;
        return 0;
    }
    if (enable == 2 && b->tm.ev_pool.empty()) {
        // create the region's event pair now, not at its first launch (inside a timed window)
        SET_DEV(b);
        if (int rc = b->ev_new_pair()) return rc;
    }
    b->tm.mode = enable;
    b->tm.ev_used = 0;
    b->tm.region_launches = 0;
    b->tm.region_closed = false;
    b->tm.region_start = b->tm.region_end = nullptr;
    return 0;
}

int pbn_timing_read_each(pbn_batch* b, double* ms_each, uint64_t cap, uint64_t* launches) {
    CHECK_NN(b, "batch");
    if (b->tm.mode == 2 || b->tm.region_closed) return fail(PBN_E_INVALID, "per-launch times need timing mode 1");
    SET_DEV(b);
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t k = 0; k < b->tm.ev_used && k < cap; k++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, b->tm.ev_pool[k].first, b->tm.ev_pool[k].second));
        if (ms_each) ms_each[k] = ms;
    }
    if (launches) *launches = b->tm.ev_used;
    b->tm.ev_used = 0;
    return 0;
}

int pbn_timing_read(pbn_batch* b, double* kernel_ms, uint64_t* launches) {
    CHECK_NN(b, "batch");
    SET_DEV(b);
    const bool region = b->tm.mode == 2 || b->tm.region_closed;
    if (b->tm.mode == 2)
        if (int rc = close_region(b)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    double tot = 0;
    if (region) {
        float ms = 0;
        if (b->tm.region_launches) HIP_TRY(hipEventElapsedTime(&ms, b->tm.region_start, b->tm.region_end));
        tot = ms;
    } else {
        for (size_t k = 0; k < b->tm.ev_used; k++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, b->tm.ev_pool[k].first, b->tm.ev_pool[k].second));
            tot += ms;
        }
    }
    if (kernel_ms) *kernel_ms = tot;
    if (launches) *launches = region ? b->tm.region_launches : b->tm.ev_used;
    b->tm.ev_used = 0;
    b->tm.region_launches = 0;
    b->tm.region_closed = false;
    b->tm.region_start = b->tm.region_end = nullptr;
    return 0;
}

}  // extern "C"
