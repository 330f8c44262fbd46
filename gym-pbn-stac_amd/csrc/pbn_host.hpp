// pbn_host.hpp -- internal header of the host side of libpbnsim.so (pbn_abi*.cpp, pbn_image.cpp).
//
// The objects behind the C ABI's opaque handles, the error string and the small helpers more than one
// file uses. pbn_image.cpp (the packers) defines PBN_HOST_NO_HIP before including it: the part above the
// guard makes no use of HIP, so the packers compile and run with no HIP header (tests/host/image_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#ifndef PBN_HOST_NO_HIP
#include <hip/hip_runtime_api.h>
#endif

#include "../../include/pbn_abi.h"
#include "pbn_params.hpp"
#include "pbn_env_plan.hpp"
#include "pbn_step_plan.hpp"
#include "pbn_reach_rule.hpp"
#include "pbn_mass_rule.hpp"
#include "pbn_stateset.hpp"

using namespace pbn;

// functions and objects shared between the host files are internal: the library exports the C ABI of pbn_abi.h only
#define PBN_HIDDEN __attribute__((visibility("hidden")))

// The calling thread's last error message (pbn_last_error): one object for every file, defined in pbn_image.cpp.
extern PBN_HIDDEN thread_local std::string g_err;
PBN_HIDDEN int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define CHECK_NN(p, name) \
    if (!(p)) return fail(PBN_E_INVALID, "%s is NULL", name)

inline uint32_t align16(uint32_t x) { return (x + 15u) & ~15u; }

// One device copy per device of a host blob that never changes once uploaded (the network image, an env
// config's image, its reset cubes, its cooperative-draw image). Methods: pbn_abi.cpp.
struct DevCache {
    std::mutex mu;
    std::map<int, void*> dev;
    PBN_HIDDEN const void* on(int device, const void* host, size_t bytes);  // nullptr: the upload failed (nothing is kept)
    PBN_HIDDEN void release();
};

struct pbn_net {
    int kind = 0, N = 0, W = 0;
    int kmax = 0;                // truth-table networks: most inputs of one node
    std::vector<uint8_t> image;  // host copy of the LDS image (predictor mix: the compact image follows L.bytes)
    NetLayout L{};
    DevCache dev_image;
    const void* image_on(int device) { return dev_image.on(device, image.data(), image.size()); }
};

struct pbn_envcfg {
    const pbn_net* net = nullptr;
    int W = 0, H = 0, H_reset = 0;
    std::vector<uint8_t> image;  // net image + cubes [H][2][W] + target [2][W]
    NetLayout L{};
    uint32_t off_cubes = 0, off_target = 0, off_ndelta = 0;
    bool counters_ok = false;  // <= 8 cubes, each caring about <= 255 nodes: the byte counters apply (ENV_MODE_COUNTERS)
    std::vector<uint64_t> reset;  // care [H_reset][W], then value [H_reset][W]
    int32_t horizon = 100, reward_success = 1000, action_cost = 1, first_tested = 0;
    std::mutex mu;                   // guards gen_image's construction
    std::vector<uint8_t> gen_image;  // k_env ENV_MODE_COOP / _TAIL: the LDS image as staged (env_gen_image), built once
                                     // (erec_shift is fixed by the network and the cubes)
    DevCache dev_image, dev_reset, dev_gen;
};

// The packers (pbn_image.cpp): offset arithmetic and memcpy, no device call.
PBN_HIDDEN int build_predictor_image(const pbn_net_desc* d, pbn_net* n);
PBN_HIDDEN int build_table_image(const pbn_net_desc* d, pbn_net* n);
PBN_HIDDEN int build_envcfg_image(const pbn_net& net, const pbn_envcfg_desc* d, pbn_envcfg* c);
PBN_HIDDEN std::vector<uint8_t> env_gen_image(const pbn_envcfg* cfg, uint32_t erec_shift);
PBN_HIDDEN uint64_t net_select_u32(const pbn_net* n, int32_t node, uint32_t a);
PBN_HIDDEN void net_unstable(const pbn_net* n, int graph, const uint64_t* states, uint64_t n_states, uint64_t* masks);
PBN_HIDDEN void net_edge_mass(const pbn_net* n, int graph, const uint64_t* states, uint64_t n_states, uint64_t* mass);

#ifndef PBN_HOST_NO_HIP
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(PBN_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define SET_DEV(b) HIP_TRY(hipSetDevice((b)->device))

// Device memory, pinned host memory, streams, events and graph execs are given back by the destructor of the
// object that holds them, with the object's device current (pbn_batch_destroy, pbn_reach_destroy).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail(PBN_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        cap = bytes;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Pinned host staging for small transfers (single envs, small batches): pageable copies of a
// few bytes cost several microseconds each in the runtime's staging path.
struct PinBuf {
    static constexpr size_t CAP = 64 * 1024;
    uint8_t* p = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    bool ready() {
        if (!p && hipHostMalloc((void**)&p, CAP, hipHostMallocDefault) != hipSuccess) p = nullptr;
        return p != nullptr;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
};

struct pbn_batch;

// A sticky device flag: kernels OR 1 into it for every env they skip whole, the host reads it when a caller asks
// for a check. Zeroed at allocation and by every read. Each kernel family has its own, so that a family's check
// reports that family's skips only.
struct StickyFlag {
    DevBuf buf;
    int get(hipStream_t stream, int32_t** flag) {
        if (!buf.p) {
            if (int rc = buf.ensure(4)) return rc;
            HIP_TRY(hipMemsetAsync(buf.p, 0, 4, stream));
        }
        *flag = (int32_t*)buf.p;
        return 0;
    }
    // Waits for the batch's stream, reads the flag into *err and clears it (below pbn_batch).
    inline int read_and_clear(pbn_batch* b, int32_t* err);
};

template <size_t N>
inline void destroy_graph_execs(hipGraphExec_t (&x)[N]) {
    for (hipGraphExec_t& g : x) {
        if (g) (void)hipGraphExecDestroy(g);
        g = nullptr;
    }
}

// The device-open prologue of pbn_batch_create and pbn_reach_create.
inline int open_device(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(PBN_E_HIP, "no HIP device available (hipGetDeviceCount: %s); libpbnsim has no CPU path",
                    hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(PBN_E_RANGE, "device %d outside [0, %d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    return 0;
}

inline int check_action_shape(int A, int offset) {
    if (A < 1 || A > 4096) return fail(PBN_E_INVALID, "A=%d outside [1, 4096]", A);
    if (offset != 0 && offset != 1) return fail(PBN_E_INVALID, "offset must be 0 or 1");
    return 0;
}

// Launch knobs read from PBNSIM_* once at pbn_batch_create (read_knobs, pbn_abi.cpp): measurement / tests.
struct Knobs {
    int store_mode = -1;           // PBNSIM_STORE_MODE: 0 full, 1 changed envs whole, 2 their changed 16-B half, -1 = by size
    int envs_per_thread = 2;       // PBNSIM_ENVS_PER_THREAD: K, envs each thread walks per launch (pipelined)
    int step_block = 0;            // PBNSIM_STEP_BLOCK: 256 / 1024 threads per workgroup of the step kernel, 0 = by size
    int step_graph = -1;           // PBNSIM_STEP_GRAPH=0/1 forces step mode without / with HIP graphs, -1 = by size
    int step_chains = 0;           // PBNSIM_STEP_CHAINS: 1 / 2 / 4 launch chains of pbn_step, 0 = by size
    int roll_group = -1;           // PBNSIM_ROLL_GROUP: lanes per env of the rollout kernel, -1 = by size
    EnvKnobs env;             // PBNSIM_ENV_*: what env_plan reads (pbn_env_plan.hpp)
    int env_helpers = 3;      // PBNSIM_ENV_HELPERS: at most this many tail helpers per session (0-3; 0 = off)
    // PBNSIM_ENV_GRID_STEAL: grid-wide hand-off of tail envs (k_env, ENV_MODE_TAIL): 1 on, 0 off, unset = fused launches
    // and update caps from GPOOL_MIN_CAP (below it one env step's loops are too short to repay the waiting
    // workgroups' residency)
    int env_grid_steal = -1;
    int env_pool_cu_idle = -1;    // PBNSIM_ENV_POOL_CU_IDLE: 1 only idle CUs take pool tickets, 0 any idle workgroup,
                                  // -1 = the default (1)
    int env_grid_slots = 0;      // PBNSIM_ENV_GRID_SLOTS: pool slots in use (measurement: 1 keeps the waiting workgroups
                                 // resident but moves at most one env), 0 = GPOOL_CAP
    int ssd_wave = -1;        // PBNSIM_SSD_WAVE: 1 = one wave per env, 0 = one lane per env, -1 = by size
    bool ssd_serial = false;  // PBNSIM_SSD_SERIAL=1: wave mode applies each chunk serially (no chunk DAG)
    int ssd_shared = -1;      // PBNSIM_SSD_SHARED: 0 = one wave per env, 4 / 8 = that many, 1 = the default
                              // count, -1 = by size
    bool mt_lane_walk = false;  // PBNSIM_MT_LANES=1: MT-mode steps of predictor-mix networks on k_mt_step
    int envset_grid = 0;           // PBNSIM_ENVSET_GRID: cap on the workgroups of every lane-per-env step launch (k_tenv_step,
                                   // k_tenv_macro, k_env_set, k_census; tests: a small batch walks the grid-stride loop),
                                   // 0 = by occupancy
    bool envset_no_hull = false;   // PBNSIM_ENVSET_NO_HULL=1 (measurement): k_env_set without the hull pre-filter
    bool envset_no_skip = false;   // PBNSIM_ENVSET_NO_SKIP=1 (measurement): k_env_set looks up after unchanged updates too
};

struct pbn_batch {
    pbn_net* net = nullptr;
    int device = 0, W = 0, N = 0;
    hipStream_t stream = nullptr;      // the stream every call of this batch runs on
    hipStream_t own_stream = nullptr;  // created with the batch; `stream` unless pbn_batch_set_stream
    uint64_t B = 0, env_base = 0, seed = 0, update_count = 0;
    uint32_t reset_count = 0;
    uint64_t* d_state = nullptr;
    int64_t* d_nsteps = nullptr;
    int32_t* d_error = nullptr;
    const void* d_image = nullptr;
    int n_cu = 0, bpc_step = 1, bpc_base = 1, bpc_roll = 1;
    StepShape step;      // step mode's block, launch chains and graphs on / off (pbn_step_plan.hpp)
    int roll_group = 1;  // lanes per env of the rollout kernel
    Knobs knob;
    PinBuf pin;                         // staging for small host<->device copies
    StickyFlag s_flip_err;              // range-error flag of pbn_flip_device
    DevBuf s_act, s_obs, s_rew, s_flags, s_nup, s_replay_i, s_replay_k, s_off, s_mask;

    struct StepGraphs {
        // graph[c][j]: (STEP_GRAPH_K >> j) step launches of chain c's envs + k_bump on chain c's counter,
        // captured once (all sizes and chains at the first call of two or more steps). A graph holds one
        // chain only: it is a linear run of kernels.
        hipGraphExec_t graph[STEP_CHAINS_MAX][STEP_GRAPH_SIZES] = {};
        bool built = false;
        bool broken = false;        // capture or instantiation failed once: plain launches
        bool exact_broken = false;  // an exact-length capture failed once: no more of them
        // exact-length graphs: one replay for a whole call of n steps (pbn_step_prepare, or the second
        // call with the same n); each extra replay in a call costs a graph start on the device (~13 us)
        static constexpr int EXACT_GRAPHS = 4;
        uint32_t exact_n[EXACT_GRAPHS] = {};
        hipGraphExec_t exact_graph[EXACT_GRAPHS][STEP_CHAINS_MAX] = {};  // [slot][chain]
        uint64_t exact_used[EXACT_GRAPHS] = {};  // LRU stamps
        uint64_t exact_clock = 0;
        uint32_t last_n = 0;
        DevBuf ubase;  // device copies of update_count for graph replays, one 8-byte counter per chain
        ~StepGraphs() {
            for (auto& chain : graph) destroy_graph_execs(chain);
            for (auto& slot : exact_graph) destroy_graph_execs(slot);
        }
    } sg;
    // Launch chains of step mode (pbn_step): chain c steps the envs of step.sl[c] on its own stream, chain 0 on
    // `stream`. A call forks the extra streams off `stream` and joins them back into it, so everything else
    // queued on `stream` keeps its order against the whole batch.
    struct Chains {
        hipStream_t stream[STEP_CHAINS_MAX] = {};  // [1 .. step.chains): the batch's own, non-blocking; [0] unused
        hipEvent_t done[STEP_CHAINS_MAX] = {};     // [1 .. step.chains): end of chain c's launches of a call
        hipEvent_t fork = nullptr;
        ~Chains() {  // every call joined its chains into `stream`, and pbn_batch_destroy waited: these are idle
            for (hipStream_t s : stream)
                if (s) (void)hipStreamDestroy(s);
            for (hipEvent_t e : done)
                if (e) (void)hipEventDestroy(e);
            if (fork) (void)hipEventDestroy(fork);
        }
    } ch;
    hipStream_t chain_stream(int c) const { return c ? ch.stream[c] : stream; }
    struct R6 {
        uint32_t calls = 0;        // env steps launched (Philox call index)
        DevBuf counter;            // env-step work-queue head
        DevBuf steal;              // k_env tail hand-off: count of envs handed off
        DevBuf gpool;              // k_env grid pool: control words, slot states, slots
        uint32_t gpool_epoch = 0;  // the last R6 launch's pool epoch
        bool fault_check = false;  // a device-path env launch used the grid pool since the last pbn_sync
        EnvPlan last;              // of the last R6 launch
    } r6;
    struct MT {
        DevBuf py, np, pos_py, pos_np, seeds;  // allocated by pbn_mt_seed
        int ready = 0;
    } mt;
    struct Aux {
        DevBuf ssd_hist, ssd_tab;  // SSD histogram + gap/target tables
        uint64_t ssd_iters = 0;    // SSD iteration counter (Philox)
        DevBuf sync_tab;           // perturbation gap table
        uint64_t sync_steps = 0;   // synchronous-step counter (Philox)
    } aux;
    struct Tenv {        // the PBN-v0 env on the device (pbn_abi_tenv.cpp)
        StickyFlag err;  // of pbn_tenv_step_device / _macro_device, read by their checked calls
        int bpc = 0;     // k_tenv_step's resident workgroups per CU (0: not asked yet)
        int macro_bpc[2] = {0, 0};  // k_tenv_macro's, by mode
    } tenv;
    struct EnvSet {      // the until-attractor env over a state set (pbn_abi_env_set.cpp)
        StickyFlag err;  // of pbn_env_set_step_device / _reset_device, read by pbn_env_set_check
        int bpc = 0;     // k_env_set's resident workgroups per CU (0: not asked yet)
    } envset;
    // timing: mode 1 = an event pair around every launch; mode 2 = one region
    // (start before the first launch after enabling, stop after the latest launch)
    struct Timing {
        int mode = 0;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
        size_t ev_used = 0;
        uint64_t region_launches = 0;
        bool region_closed = false;
        hipEvent_t region_start = nullptr;  // ev_pool[0].first once the region's first launch is queued
        hipEvent_t region_end = nullptr;    // the closed region's stop event
        ~Timing() {
            for (auto& pr : ev_pool) {
                (void)hipEventDestroy(pr.first);
                (void)hipEventDestroy(pr.second);
            }
        }
    } tm;

    ~pbn_batch() {  // pbn_batch_destroy: the device is current and the streams have drained
        if (d_state) (void)hipFree(d_state);
        if (d_nsteps) (void)hipFree(d_nsteps);
        if (d_error) (void)hipFree(d_error);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }

    int grid_for(uint64_t items, int bpc, int block = BLOCK) const { return resident_grid(items, n_cu, bpc, block); }
    int grid_all(uint64_t items) const { return (int)std::max<uint64_t>((items + BLOCK - 1) / BLOCK, 1); }
    int ev_new_pair() {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        tm.ev_pool.emplace_back(a, b);
        return 0;
    }
    int ev_begin(hipEvent_t* stop) {
        *stop = nullptr;
        if (!tm.mode) return 0;
        if (tm.mode == 2) {
            if (tm.ev_pool.empty())
                if (int rc = ev_new_pair()) return rc;
            if (tm.region_launches == 0) {
                HIP_TRY(hipEventRecord(tm.ev_pool[0].first, stream));
                tm.region_start = tm.ev_pool[0].first;
            }
            tm.region_launches++;
            tm.ev_used = 1;
            return 0;  // the stop event is recorded once: pbn_timing_enable(0) or pbn_timing_read
        }
        if (tm.ev_used == tm.ev_pool.size())
            if (int rc = ev_new_pair()) return rc;
        auto& pr = tm.ev_pool[tm.ev_used++];
        HIP_TRY(hipEventRecord(pr.first, stream));
        *stop = pr.second;
        return 0;
    }
    int ev_end(hipEvent_t stop) {
        if (stop) HIP_TRY(hipEventRecord(stop, stream));
        return 0;
    }
};

// ev_begin; launch; ev_end around one kernel launch (`launch` returns the launcher's hipError_t as int).
template <class F>
inline int timed_launch(pbn_batch* b, const char* kernel, F&& launch) {
    hipEvent_t stop;
    if (int rc = b->ev_begin(&stop)) return rc;
    if (int e = launch()) return fail(PBN_E_HIP, "%s launch: %s", kernel, hipGetErrorString((hipError_t)e));
    return b->ev_end(stop);
}

// pbn_abi.cpp; used by the R6 entry points too
PBN_HIDDEN int validate_actions(const pbn_batch* b, const int32_t* actions, int A, int offset);
PBN_HIDDEN int h2d(pbn_batch* b, void* dst, const void* src, size_t bytes);
PBN_HIDDEN int run_init(pbn_batch* b, const pbn_envcfg* cfg, const void* d_mask, const void* care, const void* value);

// An exact set of packed states (pbn_stateset.hpp): the host copy, and with device >= 0 its upload. Read-only once
// built. Entry points in pbn_abi_tenv.cpp.
struct pbn_stateset {
    int device = -1;  // -1: host copy only
    StateSetTable t;
    DevBuf meta, keys;  // given back by the destructor (pbn_stateset_destroy makes the device current)
    SetView view() const { return SetView{(const uint32_t*)meta.p, (const uint64_t*)keys.p, t.slots}; }
};

inline int StickyFlag::read_and_clear(pbn_batch* b, int32_t* err) {
    int32_t* flag = nullptr;
    if (int rc = get(b->stream, &flag)) return rc;
    if (!b->pin.ready()) return fail(PBN_E_NOMEM, "pinned staging buffer");
    HIP_TRY(hipMemcpyAsync(b->pin.p, flag, 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemsetAsync(flag, 0, 4, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    memcpy(err, b->pin.p, 4);
    return 0;
}

// ---- what the entry points of the lane-per-env kernels share (pbn_abi_tenv.cpp, pbn_abi_env_set.cpp)

// The set can serve this batch's launches: uploaded, on the batch's device, over states of the batch's width.
// The two families answer a host-only set with different codes (pbn_tenv_*: PBN_E_STATE, pbn_env_set_*:
// PBN_E_INVALID), which their callers match; host_only_code keeps each its own.
inline int check_set_for_batch(const pbn_batch* b, const pbn_stateset* s, const char* what, int host_only_code) {
    if (s->device < 0) return fail(host_only_code, "%s is a host-only state set (created with device -1)", what);
    if (s->device != b->device)
        return fail(PBN_E_INVALID, "%s lives on device %d, the batch on device %d", what, s->device, b->device);
    if (s->t.n_nodes != b->N)
        return fail(PBN_E_INVALID, "%s holds states of %d nodes, the batch has %d", what, s->t.n_nodes, b->N);
    return 0;
}

inline int check_two_nodes(const pbn_batch* b) {
    if (b->N < 2) return fail(PBN_E_UNSUPPORTED, "PBN.step updates a node in [1, N-1]: the network needs two nodes");
    return 0;
}

// The kernel's resident workgroups per CU, asked once per batch: slot 0 = not asked yet.
inline int cached_bpc(int& slot, void* kernel, int W, uint32_t plane_off) {
    if (!slot)
        if (int e = max_blocks_lane_env(kernel, W, plane_off, &slot))
            return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

// The fields every lane-per-env argument struct starts from.
template <class Args>
inline void fill_lane_env(const pbn_batch* b, Args& a) {
    a.state = b->d_state;
    a.img = b->d_image;
    a.L = b->net->L;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
}

// One step launch over the whole batch: the grid is what is resident, capped by PBNSIM_ENVSET_GRID.
template <class Args>
inline int launch_lane_env_step(pbn_batch* b, const char* name, void* kernel, uint32_t plane_off, int bpc, Args& a) {
    int grid = b->grid_for(b->B, bpc);
    if (b->knob.envset_grid > 0) grid = std::min(grid, b->knob.envset_grid);
    return timed_launch(b, name, [&] { return launch_lane_env(kernel, b->W, plane_off, grid, b->stream, &a); });
}

// The graph of one state set of one network (pbn_abi_stg.cpp; the control entry points over it: pbn_abi_control.cpp).
// Host-only (device -1): the shape and the argument checks, no device memory.
struct pbn_stg {
    pbn_net* net = nullptr;
    int device = -1, W = 0;
    int graph = TABLE_GRAPH_NONE;  // truth-table networks: PBN_TABLE_GRAPH_STG / _STEP
    uint64_t n_states = 0;
    StateSetTable t;            // label = row index
    DevBuf rows, meta, keys;    // the states in row order, and the table over them
    DevBuf leaks;               // one uint64: the -1 entries written since the last pbn_stg_clear_leaks
    const void* d_image = nullptr;
    void* kernel = nullptr;
    int n_cu = 0, bpc = 1;
    int grid_cap = 0;  // PBNSIM_STG_GRID (tests: a small graph walks the grid-stride loop), 0 = what is resident
    enum { CTL_FLIP = 0, CTL_EXPECT, CTL_BACKUP, CTL_KERNELS };
    struct Ctl {  // the kernels of pbn_control.hip for this graph's shape, picked and asked for occupancy once
        void* kernel = nullptr;
        int bpc = 0;  // 0: not asked yet
    } ctl[CTL_KERNELS];
    Ctl absorb[4];  // k_stg_absorb (pbn_absorb.hip) for this graph's shape, by column tile 1, 2, 4, 8
    Ctl flipset[2];  // k_stg_flipset for this graph's shape and k_stg_flipset_select (pbn_flipset.hip)
    uint32_t first_node() const { return net->L.kind == KIND_PROB_TABLE ? table_graph_first_node(graph) : 0u; }
    SetView view() const { return SetView{(const uint32_t*)meta.p, (const uint64_t*)keys.p, t.slots}; }
};

// Attractor discovery (pbn_reach.hip); entry points in pbn_abi_reach.cpp.
struct pbn_reach {
    pbn_net* net = nullptr;
    int device = 0, W = 0;
    int graph = TABLE_GRAPH_NONE;  // truth-table networks: PBN_TABLE_GRAPH_STG / _STEP (pbn_reach_create_table)
    hipStream_t stream = nullptr;
    const void* d_image = nullptr;
    uint32_t max_states = 0, key_cap = 0, tcap = 0, fcap = 0;
    DevBuf keys, mark, table, ctl, queue, free_ring, hull, in, out;
    uint32_t* h_ctl = nullptr;  // pinned [REACH_CTL_WORDS + 1]: the control words, one word to send
    uint32_t free_limit = 0;    // free-ring positions below this are safe to take in the running level
    bool free_any = false;
    uint32_t n_keys = 0;        // entries reserved (live and dead) by the last closure
    uint32_t count = 0;         // live entries
    uint32_t epoch = 0;         // of the last mark_backward (0: none since the closure)
    bool complete = false;

    ~pbn_reach() {  // pbn_reach_destroy: the device is current and the stream has drained
        if (h_ctl) (void)hipHostFree(h_ctl);
        if (stream) (void)hipStreamDestroy(stream);
    }

    ReachArgs args() const {
        ReachArgs a{};
        a.img = d_image;
        a.L = net->L;
        a.first_node = table_graph_first_node(graph);
        a.keys = (uint64_t*)keys.p;
        a.mark = (uint32_t*)mark.p;
        a.table = (unsigned long long*)table.p;
        a.ctl = (uint32_t*)ctl.p;
        a.queue = (uint32_t*)queue.p;
        a.free_ring = (uint32_t*)free_ring.p;
        a.fmask = fcap - 1u;
        a.free_limit = free_limit;
        a.free_any = free_any ? 1u : 0u;
        a.hull = (unsigned long long*)hull.p;
        a.tmask = tcap - 1u;
        a.key_cap = key_cap;
        a.max_states = max_states;
        a.epoch = epoch;
        return a;
    }
    int read_ctl() {
        HIP_TRY(hipMemcpyAsync(h_ctl, ctl.p, 4 * REACH_CTL_WORDS, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return 0;
    }
    // one wave per frontier entry, at most REACH_CHUNK entries and REACH_MAX_GRID workgroups per launch
    int sweep(int which, uint32_t lo, uint32_t hi) {
        for (uint32_t c = lo; c < hi; c += REACH_CHUNK) {
            ReachArgs a = args();
            a.lo = c;
            a.hi = std::min(hi, c + REACH_CHUNK);
            const uint32_t grid = std::min(REACH_MAX_GRID, (a.hi - a.lo + 3u) / 4u);
            if (int e = launch_reach(W, which, a, (int)grid, stream))
                return fail(PBN_E_HIP, "reach launch: %s", hipGetErrorString((hipError_t)e));
        }
        return 0;
    }
    int upload(const uint64_t* words, uint64_t n) {
        if (int rc = in.ensure(8 * (size_t)W * n)) return rc;
        HIP_TRY(hipMemcpyAsync(in.p, words, 8 * (size_t)W * n, hipMemcpyHostToDevice, stream));
        return 0;
    }
};
#endif  // PBN_HOST_NO_HIP
