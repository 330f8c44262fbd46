// pbn_params.hpp -- plain structs shared by the host ABI (g++) and the kernels (hipcc).
#pragma once
#include <stdint.h>

namespace pbn {

enum { KIND_PREDICTOR_MIX = 1, KIND_PROB_TABLE = 2 };
enum {
    STREAM_STEP = 1,
    STREAM_INIT = 2,
    STREAM_ENV = 3,
    STREAM_RESET = 4,
    STREAM_SSD = 5,
    STREAM_SSD_FLIP = 6,
    STREAM_SYNC = 7,
    STREAM_SYNC_PERT = 8,
    STREAM_TENV_RESET = 9,  // pbn_tenv_reset_device: ctr {0, reset_count, env id}, row = mulhi(w[0], n_states)
    // pbn_tenv_macro_device, trigger mode: the stop draw after update u of env g is ctr {u_lo, u_hi, g} (one call per
    // env, not shared by an env pair), k53 = k53_of(w[0], w[1])
    STREAM_TENV_TRIGGER = 10
};
// STORE_DIRTY / STORE_HALF write back the envs whose updated bit changed: the whole env, or (W even and >= 4,
// 1024-thread step kernels) only the 16-B half that holds the bit (store_changed, pbn_device.hpp)
enum { STORE_FULL = 0, STORE_DIRTY = 1, STORE_HALF = 2 };
// R6 env-step modes: EnvArgs::mode, EnvPlan::mode and k_env's template parameter
enum EnvMode {
    ENV_MODE_CUBES = 0,     // the state matched against every cube after a change
    ENV_MODE_COUNTERS = 1,  // <= 8 cubes, each caring about <= 255 nodes: packed byte counters
    ENV_MODE_COOP = 2,      // and predictor mix, <= 16 predictors per node, Philox: cooperative draws
    ENV_MODE_GROUP = 3,     // group mode (k_env_grp)
    ENV_MODE_TAIL = 4       // as ENV_MODE_COOP with <= 4 cubes (one counter word): the tail kernel
};

constexpr int BLOCK = 256;          // 4 wave64 per workgroup
#ifndef PBN_ENV_BLOCK
#define PBN_ENV_BLOCK 256
#endif
// k_env's workgroup (lane / tail / hand-off modes; group mode k_env_grp keeps BLOCK): the workgroup is the
// tail hand-off's and the helpers' domain
constexpr int ENV_BLOCK = PBN_ENV_BLOCK;
static_assert(ENV_BLOCK % 64 == 0 && ENV_BLOCK / 64 <= 16, "k_env: whole waves, idle mask / helper codes fit");
// k_env's LDS budget per workgroup: 64 KiB at 256 threads (two workgroups per CU), the CU's 160 KiB above
constexpr uint32_t ENV_LDS_MAX = ENV_BLOCK > 256 ? 160u * 1024u : 64u * 1024u;
// a plane byte offset (dword * 4 * ENV_BLOCK) >> ENV_ROW_SHIFT = dword * 256: the tail writer-mask tables' row
constexpr uint32_t ENV_ROW_SHIFT = __builtin_ctz((unsigned)ENV_BLOCK / 64u);
constexpr int MAX_WORDS = 8;        // N <= 512
constexpr uint32_t MAX_IMAGE = 48 * 1024;  // LDS bytes for the network image (state planes come on top)

// Byte offsets of the tables inside the LDS image (16-byte aligned image).
// Predictor-mix networks use a padded per-node layout so that both table reads of an
// update are addressed by the node index alone (no dependent "node info" read):
//   thr [N][tp]   u64 selection thresholds, tp = max predictors - 1 rounded up to even,
//                 padding = UINT64_MAX (never reached: k53 < 2^53)
//   rec [N][pmax] u64 records in0 | in1<<16 | in2<<32 | tt<<48
struct NetLayout {
    uint32_t off_node;  // per-node info (truth-table networks)
    uint32_t off_thr;   // u64 thresholds
    uint32_t off_rec;   // predictor records (u64) or input lists (u16)
    uint32_t bytes;     // total, multiple of 16
    int32_t kind;
    int32_t n_nodes;
    uint32_t tp;        // predictor mix: thresholds per node (even)
    uint32_t pmax;      // predictor mix: record slots per node
    // LDS offset of the state planes of k_step / k_rollout / k_rollout_grp: max(bytes, the compact
    // image's size) for predictor mix (those kernels stage the compact image, which for pmax <= 3
    // is larger than the u64 one), bytes for tables. Every other kernel places its planes at bytes.
    uint32_t plane_off;
};

// Draws of the step and R6 streams use two 32-bit words per update: the node word and the
// predictor-choice uniform a, taken as k53 = a << 21 | a >> 11 (32 random bits spread over the
// 53-bit grid, monotone in a, so the integer thresholds decide the choice exactly; choice
// probabilities exact to 2^-32). One Philox call (four words) thus serves two updates:
//   STREAM_STEP: update u of env g takes call {u, g >> 1}, words 2(g & 1) and 2(g & 1) + 1 (envs
//                2m and 2m + 1 share a call);
//   STREAM_ENV:  update u of an env step takes call {u >> 1, call index}, words 2(u & 1), +1.
// Shared with oracle/pbn_oracle.c (u32_k53, step_words), which keeps its own copy.
constexpr uint64_t u32_k53(uint32_t a) { return ((uint64_t)a << 21) | (uint64_t)(a >> 11); }

// Threshold T re-expressed on a: the smallest a with u32_k53(a) >= T (2^32 = never), so that
// u32_k53(a) >= T <=> a >= u32_threshold(T) (u32_k53 is monotone; u32_k53(T >> 21 - 1) < T).
constexpr uint64_t u32_threshold(uint64_t T) {
    const uint64_t a0 = T >> 21;
    if (a0 >= (1ull << 32)) return 1ull << 32;
    return u32_k53((uint32_t)a0) >= T ? a0 : a0 + 1u;
}

// Compact LDS image of the Philox-driven predictor-mix kernels (k_step, k_rollout), whose choice
// uniform is a 32-bit word a (k53 = u32_k53(a)): thresholds re-expressed on a (u32_threshold)
// and stored as u32, rows padded to tp4 (a multiple of 4) so one ds_read_b128 serves 4 of them
// -- half the LDS bytes of the u64 thresholds, whose random-node reads are the most
// bank-conflicted reads of an update. u32_threshold can be 2^32 ("never": the u64 padding, or
// a threshold above k53(2^32 - 1)); it is stored saturated to 2^32 - 1, which a = 2^32 - 1
// passes. Thresholds are non-decreasing, so the never-entries of a node are its last tp - m_i;
// record slots q >= m_i all hold record m_i (slot rs >= tp4 + 1 per node), and the count's
// overshoot at a = 2^32 - 1 lands on the same record. Bit-exact with predictor_record(i, u32_k53(a)).
// Layout: thr32 [N][tp4] at 0, records u64 [N][rs] at rec_off (16-aligned). For pmax <= 3 it is
// larger than the u64 image, so the kernels that stage it place their planes at L.plane_off =
// max(L.bytes, its size); L.bytes itself stays the u64 image's size (what every other kernel and
// the env config stage). The host builds it (build_predictor_image, pbn_image.cpp) and appends it
// to the device image at offset L.bytes. This is the one definition, for host and kernels.
struct Thr32 {
    uint32_t tp4, rs, rec_off, bytes;
};

constexpr Thr32 thr32_layout(const NetLayout& L) {
    Thr32 X{};
    X.tp4 = (L.tp + 3u) & ~3u;
    X.rs = X.tp4 + 1u > L.pmax ? X.tp4 + 1u : L.pmax;
    X.rec_off = ((uint32_t)L.n_nodes * X.tp4 * 4u + 15u) & ~15u;
    X.bytes = (X.rec_off + (uint32_t)L.n_nodes * X.rs * 8u + 15u) & ~15u;
    return X;
}

struct StepArgs {
    uint64_t* state;             // [B][W]
    const void* img;             // network image (device, 16-B aligned)
    NetLayout L;
    uint64_t B;
    uint64_t env_base;           // global id of env 0 of this batch
    uint64_t seed;
    uint64_t update_base;        // Philox update counter of the first update
    uint32_t T;                  // updates per launch
    const uint32_t* replay_node; // [T][B] (replay mode)
    const uint64_t* replay_k53;  // [T][B]; null: forced nodes, choice words from the Philox step stream
    int32_t grp;                 // rollout: lanes per env (1 = k_rollout; 2/4/8 = k_rollout_grp)
    const uint64_t* ubase_dev;   // step mode in a HIP graph: update counter = *ubase_dev + update_base
};

struct InitArgs {
    uint64_t* state;
    uint64_t B, env_base, seed;
    uint32_t reset_count;
    int32_t n_nodes, kind;
    // env reset (R6): choose a cube among n_cubes, keep its cared bits, draw the rest
    const uint64_t* cube_care;   // [n_cubes][W] or null (plain randomize)
    const uint64_t* cube_value;
    int32_t n_cubes;
    const uint8_t* mask;         // [B] or null
    int64_t* n_steps;            // zeroed for reset envs, if non-null
};

struct FlipArgs {
    uint64_t* state;
    const int32_t* actions;  // [B][A]
    uint64_t B;
    int32_t A, offset, dedup, n_nodes;
    int32_t* error;          // set to 1 on an out-of-range action (device path)
};

struct EnvArgs {
    uint64_t* state;         // [B][W]
    int64_t* n_steps;        // [B]
    const int32_t* actions;  // [B][A]
    uint64_t* obs;           // [B][W]
    int32_t* reward;         // [B]
    uint8_t* flags;          // [B]
    uint32_t* n_updates;     // [B]
    int32_t* error;
    const void* img;         // network image + cubes appended
    NetLayout L;
    uint32_t off_cubes;      // care/value pairs [H][2][W] u64 inside the LDS image
    uint32_t off_target;     // target care/value [2][W]
    uint32_t off_ndelta;     // per node: uint2 packed mismatch-counter deltas (fast attractor test)
    unsigned long long* counter;  // work-queue head (zeroed per launch)
    int32_t n_cubes;
    int32_t mode;            // the kernel's mode: an EnvMode (above)
    uint32_t off_gen;        // ENV_MODE_COOP / _TAIL: per-wave draw buffers (ENV_GEN_WAVE_BYTES each);
                             // ENV_MODE_GROUP: per-group env rows (2W dwords per group of grp lanes)
    uint64_t B, env_base, seed;
    uint32_t call_idx, update_cap;
    int32_t A, offset, dedup, horizon, reward_success, action_cost;
    int32_t first_tested;     // 1: test the state after the first update too (pbn_target.py R5)
    const int64_t* draw_off;  // replay mode: [B+1]
    const uint32_t* draws_i;
    const uint64_t* draws_k;
    int32_t grp;              // ENV_MODE_GROUP: lanes per env (2, 4 or 8), k_env_grp
    uint32_t n_calls;         // env steps per env in this launch: actions [n_calls][B][A], outputs
                              // [n_calls][B]...; step t draws with Philox c1 = call_idx + t
    uint32_t erec_shift;      // ENV_MODE_COOP / _TAIL: LDS bytes the 16-B env records add over the 8-B records
                              // (off_cubes / off_target / off_ndelta / off_gen are LDS offsets)
    uint32_t tail_max;        // ENV_MODE_TAIL: a wave whose queue ran dry resolves its envs one at a time,
                              // 64 updates per block, once it holds at most this many (0 = never)
    uint32_t lane_limit;      // ENV_MODE_TAIL: lanes per wave that take envs from the work queue (64 = all;
                              // <= tail_max: every wave in tail mode from its first env)
    int32_t steal_local;      // ENV_MODE_TAIL: hand-off of tail envs between the waves of a workgroup (LDS)
    uint32_t* steal_count;    // envs handed off in this launch (diagnostics), zeroed per launch
    const void* gen_img;      // ENV_MODE_COOP / _TAIL: the LDS image as staged (host-built, pbn_image.cpp env_gen_image);
                              // null: the kernel builds it from img
    uint32_t chunk;           // ENV_MODE_COOP / _TAIL: updates per lane between draw rounds (ENV_CHUNK_SMALL / _LARGE)
    int32_t tail_helpers;     // ENV_MODE_TAIL (with steal_local): up to this many (<= 3) idle waves of the workgroup prepare a long tail
                              // session's blocks ahead (draws, records, writer masks) into the session wave's
                              // LDS ring, so the session wave only resolves (k_env, tail helpers)
    // ENV_MODE_TAIL (with steal_local): grid-wide hand-off of tail envs to workgroups that have run out of work
    // (k_env, "grid pool"). Device memory, control words zeroed per launch:
    uint32_t* gpool_ctl;      // [0] slots reserved by pushers, [1] tickets taken by idle workgroups, [2] live:
                              // workgroups working + envs in the pool, [3] envs pushed, [4] waits given up,
                              // [5] of the pushed, sessions moved mid-way (a long session no sibling could help)
    uint32_t* gpool_state;    // [gpool_cap] per slot: epoch << 2 | 1 (a pusher claimed it) or | 2 (its ticket
                              // holder gave up on it); any other epoch: unclaimed
    uint64_t* gpool;          // [gpool_cap][GPOOL_GRANULES] 8-B {epoch, value} granules: one env's hand-off words
    uint32_t gpool_cap;       // slots; 0 = grid hand-off off
    uint32_t gpool_epoch;     // this launch's tag (1 .. 2^30 - 1, a new one per launch)
    uint32_t gpool_cu_idle;   // 1: a workgroup takes tickets only once no workgroup of its CU is on its own envs;
                              // 0: as soon as its own waves have run out of work
};

// Env record (k_env, cooperative-draw mode): predictor record rec (in0 | in1<<16 | in2<<32 | tt<<48)
// of node i re-encoded for the LDS state planes of k_env's workgroups (ENV_BLOCK lanes): byte offsets of the plane
// dwords holding in0 / in1 (x), in2 / node i (y), tt | i << 16
// (w): the bit positions of in0, in1, in2, i in those dwords (one byte each). An update then reads
// its four plane dwords with no index arithmetic. Inputs are < 512 (W <= 8), so every offset is
// < 16 KiB.
// w: the truth table | the LDS byte address of node i's counter deltas (nd_off = the table's offset,
// 8 B per node; the R6 kernel's LDS stays below 64 KiB) << 16
struct EnvRecord {
    uint32_t x, y, z, w;
};

constexpr uint32_t env_plane_off(uint32_t x) { return (x >> 5) * (uint32_t)(ENV_BLOCK * 4); }

constexpr EnvRecord env_record_words(uint64_t rec, uint32_t i, uint32_t nd_off) {
    const uint32_t x0 = (uint32_t)rec & 0xFFFFu, x1 = (uint32_t)(rec >> 16) & 0xFFFFu,
                   x2 = (uint32_t)(rec >> 32) & 0xFFFFu;
    return EnvRecord{env_plane_off(x0) | (env_plane_off(x1) << 16), env_plane_off(x2) | (env_plane_off(i) << 16),
                     (x0 & 31u) | ((x1 & 31u) << 8) | ((x2 & 31u) << 16) | ((i & 31u) << 24),
                     (uint32_t)(rec >> 48) | ((nd_off + 8u * i) << 16)};
}

constexpr uint32_t GPOOL_GRANULES = 64;  // per slot: the hand-off box as u32 words (10 + 4W <= 64 for W <= 13)
constexpr uint32_t GPOOL_CAP = 8192;     // grid pool slots (4 MiB); envs past them stay with their wave
// control words: [0, 16) counters, [GPOOL_CU_WORD + __smid()] workgroups on that CU still on their own envs
// (__smid() < 1024: XCC, SE, CU id bits); the block is zeroed per launch
constexpr uint32_t GPOOL_CU_WORD = 16, GPOOL_CTL_BYTES = 4u * (GPOOL_CU_WORD + 1024u);
// the pool is on by default for fused launches (several env steps) and for launches whose update cap is at least
// this (pbn_abi_env.cpp env_plan): one env step at config 5's 4,096 cap lost more to the waiting workgroups'
// residency than the moved envs gave back (1.14 -> 1.18-1.20 ms per step)
constexpr uint32_t GPOOL_MIN_CAP = 16384;

constexpr uint32_t MT_ROW = 624;
constexpr uint32_t MT_TAIL_PAD = 64;  // words allocated past the last row (the twist's unconditional loads read up to 29)

// 1 / log2(1-p) from a geometric-gap table T_k = floor((1-p)^k 2^32) (host side): taken at the
// largest k whose T_k keeps >= 20 significant bits; 0 when every T_k is tiny (p ~ 1).
inline float gap_inv_log2(const uint32_t* T, int N) {
    for (int k = N; k >= 1; --k)
        if (T[k - 1] >= (1u << 20)) return (float)((double)k / __builtin_log2((double)T[k - 1] / 4294967296.0));
    return 0.0f;
}  // u32 words of one MT19937 state row

struct MTArgs {
    uint64_t* state;        // [B][W]
    const void* img;        // network image
    NetLayout L;
    uint64_t B;
    uint32_t T;             // transitions per launch (k_mt_step)
    int32_t n_nodes;
    int32_t init_state;     // k_mt_step: run genRandState / PBN.reset(None) (N init draws) instead of T updates
    const uint64_t* seeds;  // [B] (k_mt_seed)
    uint32_t* mt_py;        // [B][MT_ROW] CPython `random` state
    uint32_t* mt_np;        // [B][MT_ROW] numpy legacy RandomState (probability-table networks)
    uint32_t* pos_py;       // [B] next word index (624 = twist before next use: k_mt_step twists it, coalesced)
    uint32_t* pos_np;
    int32_t lane_walk;      // predictor-mix steps on k_mt_step instead of k_mt_staged (PBNSIM_MT_LANES=1, tests)
};

constexpr int SSD_DAG_KMAX = 6;
// waves per env in shared mode (k_ssd_wave): 4 measured faster than 8 (300 envs x 4,000: 0.19 vs
// 0.23 ms; 1,024 envs: 10.4 vs 8.8 G transitions/s; tools/ssd_shared_sweep.py)
constexpr int SSD_SHARED_WAVES = 4;  // truth-table nodes with more inputs: k_ssd_wave applies serially

struct SSDArgs {
    uint64_t* state;           // [B][W]
    const void* img;           // network image
    NetLayout L;
    uint64_t B, env_base, seed;
    uint64_t iter_base;        // SSD iteration counter of the first iteration (Philox c0/c1)
    uint32_t iters;
    int32_t n_targets;         // g <= 12 (2^g LDS bins)
    const int32_t* targets;    // [g] node indices, first = most significant bucket bit
    const uint32_t* gap_thr;   // [N] T_k = floor((1-p)^k 2^32), k = 1..N; null = no flips
    float gap_inv_log2;        // 1 / log2(1-p) estimated from the table (geo_gap's first guess)
    uint64_t* hist;            // [2^g] accumulated counts (device)
    uint32_t off_planes, off_gap, off_tbit, off_targets, off_hist, lds_bytes;
    int32_t wave;              // 1: one wave per env (k_ssd_wave), small batches
    int32_t dag;               // wave mode: resolve each 64-iteration chunk in parallel (predictor mix,
                               // or truth tables with <= SSD_DAG_KMAX inputs per node); the value is
                               // the waves per env (1, or 4: the workgroup shares one env)
    int32_t* error;            // set to 1 if a shared-mode wave gave up waiting for its turn (never expected)
};

struct SyncArgs {
    uint64_t* state;          // [B][W]
    const void* img;          // network image
    NetLayout L;
    uint64_t B, env_base, seed;
    uint64_t step_base;       // synchronous-step counter of the first step (Philox)
    uint32_t T;
    const uint32_t* gap_thr;  // [N] perturbation gap table (T_k = floor((1-p)^k 2^32)); null = off
    float gap_inv_log2;       // 1 / log2(1-p) estimated from the table
    uint32_t off_planes, off_gap, lds_bytes;
};

// Attractor discovery (pbn_reach.hip): an exact device set of packed states plus the support-graph kernels
// that grow it (forward closure) and mark inside it (backward reachability). DESIGN.md §11.
//   keys   [key_cap][W]; entry e is live once a table slot points at it, dead (mark REACH_DEAD) if its
//          inserter lost the publish to an equal key or could not place it. A dead entry goes onto the free
//          ring and is handed out again from the next BFS level on.
//   table  open addressing, [tmask + 1] u64: 0 = empty, else hash tag << 32 | entry + 1; written once (CAS)
//   queue  [key_cap] entry indices: every publish (forward) or mark (backward) appends one; a frontier is a
//          range of it
//   ctl    REACH_CTL_WORDS u32 counters, see the enum
enum {
    REACH_KEYS = 0,       // entries taken from the end of keys (may run past key_cap: the host clamps)
    REACH_COUNT = 1,      // live entries: successful publishes
    REACH_OVERFLOW = 2,   // an insert found max_states entries, a full key array or a full table
    REACH_QTAIL = 3,      // queue: entries appended
    REACH_MISSING = 4,    // mark_backward: the start state is not in the set
    REACH_FREE_HEAD = 5,  // free ring: entries taken (may run past the level's limit: the host clamps)
    REACH_FREE_TAIL = 6,  // free ring: entries pushed
    REACH_CTL_WORDS = 8
};
constexpr uint32_t REACH_NONE = 0xFFFFFFFFu;
constexpr uint32_t REACH_DEAD = 0x80000000u;     // mark of a dead entry (epochs stay below it)
constexpr uint32_t REACH_CHUNK = 16384;          // frontier entries per launch (short launches; a level takes several)
constexpr uint32_t REACH_MAX_GRID = 2048;        // workgroups per launch (4 waves each; a wave walks its entries)
// the edge-rule kernels stage the whole network image as dynamic LDS and ask for no more than a launch gets
// without opting in; a network whose image is larger has no pbn_reach (TT-200: 28.8 KiB)
constexpr uint32_t REACH_LDS_MAX = 64u * 1024u;

struct ReachArgs {
    const void* img;             // network image (the u64 image of either kind; L.kind selects the edge rule)
    NetLayout L;
    uint32_t first_node;         // lowest node that may move: 0, or 1 for a truth-table network's "step" graph
    uint64_t* keys;
    uint32_t* mark;              // [key_cap] epoch of the last mark_backward that reached the entry, or REACH_DEAD
    unsigned long long* table;
    uint32_t* ctl;
    uint32_t* queue;
    uint32_t* free_ring;         // [fmask + 1] dead entries, positions REACH_FREE_HEAD .. REACH_FREE_TAIL
    unsigned long long* hull;    // [2][W]: AND, OR over the live entries
    const uint64_t* in;          // unstable / seed / mark start: states [n_in][W]
    uint64_t* out;               // unstable: masks [n_in][W]
    uint64_t n_in;
    uint32_t tmask, key_cap, max_states, fmask;
    uint32_t free_limit;         // ring positions below this were pushed by earlier levels: safe to take
    uint32_t free_any;           // 0: nothing to take in this level (skip the counter)
    uint32_t lo, hi;             // this launch's slice of the queue (hull: of keys)
    uint32_t epoch;
};

// The PBN-v0 env on the device (pbn_tenv.hip): an exact state set a kernel can query
// (pbn_stateset.hpp) and the fused step; its reset over a table of states is EnvSetResetArgs' (below).
struct SetView {
    const uint32_t* meta;  // [slots] 0 = empty, else label + 1
    const uint64_t* keys;  // [slots][W]
    uint32_t slots;        // a power of two
};

struct SetLookupArgs {
    const uint64_t* words;  // [B][W]: the batch's state or the caller's words
    SetView set;
    uint64_t B;
    int32_t* labels;  // [B]
};

struct TenvArgs {
    uint64_t* state;         // [B][W]
    const void* img;         // truth-table network image
    NetLayout L;
    uint64_t B, env_base, seed;
    uint64_t update;         // the batch's update counter: this step is update `update` of every env
    const int32_t* actions;  // [B]: 0 = none, a in [1, N-1] flips node a
    SetView target;
    int32_t reward_target, step_cost, action_cost;
    uint64_t* obs;           // [B][W] or null
    int32_t* reward;         // [B]
    uint8_t* flags;          // [B]
    int32_t* labels;         // [B] or null
    int32_t* error;          // sticky: set to 1 by an env whose action names no node (the env is skipped)
};

// The macro-action envs (k_tenv_macro): up to t_max rounds of flip + update + lookup + reward per env in
// one launch. TenvMacroArgs::mode and the kernel's template parameter (PBN_MACRO_* in pbn_abi.h).
enum { TENV_MACRO_INTERVAL = 0, TENV_MACRO_TRIGGER = 1 };
constexpr uint32_t TENV_MACRO_MAX_T = 65536;  // PBN_TENV_MACRO_MAX_T
constexpr int32_t TENV_MACRO_MAX_PROB = 10;   // trigger mode: the stop probability in tenths

struct TenvMacroArgs {
    uint64_t* state;         // [B][W]
    const void* img;         // truth-table network image
    NetLayout L;
    uint64_t B, env_base, seed;
    uint64_t update;         // the batch's update counter: inner iteration i is update `update + i` of every env
    const int32_t* actions;  // [B]: 0 = none, a in [1, N] flips node a - 1 before every inner update
    const int32_t* limit;    // [B]: the interval in [1, t_max], or the stop probability in tenths in [1, 10]
    SetView target;
    int32_t reward_target, step_cost, action_cost;
    int32_t mode;
    uint32_t t_max;
    const double* gpow;        // [t_max] gamma ** i (trigger mode)
    const uint64_t* stop_thr;  // [11] floor((p / 10) 2^53), entry 0 unused (trigger mode)
    uint64_t* obs;             // [B][W] or null: the final state
    int32_t* reward_i32;       // [B] (interval mode)
    double* reward_f64;        // [B] (trigger mode)
    uint8_t* flags;            // [B]
    int32_t* interval;         // [B] or null: inner iterations run
    int32_t* first_hit;        // [B] or null: the first iteration whose state was in the target, or -1
    int32_t* labels;           // [B] or null: the target set's label of the final state
    int32_t* error;            // the sticky flag of TenvArgs::error
};

// The until-attractor multi-flip env over an exact labelled state set (k_env_set, pbn_env_set.hip):
// k_env's env step with "attracting" read as "member of the set", a target label per env.
struct EnvSetArgs {
    uint64_t* state;         // [B][W]
    int64_t* n_steps;        // [B]
    const int32_t* actions;  // [B][A]
    const void* img;         // network image (either kind)
    NetLayout L;
    uint64_t B, env_base, seed;
    uint32_t call_idx, update_cap;
    int32_t A, offset, dedup, horizon, reward_success, action_cost;
    int32_t first_tested;    // 1: the state after the first update is tested, not the snapshot
    SetView set;
    uint64_t hull_all[MAX_WORDS], hull_any[MAX_WORDS];  // the set's AND / OR words (the first W are read)
    int32_t always_lookup;   // measurement (PBNSIM_ENVSET_NO_SKIP): look up after unchanged updates too
    int32_t target_label;    // the target of every env when target_labels is null
    const int32_t* target_labels;  // [B] or null
    uint64_t* obs;           // [B][W]
    int32_t* reward;         // [B]
    uint8_t* flags;          // [B]
    uint32_t* n_updates;     // [B]
    int32_t* labels;         // [B] or null
    int32_t* error;          // sticky: set to 1 by an env whose action row names no node (the env is skipped)
};

// k_env_set_reset serves pbn_env_set_reset_device and, with row_off and n_steps null, pbn_tenv_reset_device.
struct EnvSetResetArgs {
    uint64_t* state;
    int64_t* n_steps;          // zeroed for reset envs, if non-null
    uint64_t B, env_base, seed;
    uint32_t reset_count;
    uint32_t n_rows;           // row_off null: rows is one attractor of n_rows >= 1 rows
    const uint64_t* rows;      // [S][W], ordered by label
    const uint32_t* row_off;   // [n_labels + 1]: attractor k's rows are row_off[k] .. row_off[k + 1] - 1; or null
    int32_t n_labels;
    int32_t source_label;      // the source of every env when source_labels is null
    const int32_t* source_labels;  // [B] or null
    const uint8_t* mask;       // [B] or null
    int32_t clear_node0;       // truth-table networks: node 0 cleared (pbn.py:118)
    int32_t* error;            // EnvSetArgs::error: set to 1 by an env whose source names no non-empty attractor
};

// The exact transition graph of a state set (k_stg_rows, pbn_stg.hip): for rows [first_row, first_row +
// n_rows) of `states`, the edge mass (pbn_mass_rule.hpp) of every node and the row of the neighbour it leads to.
constexpr uint64_t STG_MAX_CELLS = 1ull << 31;  // n_rows * N of one call: a cell index fits 32 bits

struct StgArgs {
    const void* img;            // network image (the u64 image of either kind; L.kind selects the mass rule)
    NetLayout L;
    uint32_t first_node;        // lowest node that may move (ReachArgs::first_node)
    const uint64_t* states;     // [S][W] the set's rows, in row order
    SetView set;                // the same rows as a table, label = row index
    uint32_t first_row;
    uint64_t n_cells;           // n_rows * N <= STG_MAX_CELLS
    unsigned long long* mass;   // [n_rows][N]
    int32_t* succ;              // [n_rows][N]: the neighbour's row; -1 a leak; the row itself where mass == 0
    unsigned long long* leaks;  // += the -1 entries written
};

// Optimal control over a transition graph (pbn_control.hip). The cell index row * N + node is 64-bit
// in all three: S * N reaches 2^33.
struct StgFlipArgs {
    const uint64_t* states;        // [S][W] the set's rows, in row order
    SetView set;                   // the same rows as a table, label = row index
    uint64_t first_row, n_cells;   // rows [first_row, first_row + n_cells / N)
    uint32_t n_nodes;
    uint64_t allowed[MAX_WORDS];   // bit i: node i may be flipped (the first W words are read)
    int32_t* nbr;                  // [n_rows][N]: the row of x_row ^ bit(i); -1 outside the set or not allowed
};

struct StgExpectArgs {
    const unsigned long long* mass;  // [S][N]
    const int32_t* succ;             // [S][N]
    const double* v;                 // [S]
    double* out;                     // [S] E[v(next) | s]
    const double* pen;               // [S] or null
    double cost;
    double* out_pen;                 // [S] out - cost * pen (pen non-null)
    uint64_t n_states;
    uint32_t n_nodes;
    double n_movable;
};

struct StgBackupArgs {
    const int32_t* nbr;  // [S][N]
    const double* u;     // [S] the no-op's value
    const double* ua;    // [S] the value of arriving at a row by a flip
    double* v;           // [S] the max
    int32_t* policy;     // [S] -1 the no-op, else the node
    uint64_t n_states;
    uint32_t n_nodes;
};

// Absorption over a transition graph (pbn_absorb.hip): one Jacobi sweep of n_cols columns of x into out.
constexpr int STG_ABSORB_MAX_COLS = 8;  // PBN_STG_ABSORB_MAX_COLS
struct StgAbsorbSrc {
    double b[STG_ABSORB_MAX_COLS];  // the source constant of each column (the first n_cols are read)
};
struct StgAbsorbArgs {
    const unsigned long long* mass;  // [S][N]
    const int32_t* succ;             // [S][N]
    const int32_t* label;            // [S]: -1 a transient row, >= 0 a held row
    const double* x;                 // [S][ld]
    double* out;                     // [S][ld], not x: columns [0, n_cols) are written
    uint64_t ld;                     // >= n_cols
    uint64_t n_states;
    uint32_t n_nodes;
    uint32_t n_cols;                 // [1, STG_ABSORB_MAX_COLS]
    double n_movable;
    StgAbsorbSrc src;
};

// The max over multi-flip action sets (pbn_flipset.hip). A summary is base [S][2] float64 and tag [S][2]
// int32 (pbn_flipset_rule.hpp: y | d << 24, -1 none), the better entry first.
struct StgFlipsetArgs {
    const int32_t* nbr;      // [S][N]: pbn_stg_flip_rows_device's array for the allowed nodes
    const double* m;         // [S] the worth of arriving at a row: level 0 (in_base null), and the select
    const double* in_base;   // [S][2] T_{j-1}, or null: T_0 is made from m
    const int32_t* in_tag;   // [S][2]
    double* out_base;        // [S][2] T_j, not in_base
    int32_t* out_tag;        // [S][2]
    double cost;             // k >= 0, per flip
    uint64_t n_states;
    uint32_t n_nodes;
};

struct StgFlipsetSelectArgs {
    const double* base;      // [S][2] T_A
    const int32_t* tag;      // [S][2]
    const double* m;         // [S]
    double cost, noop_cost;  // noop_cost is read where has_noop
    uint32_t has_noop;
    uint64_t n_states;
    double* v;               // [S] the best action's value (-inf: none)
    int32_t* policy_end;     // [S] the row it leads to (the row itself: the empty set; -1: none)
    int32_t* policy_flips;   // [S] its flip count
};

// Launchers (pbn_step.hip, pbn_state.hip, pbn_env.hip, pbn_group.hip, pbn_mt.hip, pbn_ssd.hip, pbn_sync.hip, pbn_reach.hip,
// pbn_tenv.hip, pbn_tenv_macro.hip, pbn_env_set.hip, pbn_stg.hip, pbn_control.hip, pbn_absorb.hip, pbn_flipset.hip). Return hipError_t as int.
// The lane-per-env kernels (pbn_lane_env.hpp): each file picks its kernel (nullptr: none for that shape), one
// launcher and one occupancy query serve them all. plane_off: the LDS byte offset of the kernel's state planes;
// args: the kernel's argument struct.
void* tenv_step_kernel(int W);
void* tenv_macro_kernel(int W, int mode);
void* env_set_kernel(int W, int kind);
int launch_lane_env(void* kernel, int W, uint32_t plane_off, int grid, void* stream, void* args);
int max_blocks_lane_env(void* kernel, int W, uint32_t plane_off, int* blocks_per_cu);
int launch_env_set_reset(int W, const EnvSetResetArgs& a, void* stream);
enum { REACH_K_UNSTABLE = 0, REACH_K_SEED, REACH_K_EXPAND, REACH_K_BACK_START, REACH_K_BACK, REACH_K_HULL };
int launch_reach(int W, int which, const ReachArgs& a, int grid, void* stream);
int launch_set_lookup(int W, const SetLookupArgs& a, void* stream);
void* stg_rows_kernel(int W, int kind);  // pbn_stg.hip; nullptr: none for that shape
int launch_stg_rows(void* kernel, const StgArgs& a, int grid, void* stream);
int max_blocks_stg_rows(void* kernel, uint32_t image_bytes, int* blocks_per_cu);
// pbn_control.hip: each picks its kernel (nullptr: none for that shape; G, one_cell: ControlPlan's G and cells_per_lane == 1),
// one launcher (BLOCK threads, no LDS; args: the kernel's argument struct) and one occupancy query serve the three
void* stg_flip_rows_kernel(int W);
void* stg_expect_kernel(uint32_t G, bool one_cell);
void* stg_backup_kernel(uint32_t G, bool one_cell);
int launch_control(void* kernel, int grid, void* stream, void* args);
int max_blocks_control(void* kernel, int* blocks_per_cu);
// pbn_absorb.hip: the kernel for AbsorbPlan's G, cells_per_lane == 1 and col_tile (nullptr: none for that shape); launched
// and asked for occupancy through launch_control / max_blocks_control
void* stg_absorb_kernel(uint32_t G, bool one_cell, uint32_t col_tile);
// pbn_flipset.hip: the level kernel for ControlPlan's G and cells_per_lane == 1 (nullptr: none for that shape) and the
// select kernel (a lane per row); launched and asked for occupancy through launch_control / max_blocks_control
void* stg_flipset_kernel(uint32_t G, bool one_cell);
void* stg_flipset_select_kernel();
int launch_bump(uint64_t* p, uint64_t k, void* stream);
int launch_set_counters(uint64_t* p, uint64_t v, uint32_t n, void* stream);
int launch_step(int W, const StepArgs& a, int store_mode, int replay, int sb, int grid, void* stream);
uint32_t step_lds_bytes(int W, uint32_t image_bytes, int sb, int grp = 1);
int launch_init(int W, const InitArgs& a, int grid, void* stream);
int launch_flip(int W, const FlipArgs& a, int grid, void* stream);
int launch_unpack(const uint64_t* words, uint8_t* out, uint64_t B, uint32_t N, uint32_t W, int grid, void* stream);
int launch_env_multi(int W, const EnvArgs& a, int replay, int grid, void* stream);
int max_blocks_step(int W, int kind, uint32_t lds_bytes, int sb, int* blocks_per_cu, int rollout = 0, int grp = 1);

#ifndef PBN_ENV_CHUNK
#define PBN_ENV_CHUNK 32
#endif
constexpr uint32_t ENV_CHUNK = PBN_ENV_CHUNK;  // updates per lane between refill rounds
#ifndef PBN_ENV_UNROLL
#define PBN_ENV_UNROLL 8
#endif
constexpr uint32_t ENV_UNROLL = PBN_ENV_UNROLL;  // updates between the wave's "any lane active" tests
// k_env tail mode: live envs per wave at (or below) which a wave whose queue ran dry switches to
// resolving one env at a time across all 64 lanes (PBNSIM_ENV_TAIL overrides; measured: DESIGN.md §6)
constexpr uint32_t ENV_TAIL_DEFAULT = 16;
// Batches of up to this many envs per wave slot (n_cu x workgroups per CU x 4 waves: 3,072 for
// Bittner-200 on 256 CUs): one lane per wave takes envs (EnvArgs::lane_limit = 1), so every wave
// works in tail mode on one env at a time and takes the next from the queue. Measured against lane
// mode (profiles/r03_r6_lanes_sweep.json): faster or tied on every line up to 16,384 envs (5.3 per
// slot; e.g. 8,192 envs, cap 4,096: 0.19 vs 0.96 ms per step); at 32,768 the spec attractors' per-step
// line is 31 % slower (short env steps queue behind long ones in one wave), so 6 per slot
constexpr uint64_t ENV_ONE_LANE_ENVS_PER_SLOT = 6;
// Cooperative-draw kernels (ENV_MODE_COOP / _TAIL) take their chunk (updates per lane between draw
// rounds) per launch, EnvArgs::chunk: 48 by default -- fewer chunk prologues on the long per-lane
// chains of a per-step launch (131,072 envs, cap 4,096: 1.22 -> 1.17 ms per step) -- and 32 where the
// smaller draw buffers let one more workgroup onto a CU and the launch is throughput-bound (a fused
// multi-step launch over a queue of several envs per lane: 1M envs, T = 100, 3.46 vs 4.05 ms per env
// step); profiles/r04_r6_chunk_sweep.json
constexpr uint32_t ENV_CHUNK_SMALL = 32, ENV_CHUNK_LARGE = 48;
// a wave's draw buffer: the draw table [chunk][64] u16, 64 B (the hand-off flag in tail mode), the
// shared rounds' counter table [64] uint4 by rank (the hand-off box in tail mode)
constexpr uint32_t env_gen_wave_bytes(uint32_t chunk) { return chunk * 64u * 2u + 64u + 64u * 16u; }
// lds_bytes: the image's; the workgroup's LDS is env_lds_bytes of it (pbn_env_plan.hpp)
int max_blocks_env(int W, int kind, int mode, int grp, uint32_t lds_bytes, int* blocks_per_cu, uint32_t chunk = ENV_CHUNK_LARGE);
inline int env_block(int mode) { return mode == ENV_MODE_GROUP ? BLOCK : ENV_BLOCK; }  // threads per workgroup of the R6 kernel
int launch_mt_seed(int W, const MTArgs& a, int grid, void* stream);
int launch_mt_step(int W, const MTArgs& a, int n_cu, void* stream);  // grid from the kernel's occupancy
uint32_t ssd_block(const SSDArgs& a);
uint32_t ssd_layout(int W, uint32_t image_bytes, int n_nodes, int n_targets, SSDArgs* a);
int launch_ssd(int W, const SSDArgs& a, int grid, void* stream);
uint32_t sync_layout(int W, uint32_t image_bytes, int n_nodes, SyncArgs* a);
int launch_sync(int W, const SyncArgs& a, int grid, void* stream);

}  // namespace pbn
