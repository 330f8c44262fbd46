// env_plan_check.cpp -- the R6 launch plan (csrc/pbn_env_plan.hpp) on the CPU.
//
// Built by `make envplancheck` with ASan + UBSan; no HIP header, no library, no GPU. plan_ref below restates
// env_plan, env_group_size, pbn_batch::grid_for and env_lds_bytes as pbn_abi_env.cpp, pbn_host.hpp and pbn_env.hip
// held them before the header existed, with the constants written out, so a change to the header that changes
// what a launch does fails here. Both sides query the same made-up occupancy function; the queries they make
// must be the same, in the same order. Every plan is counted into classes, and an empty class fails the check:
// the grid below cannot shrink to one that misses a branch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "pbn_env_plan.hpp"

using namespace pbn;

static_assert(ENV_BLOCK == 256 && BLOCK == 256, "plan_ref writes the default workgroup sizes out");

#define REQUIRE(cond)                                                                                  \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            std::fprintf(stderr, "env_plan_check: %s failed (%s) at line %d\n", #cond, context(), __LINE__); \
            std::exit(1);                                                                              \
        }                                                                                              \
    } while (0)

// what a failed REQUIRE names: the input under check (written out only then), or a fixed text
static const EnvPlanIn* ctx_in = nullptr;
static int ctx_fail_at = -1;
static const char* ctx_text = "";

static const char* context() {
    static char buf[512];
    if (!ctx_in) return ctx_text;
    const EnvPlanIn& in = *ctx_in;
    std::snprintf(buf, sizeof buf,
                  "B=%llu W=%d N=%d kind=%d cu=%d ok=%d H=%d pmax=%u bytes=%u replay=%d cap=%u calls=%u | no_gen=%d "
                  "group=%d bpc=%d chunk=%d grid=%d tail=%d lanes=%d steal=%d kimg=%d gsteal=%d fail_at=%d",
                  (unsigned long long)in.B, in.W, in.N, in.kind, in.n_cu, (int)in.counters_ok, in.H, in.pmax,
                  in.image_bytes, (int)in.replay, in.cap, in.n_calls, (int)in.knob.no_gen, in.knob.group, in.knob.bpc,
                  in.knob.chunk, in.knob.grid_cap, in.knob.tail, in.knob.lane_limit, (int)in.knob.steal,
                  (int)in.knob.kernel_image, in.grid_steal, ctx_fail_at);
    return buf;
}

// ------------------------------------------------------------------ the occupancy stand-in
struct Query {
    int mode, grp;
    uint32_t bytes, chunk;
    bool operator==(const Query& o) const { return mode == o.mode && grp == o.grp && bytes == o.bytes && chunk == o.chunk; }
};

// pbn_env.hip's env_lds_bytes as it was (modes: 2 and 4 cooperative draws, 3 group)
static uint32_t lds_ref(int W, uint32_t image_bytes, int fast, int grp, uint32_t chunk) {
    if (fast == 3) return image_bytes + 8u * (uint32_t)W * (256u / (uint32_t)grp);
    const uint32_t planes = image_bytes + 8u * (uint32_t)W * 256u;
    const bool coop = fast == 2 || fast == 4;
    return coop ? planes + 4u * (chunk * 64u * 2u + 64u + 64u * 16u) + (fast == 4 ? 16u : 0u) : planes;
}

// Workgroups per CU: falls as the workgroup's LDS rises (160 KiB per CU, at most 8), so the small chunk can fit
// more than the large one. Query number fail_at of a plan fails (-1: none).
struct FakeOccupancy {
    int W, fail_at;
    int n = 0;
    Query log[4] = {};
    int operator()(int mode, int grp, uint32_t image_bytes, uint32_t chunk, int* bpc) {
        const bool fails = n == fail_at;
        if (n < 4) log[n] = Query{mode, grp, image_bytes, chunk};
        ++n;
        if (fails) return 719;  // any hipError_t but hipSuccess
        const uint32_t per_cu = 160u * 1024u / lds_ref(W, image_bytes, mode, grp, chunk);
        *bpc = (int)(per_cu < 8u ? per_cu : 8u);
        return 0;
    }
};

// ------------------------------------------------------------------ the rule as it was
struct RefPlan : EnvPlan {
    int kernel = -1;  // EnvPlan::kernel, pbn_batch_info.env_kernel
};

static int grid_for_ref(uint64_t items, int n_cu, int bpc, int block) {
    uint64_t need = (items + block - 1) / block;
    uint64_t cap = (uint64_t)n_cu * (uint64_t)bpc;
    uint64_t g = need < cap ? need : cap;
    return (int)(g > 1 ? g : 1);
}

static RefPlan plan_ref(const EnvPlanIn& in, FakeOccupancy& occ) {
    RefPlan p;
    const EnvKnobs& k = in.knob;
    const int fast = in.counters_ok ? 1 : 0;  // pbn_envcfg::fast
    int mode = (fast && !in.replay && in.kind == 1 && in.pmax <= 16 && in.N <= 512 && !k.no_gen) ? 2 : fast;
    uint32_t erec_shift = 0;
    bool erec_fits = false;
    if (mode == 2) {
        const uint32_t nrec = (uint32_t)in.N * in.rs;
        erec_shift = in.off_rec + 16u * nrec - in.off_cubes;
        erec_fits = nrec <= 65535u && lds_ref(in.W, in.image_bytes + erec_shift, 2, 1, 32) <= 65536u;
    }
    int grp = 1;
    if (mode == 2 && in.N <= 256) {
        if (k.group)
            grp = k.group;
        else if (erec_fits && in.H <= 4)
            grp = 1;
        else
            grp = in.B * 8 <= (uint64_t)in.n_cu * 1536 ? 8 : 1;
        if (grp != 2 && grp != 4 && grp != 8) grp = 1;
        if (grp > 1) mode = 3;
    }
    if (mode == 2) {
        if (!erec_fits)
            mode = fast;
        else if (in.H <= 4)
            mode = 4;
        if (mode == 4 && lds_ref(in.W, in.image_bytes + erec_shift, 4, 1, 32) > 65536u) mode = fast;
    }
    const bool coop = mode == 2 || mode == 4;
    if (!coop) erec_shift = 0;
    const uint32_t img = in.image_bytes + erec_shift;
    p.host_image = coop && img % 16u == 0u && !k.kernel_image;
    int bpc = 1;
    uint32_t chunk = 32;
    if (coop) {
        int bpc_s = 1, bpc_l = 1;
        p.error = occ(mode, grp, img, 32, &bpc_s);
        const bool large_fits = lds_ref(in.W, img, mode, 1, 48) <= 65536u;
        if (large_fits && !p.error) p.error = occ(mode, grp, img, 48, &bpc_l);
        const uint64_t lanes_l = (uint64_t)in.n_cu * (uint64_t)bpc_l * 256;
        const bool throughput = in.n_calls >= 16u && in.B >= 4u * lanes_l && bpc_s > bpc_l;
        chunk = large_fits && !throughput ? 48 : 32;
        if (k.chunk == 32 || (k.chunk == 48 && large_fits)) chunk = (uint32_t)k.chunk;
        bpc = chunk == 48 ? bpc_l : bpc_s;
    } else {
        p.error = occ(mode, grp, img, 48, &bpc);  // max_blocks_env's default chunk
    }
    if (k.bpc) bpc = bpc < k.bpc ? bpc : k.bpc;
    p.tail_max = k.tail >= 0 ? (uint32_t)k.tail : 16u;
    p.lane_limit = 64u;
    if (mode == 4) {
        const uint64_t slots = (uint64_t)in.n_cu * (uint64_t)bpc * 4;
        if (k.lane_limit > 0)
            p.lane_limit = (uint32_t)k.lane_limit;
        else if (p.tail_max >= 1 && in.B <= 6 * slots)
            p.lane_limit = 1u;
    }
    p.grid = grid_for_ref(p.lane_limit < 64u ? (in.B * 64u + p.lane_limit - 1u) / p.lane_limit : in.B * (uint64_t)grp,
                          in.n_cu, bpc, 256);
    if (k.grid_cap) p.grid = k.grid_cap < in.n_cu * bpc ? k.grid_cap : in.n_cu * bpc;
    p.handoff = mode == 4 && k.steal && p.tail_max >= 1u && p.lane_limit >= 2u;
    p.gpool = p.handoff && (in.grid_steal > 0 || (in.grid_steal < 0 && (in.cap >= 16384u || in.n_calls > 1u)));
    p.mode = mode;
    p.grp = grp;
    p.erec_shift = erec_shift;
    p.chunk = chunk;
    p.bpc = bpc;
    p.kernel = in.replay ? (mode < 1 ? mode : 1) : mode;
    return p;
}

// ------------------------------------------------------------------ classes
enum {
    C_MODE0, C_MODE1, C_MODE2, C_MODE3, C_MODE4,
    C_COOP_32, C_COOP_48, C_TAIL_32, C_TAIL_48,
    C_THROUGHPUT_32,   // the small chunk chosen by the rule, not by the knob
    C_LARGE_NO_FIT,    // the large chunk's buffers do not fit: one occupancy query
    C_GRP2, C_GRP4, C_GRP8,
    C_LANES_1, C_LANES_64, C_LANES_OTHER,
    C_HANDOFF_ON, C_HANDOFF_OFF_TAIL,
    C_POOL_ON, C_POOL_OFF_HANDOFF,
    C_HOST_IMAGE, C_KERNEL_IMAGE,
    C_REPLAY, C_QUERY_FAILED, C_GRID_CAPPED_BY_RESIDENCY,
    C_COUNT
};
static const char* const class_name[C_COUNT] = {
    "mode 0", "mode 1", "mode 2", "mode 3", "mode 4", "coop chunk 32", "coop chunk 48", "tail chunk 32",
    "tail chunk 48", "throughput chunk 32", "large chunk does not fit", "group 2", "group 4", "group 8",
    "lane limit 1", "lane limit 64", "lane limit forced", "hand-off on", "hand-off off (tail kernel)", "pool on",
    "pool off (hand-off on)", "host image", "kernel image", "replay", "occupancy query failed",
    "grid = resident workgroups"};
static uint64_t seen[C_COUNT], plans;

// ------------------------------------------------------------------ one input
static void check(const EnvPlanIn& in, int fail_at) {
    FakeOccupancy occ_new{in.W, fail_at}, occ_ref{in.W, fail_at};
    const EnvPlan p = env_plan(in, occ_new);
    const RefPlan r = plan_ref(in, occ_ref);
    ctx_in = &in;
    ctx_fail_at = fail_at;
    REQUIRE(p.mode == r.mode);
    REQUIRE(p.grp == r.grp);
    REQUIRE(p.erec_shift == r.erec_shift);
    REQUIRE(p.chunk == r.chunk);
    REQUIRE(p.bpc == r.bpc);
    REQUIRE(p.lane_limit == r.lane_limit);
    REQUIRE(p.tail_max == r.tail_max);
    REQUIRE(p.grid == r.grid);
    REQUIRE(p.host_image == r.host_image);
    REQUIRE(p.handoff == r.handoff);
    REQUIRE(p.gpool == r.gpool);
    REQUIRE(p.error == r.error);
    REQUIRE(occ_new.n == occ_ref.n && occ_new.n >= 1 && occ_new.n <= 2);
    for (int q = 0; q < occ_new.n; ++q) REQUIRE(occ_new.log[q] == occ_ref.log[q]);
    // EnvPlan::kernel and launch_env_multi's clamp were the identity: a replay launch's mode is 0 or 1
    REQUIRE(r.kernel == r.mode);
    if (in.replay) REQUIRE(p.mode <= ENV_MODE_COUNTERS);
    REQUIRE(p.mode >= ENV_MODE_CUBES && p.mode <= ENV_MODE_TAIL);
    REQUIRE(env_lds_bytes(in.W, in.image_bytes + p.erec_shift, p.mode, p.grp, p.chunk) ==
            lds_ref(in.W, in.image_bytes + p.erec_shift, p.mode, p.grp, p.chunk));
    ++plans;
    if (p.error) {
        ++seen[C_QUERY_FAILED];
        return;  // no launch: nothing else of the plan is used
    }
    REQUIRE(env_lds_bytes(in.W, in.image_bytes + p.erec_shift, p.mode, p.grp, p.chunk) <= ENV_LDS_MAX);
    REQUIRE(p.grid >= 1);
    REQUIRE(p.grid <= in.n_cu * 8);
    if (p.gpool) REQUIRE(p.handoff);
    if (p.handoff) REQUIRE(p.mode == ENV_MODE_TAIL);
    if (p.mode == ENV_MODE_GROUP) REQUIRE(p.grp == 2 || p.grp == 4 || p.grp == 8); else REQUIRE(p.grp == 1);
    const bool coop = p.mode == ENV_MODE_COOP || p.mode == ENV_MODE_TAIL;
    if (!coop) REQUIRE(p.erec_shift == 0 && !p.host_image);
    if (coop) REQUIRE(p.chunk == ENV_CHUNK_SMALL || p.chunk == ENV_CHUNK_LARGE);

    ++seen[C_MODE0 + p.mode];
    if (p.mode == ENV_MODE_COOP) ++seen[p.chunk == ENV_CHUNK_SMALL ? C_COOP_32 : C_COOP_48];
    if (p.mode == ENV_MODE_TAIL) ++seen[p.chunk == ENV_CHUNK_SMALL ? C_TAIL_32 : C_TAIL_48];
    if (coop && occ_new.n == 1) ++seen[C_LARGE_NO_FIT];
    if (coop && occ_new.n == 2 && p.chunk == ENV_CHUNK_SMALL && in.knob.chunk == 0) ++seen[C_THROUGHPUT_32];
    if (p.grp == 2) ++seen[C_GRP2];
    if (p.grp == 4) ++seen[C_GRP4];
    if (p.grp == 8) ++seen[C_GRP8];
    ++seen[p.lane_limit == 1 ? C_LANES_1 : p.lane_limit == 64 ? C_LANES_64 : C_LANES_OTHER];
    if (p.mode == ENV_MODE_TAIL) ++seen[p.handoff ? C_HANDOFF_ON : C_HANDOFF_OFF_TAIL];
    if (p.handoff) ++seen[p.gpool ? C_POOL_ON : C_POOL_OFF_HANDOFF];
    if (coop) ++seen[p.host_image ? C_HOST_IMAGE : C_KERNEL_IMAGE];
    if (in.replay) ++seen[C_REPLAY];
    if (p.grid == in.n_cu * p.bpc) ++seen[C_GRID_CAPPED_BY_RESIDENCY];
}

// ------------------------------------------------------------------ the grid
// A network's layout as the packers fix it (build_predictor_image / build_table_image, pbn_image.cpp): N nodes in W
// words, kind 1 predictor mix / 2 truth tables, pmax record slots per node, the image's bytes (where an env config
// puts its cubes), the records' offset, and thr32_layout's record stride rs.
struct Net {
    const char* name;
    int N, W, kind;
    uint32_t pmax, bytes, off_rec, rs;
};
static const Net nets[] = {
    {"bittner28", 28, 1, 1, 15, 6496, 3136, 17},
    {"bittner70", 70, 2, 1, 5, 5040, 2240, 5},
    {"bittner100", 100, 2, 1, 5, 7200, 3200, 5},
    {"bittner199", 199, 4, 1, 5, 14336, 6368, 5},
    {"tt200", 200, 4, 2, 0, 28800, 1600, 1},
    // synthetic predictor mixes: more than 16 predictors at a node (no cooperative draws);
    {"syn40_p20", 40, 1, 1, 20, 12800, 6400, 21},
    // 16-B env records that do not fit a workgroup's 64 KiB, with and without group mode's N <= 256;
    {"syn256_p9", 256, 4, 1, 9, 34816, 16384, 9},
    {"syn500_p4", 500, 8, 1, 4, 32000, 16000, 5},
    // and records that fit with the small chunk's draw buffers only
    {"syn240_p5", 240, 4, 1, 5, 17280, 7680, 5},
};

static uint32_t align16(uint32_t x) { return (x + 15u) & ~15u; }

// build_envcfg_image's offsets: the cubes [H][2][W] after the network's image, the target, the counter deltas
static EnvPlanIn config(const Net& n, int H, bool counters_ok) {
    EnvPlanIn in;
    in.W = n.W;
    in.N = n.N;
    in.kind = n.kind;
    in.counters_ok = counters_ok;
    in.H = H;
    in.pmax = n.pmax;
    in.off_rec = n.off_rec;
    in.off_cubes = n.bytes;
    in.rs = n.rs;
    const uint32_t off_target = align16(in.off_cubes + 16u * (uint32_t)n.W * (uint32_t)H);
    const uint32_t off_ndelta = align16(off_target + 16u * (uint32_t)n.W);
    in.image_bytes = align16(off_ndelta + 8u * (uint32_t)n.N);
    return in;
}

// every knob at its default, then each at each value the tests and tools force (and one outside them)
static std::vector<std::function<void(EnvPlanIn&)>> knob_variants() {
    std::vector<std::function<void(EnvPlanIn&)>> v{[](EnvPlanIn&) {}};
    auto with = [&](auto set) { v.push_back(set); };
    with([](EnvPlanIn& in) { in.knob.no_gen = true; });
    for (int g : {1, 2, 3, 4, 8}) with([g](EnvPlanIn& in) { in.knob.group = g; });
    for (int c : {1, 2}) with([c](EnvPlanIn& in) { in.knob.bpc = c; });
    for (int c : {32, 40, 48}) with([c](EnvPlanIn& in) { in.knob.chunk = c; });
    for (int g : {1, 4, 32, 100000}) with([g](EnvPlanIn& in) { in.knob.grid_cap = g; });
    for (int t : {0, 3, 64}) with([t](EnvPlanIn& in) { in.knob.tail = t; });
    for (int l : {1, 2, 16, 64}) with([l](EnvPlanIn& in) { in.knob.lane_limit = l; });
    with([](EnvPlanIn& in) { in.knob.steal = false; });
    with([](EnvPlanIn& in) { in.knob.kernel_image = true; });
    for (int s : {0, 1}) with([s](EnvPlanIn& in) { in.grid_steal = s; });
    // the hand-off needs two or more lanes taking envs: its switches with the lane limit forced, as the tests set them
    for (int l : {2, 64})
        for (int s : {-1, 0, 1})
            for (int steal : {0, 1})
                for (int t : {-1, 0})
                    with([=](EnvPlanIn& in) {
                        in.knob.lane_limit = l;
                        in.grid_steal = s;
                        in.knob.steal = steal != 0;
                        in.knob.tail = t;
                    });
    return v;
}

int main() {
    const int H_values[] = {1, 4, 5, 8, 9, 12};
    const uint32_t call_counts[] = {1, 15, 16, 100}, caps[] = {16383, 16384};  // either side of GPOOL_MIN_CAP
    const auto variants = knob_variants();
    const int n_cu = 256;
    for (const Net& n : nets)
        for (int H : H_values)
            for (int ok = 0; ok <= 1; ++ok) {
                if (ok && H > 8) continue;  // build_envcfg_image: the byte counters hold 8 cubes
                const EnvPlanIn cfg = config(n, H, ok != 0);
                // batch sizes: the group-size crossover (8 B = 1536 n_cu), one lane per wave up to 6 envs per
                // wave slot (4 n_cu bpc slots) and the throughput rule's 4 envs per lane of the large chunk's
                // grid (256 n_cu bpc lanes), for every bpc the stand-in gives, each with its neighbours
                std::vector<uint64_t> Bs{1, 64, 131072, 1ull << 20};
                auto around = [&](uint64_t T) {
                    for (uint64_t B = T - 1; B <= T + 1; ++B) Bs.push_back(B);
                };
                around((uint64_t)n_cu * 192);
                for (uint64_t bpc = 1; bpc <= 8; ++bpc) {
                    around(6 * 4 * (uint64_t)n_cu * bpc);
                    around(4 * 256 * (uint64_t)n_cu * bpc);
                }
                for (uint64_t B : Bs)
                    for (uint32_t n_calls : call_counts)
                        for (uint32_t cap : caps)
                            for (int replay = 0; replay <= 1; ++replay) {
                                EnvPlanIn base = cfg;
                                base.B = B;
                                base.n_cu = n_cu;
                                base.n_calls = n_calls;
                                base.cap = cap;
                                base.replay = replay != 0;
                                for (const auto& set : variants) {
                                    EnvPlanIn in = base;
                                    set(in);
                                    check(in, -1);
                                }
                                check(base, 0);  // the first occupancy query fails, or the second
                                check(base, 1);
                            }
            }
    ctx_in = nullptr;
    for (int c = 0; c < C_COUNT; ++c) {
        ctx_text = class_name[c];  // a class no plan fell into
        REQUIRE(seen[c] > 0);
    }
    std::printf("env_plan_check: %llu plans;", (unsigned long long)plans);
    for (int c = 0; c < C_COUNT; ++c) std::printf(" %s: %llu;", class_name[c], (unsigned long long)seen[c]);
    std::puts("\nenv_plan_check ok");
    return 0;
}
