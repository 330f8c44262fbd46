// step_plan_check.cpp -- step mode's plan (csrc/pbn_step_plan.hpp) on the CPU.
//
// Built by `make stepplancheck` with ASan + UBSan; no HIP header, no library, no GPU. The references below restate
// the rules as pbn_batch_create and pbn_step held them inline before the header existed, with the constants
// written out, so a change to the header that changes what a batch or a call does fails here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pbn_step_plan.hpp"

using namespace pbn;

#define REQUIRE(cond)                                                                             \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            std::fprintf(stderr, "step_plan_check: %s failed (%s) at line %d\n", #cond, ctx, __LINE__); \
            std::exit(1);                                                                         \
        }                                                                                         \
    } while (0)

static char ctx[256] = "";

// ------------------------------------------------------------------ decomposition
// pbn_step's greedy loop, verbatim (t: updates queued so far)
static StepPow2 greedy(uint32_t n_updates) {
    StepPow2 d;
    uint32_t t = 0;
    for (int j = 0; j < STEP_GRAPH_SIZES; ++j) {
        const uint32_t K = STEP_GRAPH_K >> j;
        while (n_updates - t >= K && (j == 0 || n_updates - t < 2 * K)) {
            d.replays[j]++;
            t += K;
        }
    }
    d.plain = n_updates - t;
    return d;
}

static void check_pow2(uint32_t n) {
    std::snprintf(ctx, sizeof ctx, "n=%u", n);
    const StepPow2 d = step_pow2(n), ref = greedy(n);
    uint32_t covered = 0, replays = 0;
    for (int j = 0; j < STEP_GRAPH_SIZES; ++j) {
        REQUIRE(d.replays[j] == ref.replays[j]);
        covered += d.replays[j] * (STEP_GRAPH_K >> j);
        replays += d.replays[j];
    }
    REQUIRE(d.plain == ref.plain);
    REQUIRE(covered + d.plain == n);
    if (n >= 2) REQUIRE(d.plain == (n & 1u));
    REQUIRE(replays == n / 64 + (uint32_t)__builtin_popcount((n % 64) >> 1));
}

// ------------------------------------------------------------------ shape
// pbn_batch_create's rules (with step_fill_envs and step_chains_for), constants written out
static StepShape shape_ref(uint64_t B, int W, int n_cu, int step_block, int step_chains, int step_graph,
                           int envs_per_thread) {
    StepShape s;
    const uint64_t fill = (uint64_t)n_cu * 1024u * (uint64_t)envs_per_thread;
    if (step_block)
        s.block = step_block;
    else
        s.block = B >= fill ? 1024 : 256;
    int want = step_chains;
    if (!want) want = s.block == 1024 && B >= 2 * fill ? 2 : 1;
    s.chains = chain_split(B, want, s.block, s.sl);
    s.min_updates = step_chains ? 2u : 128u;
    if (step_graph >= 0)
        s.graphs_off = step_graph == 0;
    else
        s.graphs_off = B * (uint64_t)W >= (s.chains > 1 ? 1ull << 24 : 1ull << 20);
    return s;
}

static void require_same(const StepShape& a, const StepShape& b) {
    REQUIRE(a.block == b.block);
    REQUIRE(a.chains == b.chains);
    REQUIRE(a.min_updates == b.min_updates);
    REQUIRE(a.graphs_off == b.graphs_off);
    for (int c = 0; c < STEP_CHAINS_MAX; ++c) REQUIRE(a.sl[c].off == b.sl[c].off && a.sl[c].len == b.sl[c].len);
}

static void check_shapes() {
    const int n_cu = 256;
    // the knob values the tests set (0 / -1: unset)
    const int blocks[] = {0, 256, 1024}, chains[] = {0, 1, 2, 4}, graphs[] = {-1, 0, 1}, per_thread[] = {1, 2, 4, 8};
    for (int W = 1; W <= 8; ++W)
        for (int sb : blocks)
            for (int sc : chains)
                for (int sg : graphs)
                    for (int K : per_thread) {
                        const uint64_t fill = (uint64_t)n_cu * 1024u * (uint64_t)K;
                        // the first batch size at or past each threshold: block 1024, two chains, graphs off of
                        // one chain, graphs off of a batch with chains
                        const uint64_t at[] = {fill, 2 * fill, ((1ull << 20) + W - 1) / W, ((1ull << 24) + W - 1) / W};
                        for (uint64_t T : at)
                            for (uint64_t B = T - 1; B <= T + 1; ++B) {
                                std::snprintf(ctx, sizeof ctx, "B=%llu W=%d block=%d chains=%d graph=%d K=%d",
                                              (unsigned long long)B, W, sb, sc, sg, K);
                                require_same(step_shape(B, W, n_cu, sb, sc, sg, K), shape_ref(B, W, n_cu, sb, sc, sg, K));
                            }
                    }
    {  // the bench shape: 1M Bittner-200 envs
        std::snprintf(ctx, sizeof ctx, "1M x W=4");
        const StepShape s = step_shape(1ull << 20, 4, n_cu, 0, 0, -1, 2);
        REQUIRE(s.block == 1024 && s.chains == 2 && !s.graphs_off && s.min_updates == 128);
        REQUIRE(s.sl[0].len == (1ull << 19) && s.sl[1].off == (1ull << 19) && s.sl[1].len == (1ull << 19));
    }
    {  // BASELINE config 2: 65,536 Bittner-28 envs
        std::snprintf(ctx, sizeof ctx, "65536 x W=1");
        const StepShape s = step_shape(65536, 1, n_cu, 0, 0, -1, 2);
        REQUIRE(s.block == 256 && s.chains == 1 && !s.graphs_off);
        REQUIRE(s.sl[0].off == 0 && s.sl[0].len == 65536);
    }
    {  // either side of 2^24 words with chains, and of 2^20 without
        std::snprintf(ctx, sizeof ctx, "graph thresholds");
        REQUIRE(!step_shape((1ull << 22) - 1, 4, n_cu, 0, 0, -1, 2).graphs_off);
        REQUIRE(step_shape(1ull << 22, 4, n_cu, 0, 0, -1, 2).graphs_off);
        REQUIRE(!step_shape((1ull << 18) - 1, 4, n_cu, 0, 0, -1, 2).graphs_off);
        REQUIRE(step_shape(1ull << 18, 4, n_cu, 0, 0, -1, 2).graphs_off);
    }
}

// ------------------------------------------------------------------ call plan
static void check_calls() {
    const int n_cu = 256;
    // one chain; two chains by size (split from 128 updates on); forced chains (every run split); each with graphs on / off
    const StepShape shapes[] = {
        step_shape(4099, 4, n_cu, 0, 0, -1, 2), step_shape(4099, 4, n_cu, 0, 0, 0, 2),
        step_shape(1ull << 20, 4, n_cu, 0, 0, -1, 2), step_shape(1ull << 20, 4, n_cu, 0, 0, 0, 2),
        step_shape(4099, 4, n_cu, 0, 2, 1, 2), step_shape(4099, 4, n_cu, 0, 4, 0, 2),
    };
    const uint32_t lengths[] = {0, 1, 2, 127, 128, 129};
    for (const StepShape& s : shapes)
        for (uint32_t n : lengths)
            for (int mode = 0; mode <= 2; ++mode)
                for (int cap = 0; cap <= 1; ++cap)
                    for (int null_stream = 0; null_stream <= 1; ++null_stream) {
                        std::snprintf(ctx, sizeof ctx, "chains=%d min=%u off=%d n=%u mode=%d cap=%d null=%d", s.chains,
                                      s.min_updates, (int)s.graphs_off, n, mode, cap, null_stream);
                        const StepCall c = step_call(s, n, mode, cap != 0, null_stream != 0);
                        // pbn_step's booleans, as it computed them
                        const bool run = !cap && mode != 1 && n >= 2;
                        const bool chained = run && s.chains > 1 && n >= s.min_updates;
                        const bool use_graphs = run && !s.graphs_off && (s.chains == 1 || chained);
                        REQUIRE(c.run == run && c.chained == chained && c.graphs == use_graphs);
                        REQUIRE(c.capture == (use_graphs && !null_stream));  // the null stream cannot capture
                        // ... and what they amount to
                        if (n < 2 || mode == 1 || cap) REQUIRE(!c.run);
                        if (!c.run) REQUIRE(!c.chained && !c.graphs);
                        if (c.chained) REQUIRE(s.chains > 1 && n >= s.min_updates);
                        if (s.chains > 1 && !c.chained) REQUIRE(!c.graphs);  // its graphs cover the chains' slices
                        if (s.graphs_off) REQUIRE(!c.graphs);
                        if (c.capture) REQUIRE(c.graphs);
                    }
    std::snprintf(ctx, sizeof ctx, "default two chains");
    const StepShape two = shapes[2];
    REQUIRE(two.chains == 2 && two.min_updates == 128);
    REQUIRE(!step_call(two, 127, 0, false, false).chained && !step_call(two, 127, 0, false, false).graphs);
    REQUIRE(step_call(two, 128, 0, false, false).chained && step_call(two, 128, 2, false, false).graphs);
    std::snprintf(ctx, sizeof ctx, "forced two chains");
    REQUIRE(shapes[4].chains == 2 && step_call(shapes[4], 2, 0, false, false).chained);
}

int main() {
    for (uint32_t n = 0; n <= 5000; ++n) check_pow2(n);
    std::snprintf(ctx, sizeof ctx, "exact lengths");
    REQUIRE(!step_exact_fits(0) && !step_exact_fits(1) && step_exact_fits(2) && step_exact_fits(64) && !step_exact_fits(65));
    check_shapes();
    check_calls();
    std::puts("step_plan_check ok");
    return 0;
}
