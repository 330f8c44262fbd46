// control_plan_check.cpp -- the launch shape of the control kernels (csrc/pbn_control_plan.hpp) on the CPU.
//
// Built by `make controlplancheck` with ASan + UBSan; no HIP header, no library, no GPU. For every node count 1 .. 512,
// state counts either side of a workgroup's rows, resident counts and grid caps: every field of the plan against a
// restatement of the rule; then the walk the kernels make under that plan, replayed lane by lane -- every (row, cell)
// is visited exactly once and nothing outside [0, S) x [0, N) is touched, whatever the grid; and the order in which a
// row's cells are combined (lane-local, then the xor butterfly) is the same for every grid.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pbn_control_plan.hpp"

using namespace pbn;

#define REQUIRE(cond)                                                                                              \
    do {                                                                                                           \
        if (!(cond)) {                                                                                             \
            std::fprintf(stderr, "control_plan_check: %s failed (S=%llu N=%u n_cu=%d bpc=%d cap=%d) at line %d\n", \
                         #cond, (unsigned long long)S, N, n_cu, bpc, cap, __LINE__);                               \
            std::exit(1);                                                                                          \
        }                                                                                                          \
    } while (0)

// the rule, restated: G by doubling is "the smallest power of two >= N, at most 64"
static uint32_t group_of(uint32_t N) {
    for (uint32_t g : {1u, 2u, 4u, 8u, 16u, 32u}) {
        if (g >= N) return g;
    }
    return 64u;
}

static void check_plan(uint64_t S, uint32_t N, int n_cu, int bpc, int cap) {
    const ControlPlan p = control_plan(S, N, n_cu, bpc, cap);
    const uint32_t G = group_of(N);
    REQUIRE(p.G == G && control_group(N) == G);
    REQUIRE(G >= 1 && G <= 64 && (G & (G - 1)) == 0);
    REQUIRE(G >= N || G == 64);
    REQUIRE(G == 1 || G / 2 < N);  // the smallest such power
    REQUIRE(p.rows_per_wave * G == 64 && p.rows_per_block * G == CONTROL_BLOCK);
    REQUIRE((uint64_t)p.cells_per_lane * G >= N && (uint64_t)(p.cells_per_lane - 1) * G < N);
    REQUIRE(p.rows_unrolled == (N <= 64 ? CONTROL_UNROLL : 1u) && (p.rows_unrolled == 1 || p.cells_per_lane == 1));
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    const uint64_t need = S / per_trip + (S % per_trip ? 1 : 0);
    const uint64_t resident = (uint64_t)(n_cu > 0 ? n_cu : 1) * (uint64_t)(bpc > 0 ? bpc : 1);
    uint64_t want = need;
    if (want > resident) want = resident;
    if (cap > 0 && want > (uint64_t)cap) want = (uint64_t)cap;
    if (want < 1) want = 1;
    REQUIRE(p.grid >= 1 && (uint64_t)p.grid == want);
}

// The kernels' walk: workgroup b, thread t -> lane j = t % G of the group of row r = t / G; per trip the rows base +
// k * RPB + r, k < rows_unrolled, for base = b * RPB * rows_unrolled, += grid * RPB * rows_unrolled while base < S; cells
// j, j + G, ... < N. Returns, per row, the order of combination as text.
static std::vector<std::string> walk(uint64_t S, uint32_t N, int n_cu, int bpc, int cap) {
    const ControlPlan p = control_plan(S, N, n_cu, bpc, cap);
    std::vector<uint32_t> seen(S * N, 0);
    std::vector<std::string> order(S);
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    for (int b = 0; b < p.grid; ++b)
        for (uint64_t base = (uint64_t)b * per_trip; base < S; base += (uint64_t)p.grid * per_trip)
            for (uint32_t kr = 0; kr < per_trip; ++kr) {  // kr = k * RPB + r
                const uint64_t row = base + kr;
                if (row >= S) continue;  // the lanes stay for the shuffles and touch nothing
                std::vector<std::string> lane(p.G);
                for (uint32_t j = 0; j < p.G; ++j) {
                    uint32_t n = 0;
                    for (uint64_t i = j; i < N; i += p.G, ++n) {
                        REQUIRE(row * N + i < S * N);
                        seen[row * N + i]++;
                        lane[j] += (n ? "+" : "") + std::to_string(i);
                    }
                    REQUIRE(n <= p.cells_per_lane);
                    if (!n) lane[j] = "0";
                }
                for (uint32_t d = p.G / 2; d >= 1; d >>= 1) {
                    std::vector<std::string> next(p.G);
                    for (uint32_t j = 0; j < p.G; ++j) {
                        const uint32_t lo = j < (j ^ d) ? j : (j ^ d), hi = lo ^ d;  // a + b is b + a: one spelling
                        next[j] = "(" + lane[lo] + ")+(" + lane[hi] + ")";
                    }
                    lane = next;
                }
                for (uint32_t j = 1; j < p.G; ++j) REQUIRE(lane[j] == lane[0]);  // every lane holds the same sum
                REQUIRE(order[row].empty());
                order[row] = lane[0];
            }
    for (uint64_t c = 0; c < S * N; ++c) REQUIRE(seen[c] == 1);
    for (uint64_t s = 1; s < S; ++s) REQUIRE(order[s] == order[0]);  // a function of (N, G), not of the row
    return order;
}

int main() {
    const int cus[] = {1, 7, 256}, bpcs[] = {0, 1, 8}, caps[] = {0, 1, 3, 100000};
    for (uint32_t N = 1; N <= CONTROL_MAX_NODES; ++N) {
        const uint32_t rpb = CONTROL_BLOCK / group_of(N);
        const uint64_t sizes[] = {1, rpb - 1 ? rpb - 1 : 1, rpb, rpb + 1, 53, 1000, 3 * rpb + 1, 1ull << 20, 1ull << 24};
        for (uint64_t S : sizes)
            for (int n_cu : cus)
                for (int bpc : bpcs)
                    for (int cap : caps) check_plan(S, N, n_cu, bpc, cap);
    }
    // the walk, on sizes small enough to replay: the same order of combination under every grid
    const uint32_t nodes[] = {1, 2, 3, 8, 9, 10, 16, 28, 33, 64, 65, 100, 257};
    for (uint32_t N : nodes) {
        const uint32_t rpb = CONTROL_BLOCK / group_of(N);
        const uint64_t sizes[] = {1, 2, rpb, rpb + 1, 2 * rpb + 3, 4 * rpb, 4 * rpb + 1, 9 * rpb + 5};
        for (uint64_t S : sizes) {
            const std::vector<std::string> one = walk(S, N, 256, 8, 1);
            for (int cap : {0, 2, 3}) {
                const int n_cu = 256, bpc = 8;
                REQUIRE(walk(S, N, n_cu, bpc, cap) == one);
            }
            const int n_cu = 1, bpc = 1, cap = 0;
            REQUIRE(walk(S, N, n_cu, bpc, cap) == one);
        }
    }
    {  // by hand: N = 10 -> 16 lanes, 4 rows per wave, 16 per workgroup, 4 of those per trip; 1,024 rows are 16 workgroups
        const uint64_t S = 1024;
        const uint32_t N = 10;
        const int n_cu = 256, bpc = 8, cap = 0;
        const ControlPlan p = control_plan(S, N, n_cu, bpc, cap);
        REQUIRE(p.G == 16 && p.rows_per_wave == 4 && p.rows_per_block == 16 && p.cells_per_lane == 1);
        REQUIRE(p.rows_unrolled == 4 && p.grid == 16);
        const ControlPlan q = control_plan(1ull << 20, 21, 256, 8, 0);
        REQUIRE(q.G == 32 && q.rows_per_block == 8 && q.grid == 2048);
        const ControlPlan w = control_plan(1024, 257, 256, 8, 3);
        REQUIRE(w.G == 64 && w.rows_per_block == 4 && w.cells_per_lane == 5 && w.rows_unrolled == 1 && w.grid == 3);
    }
    std::puts("control_plan_check ok");
    return 0;
}
