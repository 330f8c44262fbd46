// absorb_plan_check.cpp -- the launch shape of k_stg_absorb (csrc/pbn_absorb_plan.hpp) on the CPU.
//
// Built by `make absorbplancheck` with ASan + UBSan; no HIP header, no library, no GPU. For every node count 1 .. 512,
// every column count 1 .. 8, state counts either side of a trip's rows, resident counts and grid caps: every field of
// the plan against a restatement of the rule. Then the walk the kernels make under that plan, replayed lane by lane on
// arrays of the real sizes: every row is visited exactly once, every index into mass / succ ([S][N]), label ([S]) and x /
// out ([S][ld]) is in range (the arrays are std::vectors of exactly that size: ASan watches them), columns [n_cols, ld)
// of out are never written, and a row past the end touches only cells of a row that exists.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pbn_absorb_plan.hpp"

using namespace pbn;

#define REQUIRE(cond)                                                                                                 \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            std::fprintf(stderr, "absorb_plan_check: %s failed (S=%llu N=%u C=%u n_cu=%d bpc=%d cap=%d) at line %d\n", \
                         #cond, (unsigned long long)S, N, C, n_cu, bpc, cap, __LINE__);                               \
            std::exit(1);                                                                                             \
        }                                                                                                             \
    } while (0)

// the rules, restated
static uint32_t group_of(uint32_t N) {
    for (uint32_t g : {1u, 2u, 4u, 8u, 16u, 32u}) {
        if (g >= N) return g;
    }
    return 64u;
}

static uint32_t tile_of(uint32_t C) { return C == 1 ? 1u : C == 2 ? 2u : C <= 4 ? 4u : 8u; }

static uint32_t rows_of(uint32_t tile, uint32_t N) {
    if (N > 64) return 1;
    return tile == 1 ? 4u : tile == 2 ? 4u : tile == 4 ? 2u : 1u;
}

static void check_plan(uint64_t S, uint32_t N, uint32_t C, int n_cu, int bpc, int cap) {
    const AbsorbPlan p = absorb_plan(S, N, C, n_cu, bpc, cap);
    const ControlPlan q = control_plan(S, N, n_cu, bpc, cap);
    const uint32_t G = group_of(N);
    REQUIRE(p.G == G && p.G == q.G);  // k_stg_expect's row mapping
    REQUIRE(p.rows_per_wave == q.rows_per_wave && p.rows_per_block == q.rows_per_block);
    REQUIRE(p.cells_per_lane == q.cells_per_lane);
    REQUIRE(p.rows_per_wave * G == 64 && p.rows_per_block * G == CONTROL_BLOCK);
    REQUIRE((uint64_t)p.cells_per_lane * G >= N && (uint64_t)(p.cells_per_lane - 1) * G < N);
    REQUIRE(p.col_tile == tile_of(C) && p.col_tile >= C && p.col_tile <= ABSORB_MAX_COLS);
    REQUIRE(p.col_tile == 1 || p.col_tile / 2 < C);  // the smallest such tile
    REQUIRE(p.rows_unrolled == rows_of(p.col_tile, N));
    REQUIRE(p.rows_unrolled == 1 || p.cells_per_lane == 1);
    REQUIRE(p.rows_unrolled * p.col_tile <= ABSORB_ROW_GATHERS || p.rows_unrolled == 1);
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    const uint64_t need = S / per_trip + (S % per_trip ? 1 : 0);
    const uint64_t resident = (uint64_t)(n_cu > 0 ? n_cu : 1) * (uint64_t)(bpc > 0 ? bpc : 1);
    uint64_t want = need;
    if (want > resident) want = resident;
    if (cap > 0 && want > (uint64_t)cap) want = (uint64_t)cap;
    if (want < 1) want = 1;
    REQUIRE(p.grid >= 1 && (uint64_t)p.grid == want);
}

// The kernels' walk: workgroup b, thread t -> lane j = t % G of the group of row r = t / G; per trip the rows base + k *
// RPB + r, k < rows_unrolled, for base = b * RPB * rows_unrolled, += grid * RPB * rows_unrolled while base < S. One-cell
// kernels clamp a row past the end to S - 1 and a lane past N to cell 0 and read there; the looping kernel reads
// nothing for such a row. Lane 0 of a live row writes columns [0, C) of out.
static void walk(uint64_t S, uint32_t N, uint32_t C, uint64_t ld, int n_cu, int bpc, int cap) {
    const AbsorbPlan p = absorb_plan(S, N, C, n_cu, bpc, cap);
    std::vector<uint8_t> cells(S * N, 0), label(S, 0), x(S * ld, 0), out(S * ld, 0);
    std::vector<uint32_t> rows(S, 0);
    std::vector<int32_t> succ(S * N);
    for (uint64_t c = 0; c < S * N; ++c) succ[c] = (int32_t)((c * 2654435761ull) % (S + 1)) - (c % 7 == 0);  // -1 and S: no row
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    const bool one_cell = p.cells_per_lane == 1;
    uint64_t trips_of_first = 0;
    for (int b = 0; b < p.grid; ++b) {
        uint64_t trips = 0;
        for (uint64_t base = (uint64_t)b * per_trip; base < S; base += (uint64_t)p.grid * per_trip, ++trips)
            for (uint32_t kr = 0; kr < per_trip; ++kr) {  // kr = k * RPB + r
                const uint64_t want = base + kr;
                const bool live = want < S;
                if (!live && !one_cell) continue;  // the lanes stay for the shuffles and touch nothing
                const uint64_t row = live ? want : S - 1;
                for (uint32_t j = 0; j < p.G; ++j) {
                    uint32_t n = 0;
                    for (uint64_t i = one_cell ? (j < N ? j : 0) : j; i < N; i += p.G, ++n) {
                        cells.at(row * N + i) += live && (!one_cell || j < N);
                        const uint64_t t0 = (uint64_t)(uint32_t)succ.at(row * N + i);
                        const uint64_t t = t0 < S ? t0 : row;
                        label.at(row) |= 1;
                        for (uint32_t c = 0; c < C; ++c) {
                            x.at(row * ld + c) |= 1;
                            x.at(t * ld + c) |= 1;
                        }
                        if (one_cell) break;
                    }
                    REQUIRE(n <= p.cells_per_lane);
                }
                if (live) {
                    rows[row]++;
                    for (uint32_t c = 0; c < C; ++c) out.at(row * ld + c)++;
                }
            }
        if (b == 0) trips_of_first = trips;
        REQUIRE(trips <= trips_of_first && trips + 1 >= trips_of_first);  // per workgroup; uniform within one by construction
    }
    for (uint64_t s = 0; s < S; ++s) {
        REQUIRE(rows[s] == 1);
        for (uint64_t c = 0; c < ld; ++c) REQUIRE(out[s * ld + c] == (c < C ? 1 : 0));
        for (uint32_t i = 0; i < N; ++i) REQUIRE(cells[s * N + i] == 1);
    }
}

int main() {
    const int cus[] = {1, 7, 256}, bpcs[] = {0, 1, 8}, caps[] = {0, 1, 3, 100000};
    for (uint32_t N = 1; N <= CONTROL_MAX_NODES; ++N)
        for (uint32_t C = 1; C <= ABSORB_MAX_COLS; ++C) {
            const uint32_t per = CONTROL_BLOCK / group_of(N) * rows_of(tile_of(C), N);
            const uint64_t sizes[] = {1, per - 1 ? per - 1 : 1, per, per + 1, 53, 3 * per + 1, 1ull << 20, 1ull << 24};
            for (uint64_t S : sizes)
                for (int n_cu : cus)
                    for (int bpc : bpcs)
                        for (int cap : caps) check_plan(S, N, C, n_cu, bpc, cap);
        }
    // the walk, on sizes small enough to replay, with spare columns and without
    const uint32_t nodes[] = {1, 2, 3, 6, 8, 10, 16, 28, 33, 64, 65, 100, 257};
    for (uint32_t N : nodes)
        for (uint32_t C = 1; C <= ABSORB_MAX_COLS; ++C) {
            const uint32_t per = CONTROL_BLOCK / group_of(N) * rows_of(tile_of(C), N);
            const uint64_t sizes[] = {1, 2, per - 1 ? per - 1 : 1, per, per + 1, 2 * per + 3, 5 * per + 1};
            for (uint64_t S : sizes)
                for (uint64_t ld : {(uint64_t)C, (uint64_t)C + 2}) {
                    walk(S, N, C, ld, 256, 8, 0);
                    walk(S, N, C, ld, 256, 8, 3);
                    walk(S, N, C, ld, 1, 1, 0);
                }
        }
    {  // by hand: the benchmark's shape, 2^20 rows of 21 nodes -> 32 lanes, 8 rows per workgroup
        const uint64_t S = 1ull << 20;
        const uint32_t N = 21;
        uint32_t C = 5;
        const int n_cu = 256, bpc = 8, cap = 0;
        const AbsorbPlan p = absorb_plan(S, N, C, n_cu, bpc, cap);
        REQUIRE(p.G == 32 && p.rows_per_block == 8 && p.col_tile == 8 && p.rows_unrolled == 1 && p.grid == 2048);
        C = 2;
        const AbsorbPlan q = absorb_plan(S, N, C, n_cu, bpc, cap);
        REQUIRE(q.col_tile == 2 && q.rows_unrolled == 4 && q.grid == 2048);
        C = 3;
        const AbsorbPlan w = absorb_plan(1024, 257, C, 256, 8, 3);
        REQUIRE(w.G == 64 && w.cells_per_lane == 5 && w.col_tile == 4 && w.rows_unrolled == 1 && w.grid == 3);
    }
    std::puts("absorb_plan_check ok");
    return 0;
}
