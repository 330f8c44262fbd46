// pbn_absorb.hip -- absorption over a transition graph: one Jacobi sweep of the first-hit recursion on
// the dense arrays of pbn_stg.hip, for up to eight columns at once, holding the labelled rows in the same pass.
//
// Reference semantics implemented (file:line in the reference):
//   k_stg_absorb  n sweeps are the exact law of "update until the state is in an attractor, at most update_cap times"
//                 (PBNTargetMultiEnv.step pbn_target_multi.py:133-146) from every row of the set at once: the
//                 probability of having hit each labelled class, of not having hit any, and the expected number of
//                 updates. The reference has no such code: it samples the loop, one env at a time.
// Launch shape: pbn_absorb_plan.hpp. The row mapping and the order in which a row's cells are combined are
// k_stg_expect's (pbn_control.hip).
#include <hip/hip_runtime.h>

#include "pbn_absorb_plan.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"

namespace pbn {

static_assert(CONTROL_BLOCK == (uint32_t)BLOCK && ABSORB_MAX_COLS == (uint32_t)STG_ABSORB_MAX_COLS,
              "pbn_absorb_plan.hpp restates pbn_params.hpp's block and column cap");

namespace {

// The arithmetic of one column of one row is spelled out and never contracted, so that it does not depend on the
// instantiation (column tile, rows per trip) the column is swept in: a lane's single term is the rounded product
// m * (x[t] - x[s]) -- what k_stg_expect_rows computes -- a lane's further terms enter by a fused multiply-add --
// what k_stg_expect's loop compiles to -- and the butterfly, the scaling, the division and the two adds are plain.

// out = x + (acc * 2^-53) / n_movable + b for a transient row, x itself (the same bits) for a labelled one. b is always
// added, as the recursion is stated: with b = +0.0 a sum of -0.0 (x and the scaled acc both -0.0) comes out +0.0, the
// one value at which the bits differ from k_stg_expect's.
__device__ __forceinline__ double absorb_value(bool held, double xs, double acc, double n_movable, double b) {
#pragma clang fp contract(off)
    const double e = (xs + (acc * 0x1p-53) / n_movable) + b;
    return held ? xs : e;
}

// N > G = 64: lane j adds its cells j, j + 64, ... in that order, one row per trip. Each lane loads its mass / succ
// cell once and gathers the successor's first n_cols columns, contiguous doubles of one row of x. The trip count is
// the workgroup's (it runs on its first row), so every lane reaches every shuffle; a row past the end takes part
// with zeros and writes nothing. A labelled row skips its cells: its sums are not used.
template <int CT>
__global__ __launch_bounds__(BLOCK, 4) void k_stg_absorb(StgAbsorbArgs a) {
#pragma clang fp contract(off)
    constexpr int G = (int)CONTROL_WAVE;
    constexpr uint32_t RPB = BLOCK / G;
    const uint32_t j = threadIdx.x % G, r = threadIdx.x / G;
    const uint64_t N = a.n_nodes, S = a.n_states, ld = a.ld;
    const int nc = (int)a.n_cols;
    const uint64_t stride = (uint64_t)gridDim.x * RPB;
    for (uint64_t base = (uint64_t)blockIdx.x * RPB; base < S; base += stride) {
        const uint64_t row = base + r;
        const bool live = row < S;
        const bool held = live && a.label[row] >= 0;
        double acc[CT], xs[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = xs[c] = 0.0;
        if (live) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < nc) xs[c] = a.x[row * ld + c];
            if (!held) {
                const uint64_t c0 = row * N;
                for (uint64_t i = j; i < N; i += G) {
                    const double m = (double)a.mass[c0 + i];  // <= 2^53: exact
                    uint64_t t = (uint64_t)(uint32_t)a.succ[c0 + i];
                    t = t < S ? t : row;
                    const double* xt = a.x + t * ld;
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c < nc) acc[c] = __builtin_fma(m, xt[c] - xs[c], acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < nc) {
#pragma unroll
                for (int d = G / 2; d >= 1; d >>= 1) acc[c] += __shfl_xor(acc[c], d);
            }
        if (live && j == 0u) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < nc) a.out[row * ld + c] = absorb_value(held, xs[c], acc[c], a.n_movable, a.src.b[c]);
        }
    }
}

// N <= G: a lane has one cell, and a group takes R rows per trip -- rows base + k * RPB + r -- with no branch between
// their loads: mass, succ, label and the row's own columns of all R rows are in flight before the first gather is
// issued, and all R * n_cols gathers before the first butterfly (k_stg_expect_rows' schedule). A lane past N and a
// row past S load cell 0 of a row that exists and contribute nothing; a labelled row gathers from itself (the line it
// has just read). The sum of a row is the butterfly over the lanes' single terms: k_stg_expect's order.
template <int G, int CT, int R>
__global__ __launch_bounds__(BLOCK, 4) void k_stg_absorb_rows(StgAbsorbArgs a) {
#pragma clang fp contract(off)
    constexpr uint32_t RPB = BLOCK / G;
    const uint32_t j = threadIdx.x % G, r = threadIdx.x / G;
    const uint64_t N = a.n_nodes, S = a.n_states, ld = a.ld;
    const int nc = (int)a.n_cols;
    const bool on = j < N;
    const uint64_t cell = on ? j : 0u;
    const uint64_t stride = (uint64_t)gridDim.x * RPB * R;
    for (uint64_t base = (uint64_t)blockIdx.x * RPB * R; base < S; base += stride) {
        uint64_t row[R];
        unsigned long long m[R];
        int32_t to[R], lab[R];
        double xs[R][CT], xt[R][CT];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint64_t want = base + (uint64_t)k * RPB + r;
            row[k] = want < S ? want : S - 1;
            m[k] = a.mass[row[k] * N + cell];
            to[k] = a.succ[row[k] * N + cell];
            lab[k] = a.label[row[k]];
#pragma unroll
            for (int c = 0; c < CT; ++c) xs[k][c] = c < nc ? a.x[row[k] * ld + c] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            uint64_t t = (uint64_t)(uint32_t)to[k];
            t = (t < S && lab[k] < 0) ? t : row[k];
#pragma unroll
            for (int c = 0; c < CT; ++c) xt[k][c] = c < nc ? a.x[t * ld + c] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const bool mine = j == 0u && base + (uint64_t)k * RPB + r < S;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (c < nc) {
                    double acc = on ? (double)m[k] * (xt[k][c] - xs[k][c]) : 0.0;
#pragma unroll
                    for (int d = G / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
                    if (mine) a.out[row[k] * ld + c] = absorb_value(lab[k] >= 0, xs[k][c], acc, a.n_movable, a.src.b[c]);
                }
        }
    }
}

template <int CT>
void* rows_by_group(uint32_t G) {
    constexpr int R = (int)absorb_rows_unrolled(CT, true);
    switch (G) {
        case 1: return (void*)k_stg_absorb_rows<1, CT, R>;
        case 2: return (void*)k_stg_absorb_rows<2, CT, R>;
        case 4: return (void*)k_stg_absorb_rows<4, CT, R>;
        case 8: return (void*)k_stg_absorb_rows<8, CT, R>;
        case 16: return (void*)k_stg_absorb_rows<16, CT, R>;
        case 32: return (void*)k_stg_absorb_rows<32, CT, R>;
        case 64: return (void*)k_stg_absorb_rows<64, CT, R>;
        default: return nullptr;
    }
}

}  // namespace

// ------------------------------------------------------------------ dispatch
// G, one_cell, col_tile: AbsorbPlan's G, cells_per_lane == 1 and col_tile. Launch and occupancy: launch_control /
// max_blocks_control (BLOCK threads, one argument struct, no LDS).
void* stg_absorb_kernel(uint32_t G, bool one_cell, uint32_t col_tile) {
    if (one_cell) switch (col_tile) {
            case 1: return rows_by_group<1>(G);
            case 2: return rows_by_group<2>(G);
            case 4: return rows_by_group<4>(G);
            case 8: return rows_by_group<8>(G);
            default: return nullptr;
        }
    if (G != CONTROL_WAVE) return nullptr;
    switch (col_tile) {
        case 1: return (void*)k_stg_absorb<1>;
        case 2: return (void*)k_stg_absorb<2>;
        case 4: return (void*)k_stg_absorb<4>;
        case 8: return (void*)k_stg_absorb<8>;
        default: return nullptr;
    }
}

}  // namespace pbn
