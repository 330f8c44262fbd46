// pbn_absorb_plan.hpp -- the launch shape of k_stg_absorb (pbn_absorb.hip), from plain integers: the
// lanes that own a row, the columns a kernel instantiation holds, the rows a group takes per trip, the grid.
//
// The row mapping is pbn_control_plan.hpp's: a group of G lanes owns a row (G the smallest power of two >= N, at most
// 64), lane j takes cells j, j + G, ..., the group reduces with the fixed xor butterfly. A launch advances n_cols in
// [1, 8] columns; the kernels are instantiated for a column tile CT in {1, 2, 4, 8}, the smallest that holds n_cols,
// and a column past n_cols is neither read nor written. Where a lane has one cell (N <= 64) a group takes
// ABSORB_ROW_GATHERS / CT rows per trip, at most 4, so that a lane has up to eight successor gathers in flight whatever
// the tile: 4, 4, 2, 1 rows for CT = 1, 2, 4, 8. Nothing here depends on the grid but the grid itself, and nothing
// in the order in which a row's cells are combined depends on the columns: it is a function of (N, G) alone.
//
// No HIP: tests/host/absorb_plan_check.cpp compiles it with pbn_control_plan.hpp alone.
#pragma once
#include <cstdint>

#include "pbn_control_plan.hpp"

namespace pbn {

constexpr uint32_t ABSORB_MAX_COLS = 8;     // columns of one launch (PBN_STG_ABSORB_MAX_COLS)
constexpr uint32_t ABSORB_ROW_GATHERS = 8;  // successor gathers a lane has in flight per trip where it has one cell
constexpr uint32_t ABSORB_MAX_UNROLL = 4;   // CONTROL_UNROLL: more rows per trip gained nothing there

struct AbsorbPlan {
    uint32_t G;               // lanes per row: a power of two in [1, 64]
    uint32_t rows_per_wave;   // 64 / G
    uint32_t rows_per_block;  // CONTROL_BLOCK / G
    uint32_t cells_per_lane;  // ceil(N / G): 1 up to N = 64
    uint32_t col_tile;        // CT: 1, 2, 4 or 8, the smallest >= n_cols
    uint32_t rows_unrolled;   // rows a group takes per trip, rows_per_block apart: min(4, 8 / CT) where cells_per_lane
                              // == 1, else 1
    int grid;                 // workgroups: what the rows need, at most what is resident, at most the cap; >= 1
};

// The smallest of 1, 2, 4, 8 that is >= n_cols (n_cols in [1, ABSORB_MAX_COLS]).
constexpr uint32_t absorb_col_tile(uint32_t n_cols) {
    uint32_t t = 1;
    while (t < n_cols && t < ABSORB_MAX_COLS) t *= 2;
    return t;
}

constexpr uint32_t absorb_rows_unrolled(uint32_t col_tile, bool one_cell) {
    if (!one_cell) return 1;
    const uint32_t r = ABSORB_ROW_GATHERS / col_tile;
    return r > ABSORB_MAX_UNROLL ? ABSORB_MAX_UNROLL : (r < 1 ? 1 : r);
}

// n_states >= 1 rows of n_nodes in [1, CONTROL_MAX_NODES] cells, n_cols in [1, ABSORB_MAX_COLS] columns; n_cu x bpc
// workgroups are resident (each taken as at least 1); grid_cap > 0 caps the grid (PBNSIM_STG_GRID).
inline AbsorbPlan absorb_plan(uint64_t n_states, uint32_t n_nodes, uint32_t n_cols, int n_cu, int bpc, int grid_cap) {
    AbsorbPlan p{};
    p.G = control_group(n_nodes);
    p.rows_per_wave = CONTROL_WAVE / p.G;
    p.rows_per_block = CONTROL_BLOCK / p.G;
    p.cells_per_lane = (n_nodes + p.G - 1) / p.G;
    p.col_tile = absorb_col_tile(n_cols);
    p.rows_unrolled = absorb_rows_unrolled(p.col_tile, p.cells_per_lane == 1);
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    const uint64_t need = (n_states + per_trip - 1) / per_trip;
    const uint64_t resident = (uint64_t)(n_cu < 1 ? 1 : n_cu) * (uint64_t)(bpc < 1 ? 1 : bpc);
    uint64_t grid = need < resident ? need : resident;
    if (grid_cap > 0 && grid > (uint64_t)grid_cap) grid = (uint64_t)grid_cap;
    p.grid = (int)(grid < 1 ? 1 : grid);
    return p;
}

}  // namespace pbn
