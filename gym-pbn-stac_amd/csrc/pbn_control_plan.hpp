// pbn_control_plan.hpp -- the launch shape of the two reducing kernels of pbn_control.hip (k_stg_expect, k_stg_backup;
// DESIGN.md §17), from plain integers: the lanes that own a row, the rows a wave and a workgroup cover, the grid.
//
// A group of G lanes owns a row: G is the smallest power of two >= N, at most 64 (the wave). Lane j of the group takes
// cells j, j + G, ... of its row, so the loads of a group are contiguous along the row and consecutive groups of a
// wave read consecutive rows; the group then reduces with a fixed xor butterfly over G lanes. Where a lane has one
// cell (N <= 64) a group takes CONTROL_UNROLL rows per trip of its row loop, a workgroup's rows apart, so that their
// loads are in flight together. Nothing here depends on the grid but the grid itself: the order in which a row's
// cells are combined is a function of (N, G) alone.
//
// No HIP and no other project header: tests/host/control_plan_check.cpp compiles it alone.
#pragma once
#include <cstdint>

namespace pbn {

constexpr uint32_t CONTROL_BLOCK = 256;  // threads per workgroup (BLOCK of pbn_params.hpp: 4 wave64)
constexpr uint32_t CONTROL_WAVE = 64;
constexpr uint32_t CONTROL_MAX_NODES = 512;  // 64 * MAX_WORDS
constexpr uint32_t CONTROL_UNROLL = 4;       // rows a group takes per trip where a lane has one cell (N <= 64)

struct ControlPlan {
    uint32_t G;               // lanes per row: a power of two in [1, 64]
    uint32_t rows_per_wave;   // 64 / G
    uint32_t rows_per_block;  // CONTROL_BLOCK / G
    uint32_t cells_per_lane;  // ceil(N / G): 1 up to N = 64
    uint32_t rows_unrolled;   // rows a group takes per trip of the row loop, rows_per_block apart: CONTROL_UNROLL where
                              // cells_per_lane == 1 (their loads go out together), else 1
    int grid;                 // workgroups: what the rows need, at most what is resident, at most the cap; >= 1
};

// The smallest power of two >= n_nodes, at most the wave.
constexpr uint32_t control_group(uint32_t n_nodes) {
    uint32_t g = 1;
    while (g < n_nodes && g < CONTROL_WAVE) g *= 2;
    return g;
}

// n_states >= 1 rows of n_nodes in [1, CONTROL_MAX_NODES] cells; n_cu x bpc workgroups are resident (each taken as at
// least 1); grid_cap > 0 caps the grid (PBNSIM_STG_GRID), anything else leaves it.
inline ControlPlan control_plan(uint64_t n_states, uint32_t n_nodes, int n_cu, int bpc, int grid_cap) {
    ControlPlan p{};
    p.G = control_group(n_nodes);
    p.rows_per_wave = CONTROL_WAVE / p.G;
    p.rows_per_block = CONTROL_BLOCK / p.G;
    p.cells_per_lane = (n_nodes + p.G - 1) / p.G;
    p.rows_unrolled = p.cells_per_lane == 1 ? CONTROL_UNROLL : 1;
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    const uint64_t need = (n_states + per_trip - 1) / per_trip;
    const uint64_t resident = (uint64_t)(n_cu < 1 ? 1 : n_cu) * (uint64_t)(bpc < 1 ? 1 : bpc);
    uint64_t grid = need < resident ? need : resident;
    if (grid_cap > 0 && grid > (uint64_t)grid_cap) grid = (uint64_t)grid_cap;
    p.grid = (int)(grid < 1 ? 1 : grid);
    return p;
}

}  // namespace pbn
