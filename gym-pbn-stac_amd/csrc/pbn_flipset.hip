// pbn_flipset.hip -- the max over multi-flip action sets of the until-attractor MDP: one level of the
// top-two recursion of pbn_flipset_rule.hpp over the flip neighbours of pbn_control.hip, and the choice of the action.
//
// Reference semantics implemented (file:line in the reference):
//   k_stg_flipset         the max over the action sets of PBNTargetMultiEnv.step (pbn_target_multi.py:105-131: up to A
//                         distinct nodes are flipped, each at action_cost) of the worth of the state the flips lead to.
//                         The reference has no such code: it trains agents against this MDP and never solves it.
//   k_stg_flipset_select  the best non-empty set from the last level's summary, against the empty set where that is an
//                         action
// Launch shape of the level kernels: pbn_control_plan.hpp, unchanged (k_stg_backup's mapping).
#include <hip/hip_runtime.h>

#include "pbn_control_plan.hpp"
#include "pbn_flipset_rule.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"

namespace pbn {

namespace {

// T_{j-1}[t] with one more flip on the way: what row t hands to a neighbour. Without an input summary (level 0 -> 1)
// T_0[t] is (t, 0, m[t]) alone. The branch is the launch's, the same for every lane.
__device__ __forceinline__ FlipPair flipset_from(const StgFlipsetArgs& a, uint64_t t) {
    FlipPair p;
    if (a.in_base) {
        const double2 b = *reinterpret_cast<const double2*>(a.in_base + 2 * t);
        const int2 g = *reinterpret_cast<const int2*>(a.in_tag + 2 * t);
        p.e0 = FlipEntry{b.x, g.x};
        p.e1 = FlipEntry{b.y, g.y};
    } else {
        p.e0 = flip_entry((int32_t)t, 0, a.m[t]);
        p.e1 = flip_none();
    }
    return p;
}

__device__ __forceinline__ FlipPair flipset_bumped(const FlipPair& p) { return FlipPair{flip_bump(p.e0), flip_bump(p.e1)}; }

__device__ __forceinline__ void flipset_store(const StgFlipsetArgs& a, uint64_t row, const FlipPair& p) {
    *reinterpret_cast<double2*>(a.out_base + 2 * row) = double2{p.e0.base, p.e1.base};
    *reinterpret_cast<int2*>(a.out_tag + 2 * row) = int2{p.e0.tag, p.e1.tag};
}

// The fixed xor butterfly over the group's G lanes with the rule's merge: the order is total and the merge of two
// pairs does not depend on the side it is made from, so every lane of the group ends with the same pair.
template <int G>
__device__ __forceinline__ FlipPair flipset_reduce(FlipPair p, double k) {
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) {
        FlipPair o;
        o.e0 = FlipEntry{__shfl_xor(p.e0.base, d), __shfl_xor(p.e0.tag, d)};
        o.e1 = FlipEntry{__shfl_xor(p.e1.base, d), __shfl_xor(p.e1.tag, d)};
        p = flip_merge(p, o, k);
    }
    return p;
}

// N > G = 64: lane j folds the pairs of the neighbours through nodes j, j + 64, ... into the row's own pair, one row
// per trip; a cell that is -1 (a node that is not allowed) or no row adds nothing. The trip count is the workgroup's
// (it runs on its first row), so every lane reaches every shuffle; a row past the end takes part with empty pairs and
// writes nothing.
template <int G>
__global__ __launch_bounds__(BLOCK, 4) void k_stg_flipset(StgFlipsetArgs a) {
#pragma clang fp contract(off)
    constexpr uint32_t RPB = BLOCK / G;
    const uint32_t j = threadIdx.x % G, r = threadIdx.x / G;
    const uint64_t N = a.n_nodes, S = a.n_states;
    const double k = a.cost;
    const uint64_t stride = (uint64_t)gridDim.x * RPB;
    for (uint64_t base = (uint64_t)blockIdx.x * RPB; base < S; base += stride) {
        const uint64_t row = base + r;
        const bool live = row < S;
        FlipPair p{flip_none(), flip_none()};
        if (live) {
            p = flipset_from(a, row);
            const uint64_t c0 = row * N;
            for (uint64_t i = j; i < N; i += G) {
                const uint64_t t = (uint64_t)(uint32_t)a.nbr[c0 + i];
                if (t < S) p = flip_merge(p, flipset_bumped(flipset_from(a, t)), k);
            }
        }
        p = flipset_reduce<G>(p, k);
        if (live && j == 0u) flipset_store(a, row, p);
    }
}

// N <= G: a lane has one node, and a group takes CONTROL_UNROLL rows per trip -- rows base + q * RPB + r -- with no
// branch between their loads: the nbr cells and the rows' own pairs of all of them are in flight before the first
// gather is issued, and all gathers before the first butterfly (k_stg_backup_rows' schedule). A lane past N and a
// row past S load cell 0 of a row that exists; the lane past N folds nothing in, the row past S is not written.
template <int G>
__global__ __launch_bounds__(BLOCK, 4) void k_stg_flipset_rows(StgFlipsetArgs a) {
#pragma clang fp contract(off)
    constexpr int R = (int)CONTROL_UNROLL;
    constexpr uint32_t RPB = BLOCK / G;
    const uint32_t j = threadIdx.x % G, r = threadIdx.x / G;
    const uint64_t N = a.n_nodes, S = a.n_states;
    const double k = a.cost;
    const bool on = j < N;
    const uint64_t cell = on ? j : 0u;
    const uint64_t stride = (uint64_t)gridDim.x * RPB * R;
    for (uint64_t base = (uint64_t)blockIdx.x * RPB * R; base < S; base += stride) {
        uint64_t row[R];
        int32_t to[R];
        FlipPair own[R], far[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint64_t want = base + (uint64_t)q * RPB + r;
            row[q] = want < S ? want : S - 1;
            to[q] = a.nbr[row[q] * N + cell];
            own[q] = flipset_from(a, row[q]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint64_t t = (uint64_t)(uint32_t)to[q];
            far[q] = flipset_from(a, t < S ? t : row[q]);
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const bool act = on && (uint64_t)(uint32_t)to[q] < S;
            FlipPair f = flipset_bumped(far[q]);
            f.e0.tag = act ? f.e0.tag : FLIPSET_EMPTY;
            f.e1.tag = act ? f.e1.tag : FLIPSET_EMPTY;
            const FlipPair p = flipset_reduce<G>(flip_merge(own[q], f, k), k);
            if (j == 0u && base + (uint64_t)q * RPB + r < S) flipset_store(a, row[q], p);
        }
    }
}

// A lane per row: the best action from T_A[row] (the first entry whose end is not the row), against the empty set at
// m[row] - noop_cost where that is an action; on a tie the empty set (fewer flips). No entry and no empty set: -inf, -1.
__global__ __launch_bounds__(BLOCK) void k_stg_flipset_select(StgFlipsetSelectArgs a) {
#pragma clang fp contract(off)
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t row = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; row < a.n_states; row += stride) {
        const double2 b = *reinterpret_cast<const double2*>(a.base + 2 * row);
        const int2 g = *reinterpret_cast<const int2*>(a.tag + 2 * row);
        const FlipPair p{FlipEntry{b.x, g.x}, FlipEntry{b.y, g.y}};
        const FlipEntry e = flip_action(p, (int32_t)row);
        double v = flip_is(e) ? flip_value(e, a.cost) : -__builtin_huge_val();
        int32_t end = flip_is(e) ? flip_end(e) : -1, flips = flip_is(e) ? flip_count(e) : 0;
        if (a.has_noop) {
            const double stay = a.m[row] - a.noop_cost;
            if (!flip_is(e) || stay >= v) {
                v = stay;
                end = (int32_t)row;
                flips = 0;
            }
        }
        a.v[row] = v;
        a.policy_end[row] = end;
        a.policy_flips[row] = flips;
    }
}

}  // namespace

// ------------------------------------------------------------------ dispatch
// G, one_cell: ControlPlan's G and cells_per_lane == 1. Launch and occupancy: launch_control / max_blocks_control (BLOCK
// threads, one argument struct, no LDS).
void* stg_flipset_kernel(uint32_t G, bool one_cell) {
    if (!one_cell) return G == CONTROL_WAVE ? (void*)k_stg_flipset<(int)CONTROL_WAVE> : nullptr;
    switch (G) {
        case 1: return (void*)k_stg_flipset_rows<1>;
        case 2: return (void*)k_stg_flipset_rows<2>;
        case 4: return (void*)k_stg_flipset_rows<4>;
        case 8: return (void*)k_stg_flipset_rows<8>;
        case 16: return (void*)k_stg_flipset_rows<16>;
        case 32: return (void*)k_stg_flipset_rows<32>;
        case 64: return (void*)k_stg_flipset_rows<64>;
        default: return nullptr;
    }
}

void* stg_flipset_select_kernel() { return (void*)k_stg_flipset_select; }

}  // namespace pbn
