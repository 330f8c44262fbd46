// pbn_control.hip -- exact optimal control over a transition graph: the per-sweep work of value
// iteration on the dense arrays of pbn_stg.hip, and the flip neighbours an action leads to.
//
// Reference semantics implemented (file:line in the reference):
//   k_stg_flip_rows  the action of PBNEnv.step pbn_env.py:141-142 (flip node `action`) as a map between rows of the set
//   k_stg_expect     the expectation over one PBN.step pbn.py:129-133 / Graph.step base.py:308 of a function of the next
//                    state, from the law k_stg_rows wrote (mass, succ)
//   k_stg_backup     the max over actions of the MDP PBNEnv.step + _get_reward (pbn_env.py:125-188) defines; the reference
//                    has no such code: it trains agents against this MDP and never solves it
// Launch shape of the two reducing kernels: pbn_control_plan.hpp.
#include <hip/hip_runtime.h>

#include "pbn_control_plan.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"
#include "pbn_stateset.hpp"

namespace pbn {

static_assert(CONTROL_BLOCK == (uint32_t)BLOCK && CONTROL_MAX_NODES == 64u * MAX_WORDS,
              "pbn_control_plan.hpp restates pbn_params.hpp's block and node cap");

namespace {

// Mapping: k_stg_rows' lane per cell (row, node), cells in row-major order: the store of a wave is 256 contiguous
// bytes whatever N is. A cell of a node that is not allowed is -1 with no probe; every other cell probes the set for
// x_row ^ bit(node) whatever the mass of that flip under the dynamics is (an action is not an update). The cell index
// is 64-bit: S * N reaches 2^33.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_stg_flip_rows(StgFlipArgs a) {
    const uint64_t N = a.n_nodes;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < a.n_cells; c += stride) {
        const uint64_t local = c / N;
        const uint32_t i = (uint32_t)(c - local * N), wi = i >> 6;
        const uint64_t bit = (uint64_t)1 << (i & 63u);
        uint64_t allowed = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) allowed = wi == (uint32_t)k ? a.allowed[k] : allowed;
        int32_t to = -1;
        if (allowed & bit) {
            const uint64_t row = a.first_row + local;
            uint64_t s[W];
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] = a.states[row * W + k] ^ (wi == (uint32_t)k ? bit : 0ull);
            to = stateset_lookup<W>(s, a.set.meta, a.set.keys, a.set.slots);
        }
        a.nbr[c] = to;
    }
}

// Where a group's lanes stand: lane j of the group that owns row r of the workgroup's RPB rows. The row loop's trip
// count is the same for every lane of the workgroup (it runs on the workgroup's first row), so every lane reaches
// every shuffle; a row past the end takes part with neutral values and writes nothing.
template <int G>
struct GroupLane {
    static constexpr uint32_t RPB = BLOCK / G;
    uint32_t j, r;
    __device__ GroupLane() : j(threadIdx.x % G), r(threadIdx.x / G) {}
};

// The fused pull: out[s] = v[s] + (sum_i mass[s][i] * (v[succ[s][i]] - v[s])) * 2^-53 / n_movable, one pass over
// mass (8 B per cell) and succ (4 B per cell), a gather of v per cell. A cell with mass 0 adds exactly 0. The sum of
// a row: each lane adds its cells j, j + G, ... in that order, then the fixed butterfly over the group's G lanes (the
// two sides of an exchange add the same two doubles, so every lane ends with the same bits): a function of (N, G).
// A successor that is no row (a leak: the callers refuse a set that is not closed) is read as "stays".
// The loop's `acc += m * (...)` compiles to a fused multiply-add under hipcc's default contraction; k_stg_absorb
// (pbn_absorb.hip) spells that out and a test holds the two bit-equal: mind it when changing the floating-point flags.
template <int G>
__global__ __launch_bounds__(BLOCK) void k_stg_expect(StgExpectArgs a) {
    const GroupLane<G> g;
    const uint64_t N = a.n_nodes, S = a.n_states;
    const uint64_t stride = (uint64_t)gridDim.x * g.RPB;
    for (uint64_t base = (uint64_t)blockIdx.x * g.RPB; base < S; base += stride) {
        const uint64_t row = base + g.r;
        const bool live = row < S;
        double acc = 0.0, vs = 0.0;
        if (live) {
            vs = a.v[row];
            const uint64_t c0 = row * N;
            for (uint64_t i = g.j; i < N; i += G) {
                const double m = (double)a.mass[c0 + i];  // <= 2^53: exact
                uint64_t t = (uint64_t)(uint32_t)a.succ[c0 + i];
                t = t < S ? t : row;
                acc += m * (a.v[t] - vs);
            }
        }
#pragma unroll
        for (int d = G / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (live && g.j == 0u) {
            const double e = vs + (acc * 0x1p-53) / a.n_movable;
            a.out[row] = e;
            if (a.pen) a.out_pen[row] = e - a.cost * a.pen[row];
        }
    }
}

// The same for N <= G (every network up to 64 nodes): a lane has one cell, and a group takes CONTROL_UNROLL rows per
// trip -- rows base + k * RPB + r -- with no branch between their loads, so the mass / succ loads of all of them are in
// flight before the first gather is issued, and all gathers before the first butterfly: a row's dependent chain
// (succ -> v[succ]) is two memory round trips, and one row per trip leaves the wave waiting through both. A lane past
// N and a row past S load cell 0 of a row that exists and contribute nothing. The sum of a row is the butterfly over
// the lanes' single terms: the same order as k_stg_expect's.
template <int G>
__global__ __launch_bounds__(BLOCK) void k_stg_expect_rows(StgExpectArgs a) {
    constexpr int R = (int)CONTROL_UNROLL;
    const GroupLane<G> g;
    const uint64_t N = a.n_nodes, S = a.n_states;
    const bool on = g.j < N;
    const uint64_t cell = on ? g.j : 0u;
    const uint64_t stride = (uint64_t)gridDim.x * g.RPB * R;
    for (uint64_t base = (uint64_t)blockIdx.x * g.RPB * R; base < S; base += stride) {
        uint64_t row[R];
        unsigned long long m[R];
        int32_t to[R];
        double vs[R], vt[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint64_t want = base + (uint64_t)k * g.RPB + g.r;
            row[k] = want < S ? want : S - 1;
            m[k] = a.mass[row[k] * N + cell];
            to[k] = a.succ[row[k] * N + cell];
            vs[k] = a.v[row[k]];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint64_t t = (uint64_t)(uint32_t)to[k];
            vt[k] = a.v[t < S ? t : row[k]];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double acc = on ? (double)m[k] * (vt[k] - vs[k]) : 0.0;
#pragma unroll
            for (int d = G / 2; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
            if (g.j == 0u && base + (uint64_t)k * g.RPB + g.r < S) {
                const double e = vs[k] + (acc * 0x1p-53) / a.n_movable;
                a.out[row[k]] = e;
                if (a.pen) a.out_pen[row[k]] = e - a.cost * a.pen[row[k]];
            }
        }
    }
}

// V'[s] = max(U[s], max over nodes i with nbr[s][i] a row of Ua[nbr[s][i]]) and its arg max: -1 for the no-op, else the
// node. Ties: the no-op first, then the lowest node -- a lane walks its nodes upwards and takes a strictly larger value
// only, the butterfly prefers the larger value and among equals the smaller node (the no-op is -1), a total order, so
// every lane of the group ends with the same pair.
template <int G>
__global__ __launch_bounds__(BLOCK) void k_stg_backup(StgBackupArgs a) {
    const GroupLane<G> g;
    const uint64_t N = a.n_nodes, S = a.n_states;
    const uint64_t stride = (uint64_t)gridDim.x * g.RPB;
    for (uint64_t base = (uint64_t)blockIdx.x * g.RPB; base < S; base += stride) {
        const uint64_t row = base + g.r;
        const bool live = row < S;
        double best = 0.0;
        int32_t node = -1;
        if (live) {
            best = a.u[row];
            const uint64_t c0 = row * N;
            for (uint64_t i = g.j; i < N; i += G) {
                const uint64_t t = (uint64_t)(uint32_t)a.nbr[c0 + i];
                if (t < S) {  // -1 (no action here) and anything that is no row
                    const double q = a.ua[t];
                    if (q > best) {
                        best = q;
                        node = (int32_t)i;
                    }
                }
            }
        }
#pragma unroll
        for (int d = G / 2; d >= 1; d >>= 1) {
            const double ob = __shfl_xor(best, d);
            const int32_t on = __shfl_xor(node, d);
            if (ob > best || (ob == best && on < node)) {
                best = ob;
                node = on;
            }
        }
        if (live && g.j == 0u) {
            a.v[row] = best;
            a.policy[row] = node;
        }
    }
}

// k_stg_backup for N <= G, CONTROL_UNROLL rows per trip as k_stg_expect_rows: a lane has one node, so its pair is
// (Ua[nbr], node) where that is an action and (U, -1) elsewhere, and the butterfly's total order does the rest.
template <int G>
__global__ __launch_bounds__(BLOCK) void k_stg_backup_rows(StgBackupArgs a) {
    constexpr int R = (int)CONTROL_UNROLL;
    const GroupLane<G> g;
    const uint64_t N = a.n_nodes, S = a.n_states;
    const bool on = g.j < N;
    const uint64_t cell = on ? g.j : 0u;
    const uint64_t stride = (uint64_t)gridDim.x * g.RPB * R;
    for (uint64_t base = (uint64_t)blockIdx.x * g.RPB * R; base < S; base += stride) {
        uint64_t row[R];
        int32_t to[R];
        double u[R], q[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint64_t want = base + (uint64_t)k * g.RPB + g.r;
            row[k] = want < S ? want : S - 1;
            to[k] = a.nbr[row[k] * N + cell];
            u[k] = a.u[row[k]];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint64_t t = (uint64_t)(uint32_t)to[k];
            q[k] = a.ua[t < S ? t : row[k]];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const bool act = on && (uint64_t)(uint32_t)to[k] < S && q[k] > u[k];
            double best = act ? q[k] : u[k];
            int32_t node = act ? (int32_t)g.j : -1;
#pragma unroll
            for (int d = G / 2; d >= 1; d >>= 1) {
                const double ob = __shfl_xor(best, d);
                const int32_t on_ = __shfl_xor(node, d);
                if (ob > best || (ob == best && on_ < node)) {
                    best = ob;
                    node = on_;
                }
            }
            if (g.j == 0u && base + (uint64_t)k * g.RPB + g.r < S) {
                a.v[row[k]] = best;
                a.policy[row[k]] = node;
            }
        }
    }
}

template <template <int> class K>
void* by_group(uint32_t G) {
    switch (G) {
        case 1: return K<1>::fn();
        case 2: return K<2>::fn();
        case 4: return K<4>::fn();
        case 8: return K<8>::fn();
        case 16: return K<16>::fn();
        case 32: return K<32>::fn();
        case 64: return K<64>::fn();
        default: return nullptr;
    }
}

template <int G>
struct Expect {
    static void* fn() { return (void*)k_stg_expect_rows<G>; }
};
template <int G>
struct Backup {
    static void* fn() { return (void*)k_stg_backup_rows<G>; }
};

}  // namespace

// ------------------------------------------------------------------ dispatch
void* stg_flip_rows_kernel(int W) {
    return by_words<MAX_WORDS>(W, [](auto w) { return (void*)k_stg_flip_rows<w>; });
}

// one_cell: N <= G, the unrolled kernels (ControlPlan::rows_unrolled rows per trip); otherwise G is the wave
void* stg_expect_kernel(uint32_t G, bool one_cell) {
    if (one_cell) return by_group<Expect>(G);
    return G == CONTROL_WAVE ? (void*)k_stg_expect<(int)CONTROL_WAVE> : nullptr;
}

void* stg_backup_kernel(uint32_t G, bool one_cell) {
    if (one_cell) return by_group<Backup>(G);
    return G == CONTROL_WAVE ? (void*)k_stg_backup<(int)CONTROL_WAVE> : nullptr;
}

// The three kernels take one argument struct, BLOCK threads and no LDS.
int launch_control(void* kernel, int grid, void* stream, void* args) {
    return launch(kernel, grid, BLOCK, 0, stream, args);
}

int max_blocks_control(void* kernel, int* blocks_per_cu) { return occupancy(kernel, BLOCK, 0, blocks_per_cu); }

}  // namespace pbn
