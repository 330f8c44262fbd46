// pbn_reach_rule.hpp -- the edge rule of the support graphs: can node i flip at state x?
//
// One definition for the kernels of pbn_reach.hip and for the host (pbn_net_unstable, tests/host/
// reach_rule_check.cpp): this header includes no HIP header, and its functions read the network image the
// same way on both sides. The state comes in as a callable bit(j) -> 0 / 1, so the kernels keep their state
// words in registers (getbit<W>) and the host reads them from memory.
#pragma once
#include <stdint.h>

#include "pbn_params.hpp"

#if defined(__HIPCC__)  // the compiler's own attributes: no HIP header needed for them
#define PBN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PBN_HD inline
#endif

namespace pbn {

constexpr uint64_t REACH_TWO53 = 1ull << 53;

// Truth-table networks, the two support graphs a caller has to choose between (PBN_TABLE_GRAPH_*, pbn_abi.h):
//   STG   nodes 0 .. N-1 may move: PBN._compute_next_states' async branch, the graph behind
//         PBNEnv.compute_attractors;
//   STEP  nodes 1 .. N-1 only: the graph PBN.step walks (randint(1, N-1); reset clears node 0).
// The value is the graph's code in the ABI; table_graph_first_node maps it to the lowest movable node.
enum { TABLE_GRAPH_NONE = 0, TABLE_GRAPH_STG = 1, TABLE_GRAPH_STEP = 2 };
constexpr uint32_t table_graph_first_node(int graph) { return graph == TABLE_GRAPH_STEP ? 1u : 0u; }

// Predictor mix: some live predictor of node i outputs 1 - x_i.
// Image (build_predictor_image): thr [N][tp] u64, the thresholds of the last predictor and of the padding
// UINT64_MAX -- clamped to 2^53 here, which is "the last threshold taken as 2^53" and makes every slot
// past the node's predictors an empty interval; rec [N][pmax] in0 | in1<<16 | in2<<32 | tt<<48.
template <class Bit>
PBN_HD uint32_t predictor_can_flip(Bit&& bit, uint32_t i, const uint8_t* tbl, const NetLayout& L) {
    const uint64_t* thr = reinterpret_cast<const uint64_t*>(tbl + L.off_thr) + i * L.tp;
    const uint64_t* rec = reinterpret_cast<const uint64_t*>(tbl + L.off_rec) + i * L.pmax;
    const uint32_t xi = bit(i);
    uint64_t prev = 0;
    uint32_t flip = 0;
    for (uint32_t q = 0; q < L.pmax; ++q) {
        uint64_t t = q < L.tp ? thr[q] : ~0ull;
        t = t > REACH_TWO53 ? REACH_TWO53 : t;
        const bool live = t > prev;
        prev = t > prev ? t : prev;
        const uint64_t r = rec[q];
        const uint32_t p = (bit((uint32_t)r & 0xFFFFu) << 3) | (bit((uint32_t)(r >> 16) & 0xFFFFu) << 2) |
                           (bit((uint32_t)(r >> 32) & 0xFFFFu) << 1) | xi;
        const uint32_t y = (uint32_t)(r >> (48 + p)) & 1u;
        flip |= live ? (y ^ xi) : 0u;
    }
    return flip;
}

// Truth tables: with T = ceil(p * 2^53) the threshold of node i's table entry at x (index: inputs in ascending
// node order, first input most significant, as table_eval_lds builds it), node i can flip iff
//   x_i = 0 and T > 0      (the reference's prob_true > 0.), or
//   x_i = 1 and T < 2^53   (prob_true < 1.).
// Exact on the thresholds: a double p > 0 is at least 2^-1074, so ceil(p * 2^53) >= 1; a double p < 1 is at
// most 1 - 2^-53, so p * 2^53 <= 2^53 - 1 with no rounding (a power-of-two scale), and its ceiling stays below
// 2^53. p = 0 and p = 1 give exactly 0 and 2^53.
// Image (build_table_image): node info [N] u64 toff | ioff<<32 | k<<48; inputs u16 at off_rec; thr u64.
// The input loop's trip count is the node's own k (0 .. 16): lanes of a wave that hold nodes of different k
// leave the loop one by one, and the wave pays the largest k among its nodes -- one 2-byte LDS read and one
// shift-or per input -- then one 8-byte read of the threshold.
template <class Bit>
PBN_HD uint32_t table_can_flip(Bit&& bit, uint32_t i, const uint8_t* tbl, const NetLayout& L) {
    const uint64_t info = reinterpret_cast<const uint64_t*>(tbl + L.off_node)[i];
    const uint32_t toff = (uint32_t)info, ioff = (uint32_t)(info >> 32) & 0xFFFFu, k = (uint32_t)(info >> 48) & 0xFFu;
    const uint16_t* in = reinterpret_cast<const uint16_t*>(tbl + L.off_rec) + ioff;
    uint32_t idx = 0;
    for (uint32_t q = 0; q < k; ++q) idx = (idx << 1) | bit(in[q]);
    const uint64_t T = reinterpret_cast<const uint64_t*>(tbl + L.off_thr)[toff + idx];
    return bit(i) ? (T < REACH_TWO53 ? 1u : 0u) : (T > 0 ? 1u : 0u);
}

// The rule of a network of either kind; nodes below `first` (table_graph_first_node) never move.
template <int KIND, class Bit>
PBN_HD uint32_t can_flip(Bit&& bit, uint32_t i, uint32_t first, const uint8_t* tbl, const NetLayout& L) {
    if (i < first) return 0u;
    if constexpr (KIND == KIND_PREDICTOR_MIX)
        return predictor_can_flip(bit, i, tbl, L);
    else
        return table_can_flip(bit, i, tbl, L);
}

}  // namespace pbn
