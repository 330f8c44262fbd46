// pbn_mass_rule.hpp -- the law of the asynchronous update: with what mass does node i flip at state x?
//
// pbn_reach_rule.hpp states the support of the dynamics (can node i flip at x); this header states the law on the
// same network image, in the same style: no HIP header, PBN_HD functions, the state as a callable bit(j) -> 0 / 1.
// One definition for the kernel of pbn_stg.hip and for the host (pbn_net_edge_mass, tests/host/mass_rule_check.cpp).
//
// edge_mass is an integer in [0, 2^53]: in units of 2^-53, the probability that node i takes the value 1 - x_i at x
// given that node i is the node updated. It is the mass of the 53-bit draws k53 in [0, 2^53) that the kernels compare
// against the same thresholds, so it is exact: no rounding happens anywhere below the division by 2^53.
// Invariant (a test, not a refactor): can_flip(x, i) == (edge_mass(x, i) > 0).
#pragma once
#include <stdint.h>

#include "pbn_params.hpp"
#include "pbn_reach_rule.hpp"

namespace pbn {

constexpr uint64_t MASS_ONE = REACH_TWO53;  // the whole draw range: probability 1

// Predictor mix: predictor q of node i is selected by the draws in [max(T_0 .. T_{q-1}), T_q), the thresholds clamped
// to 2^53 and the last one taken as 2^53 exactly as predictor_can_flip clamps them; the mass is the sum of the widths
// of the live intervals whose predictor outputs 1 - x_i at x. This is PredictorNetwork.update_probability's sum
// (network.py) for x_i = 0 and 2^53 minus it for x_i = 1: the live widths add up to 2^53. The reference's
// Node.getStateProbs (base.py:68-87) is the same sum in doubles, `currCOD / CODsum` per predictor.
template <class Bit>
PBN_HD uint64_t predictor_edge_mass(Bit&& bit, uint32_t i, const uint8_t* tbl, const NetLayout& L) {
    const uint64_t* thr = reinterpret_cast<const uint64_t*>(tbl + L.off_thr) + i * L.tp;
    const uint64_t* rec = reinterpret_cast<const uint64_t*>(tbl + L.off_rec) + i * L.pmax;
    const uint32_t xi = bit(i);
    uint64_t prev = 0, mass = 0;
    for (uint32_t q = 0; q < L.pmax; ++q) {
        uint64_t t = q < L.tp ? thr[q] : ~0ull;
        t = t > MASS_ONE ? MASS_ONE : t;
        const uint64_t width = t > prev ? t - prev : 0;
        prev = t > prev ? t : prev;
        const uint64_t r = rec[q];
        const uint32_t p = (bit((uint32_t)r & 0xFFFFu) << 3) | (bit((uint32_t)(r >> 16) & 0xFFFFu) << 2) |
                           (bit((uint32_t)(r >> 32) & 0xFFFFu) << 1) | xi;
        const uint32_t y = (uint32_t)(r >> (48 + p)) & 1u;
        mass += (y ^ xi) ? width : 0;
    }
    return mass;
}

// Truth tables: with T = ceil(p * 2^53) the threshold of node i's table entry at x, the node becomes 1 for the draws
// k53 < T (PBN._compute_next_states' prob_true, pbn.py:186-199; PBCN._async_compute_next_states, pbcn.py:72-93), so it
// leaves 0 with mass T and leaves 1 with mass 2^53 - T. T <= 2^53 for every double p <= 1; a larger stored value is
// clamped, as the draws never reach it.
template <class Bit>
PBN_HD uint64_t table_edge_mass(Bit&& bit, uint32_t i, const uint8_t* tbl, const NetLayout& L) {
    const uint64_t info = reinterpret_cast<const uint64_t*>(tbl + L.off_node)[i];
    const uint32_t toff = (uint32_t)info, ioff = (uint32_t)(info >> 32) & 0xFFFFu, k = (uint32_t)(info >> 48) & 0xFFu;
    const uint16_t* in = reinterpret_cast<const uint16_t*>(tbl + L.off_rec) + ioff;
    uint32_t idx = 0;
    for (uint32_t q = 0; q < k; ++q) idx = (idx << 1) | bit(in[q]);
    uint64_t T = reinterpret_cast<const uint64_t*>(tbl + L.off_thr)[toff + idx];
    T = T > MASS_ONE ? MASS_ONE : T;
    return bit(i) ? MASS_ONE - T : T;
}

// The mass of a network of either kind; nodes below `first` (table_graph_first_node) never move: mass 0.
template <int KIND, class Bit>
PBN_HD uint64_t edge_mass(Bit&& bit, uint32_t i, uint32_t first, const uint8_t* tbl, const NetLayout& L) {
    if (i < first) return 0ull;
    if constexpr (KIND == KIND_PREDICTOR_MIX)
        return predictor_edge_mass(bit, i, tbl, L);
    else
        return table_edge_mass(bit, i, tbl, L);
}

}  // namespace pbn
