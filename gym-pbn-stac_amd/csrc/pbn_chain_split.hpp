// pbn_chain_split.hpp -- how step mode cuts a batch into the env ranges of its launch chains.
//
// No HIP and no other project header: tests/host/chain_split_check.cpp compiles it alone.
#pragma once
#include <cstdint>

namespace pbn {

constexpr int STEP_CHAINS_MAX = 4;  // launch chains of one batch (pbn_step; PBNSIM_STEP_CHAINS)

struct ChainSlice {
    uint64_t off = 0, len = 0;  // envs [off, off + len) of the batch
};

// Cuts [0, B) into at most S contiguous slices, in order, none empty; returns how many (1 <= count <= S,
// 1 for B == 0 with an empty slice 0). Every slice starts at a multiple of 2 x step_block envs when the
// batch holds S such units (whole workgroups of env pairs, so a slice's grid is the batch's share), else at
// an even env: env_base + off keeps the parity of env_base (the paired Philox path of k_step stays on)
// and off x W words stay 16-byte aligned for the state's vector loads. Units are dealt out evenly, the
// first slices taking the remainder; the last slice ends at B.
inline int chain_split(uint64_t B, int S, int step_block, ChainSlice (&out)[STEP_CHAINS_MAX]) {
    if (S > STEP_CHAINS_MAX) S = STEP_CHAINS_MAX;
    if (S < 1) S = 1;
    const uint64_t big = 2ull * (uint64_t)(step_block > 0 ? step_block : 1);
    const uint64_t unit = B >= (uint64_t)S * big ? big : 2ull;
    const uint64_t units = (B + unit - 1) / unit;
    if (units < (uint64_t)S) S = units ? (int)units : 1;
    const uint64_t per = units / (uint64_t)S, extra = units % (uint64_t)S;
    uint64_t at = 0;
    for (int c = 0; c < S; ++c) {
        const uint64_t end = at + (per + ((uint64_t)c < extra ? 1u : 0u)) * unit;
        out[c].off = at;
        out[c].len = (end < B ? end : B) - at;
        at = end < B ? end : B;
    }
    for (int c = S; c < STEP_CHAINS_MAX; ++c) out[c] = ChainSlice{};
    return S;
}

}  // namespace pbn
