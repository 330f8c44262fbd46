// pbn_env_device.hpp -- device helpers of the env-step kernels (k_env, k_env_grp) and k_flip: action
// rows, attractor cubes, packed mismatch counters, wave scans.
#pragma once
#include "pbn_device.hpp"

namespace pbn {

// Python list indexing of flipNode(a - offset): valid for -N <= idx < N.
__device__ __forceinline__ bool action_node(int32_t a, int32_t offset, int32_t N, uint32_t* node) {
    const int32_t idx = a - offset;
    if (idx >= N || idx < -N) return false;
    *node = (uint32_t)(idx < 0 ? idx + N : idx);
    return true;
}

// Flip every (unique, if dedup) non-zero action of the row; returns the number of
// actions counted by the reference's reward (unique values incl. 0, or A).
template <int W>
__device__ __forceinline__ int apply_actions(uint64_t (&s)[W], const int32_t* row, int32_t A, int32_t offset,
                                             int32_t dedup, int32_t N, bool* bad) {
    int n_act = 0;
    for (int32_t k = 0; k < A; ++k) {
        const int32_t v = row[k];
        bool dup = false;
        if (dedup)
            for (int32_t q = 0; q < k; ++q) dup |= (row[q] == v);
        if (dup) continue;
        ++n_act;
        if (v == 0) continue;
        uint32_t node;
        if (!action_node(v, offset, N, &node)) {
            *bad = true;
            continue;
        }
        setbit<W>(s, node, getbit<W>(s, node) ^ 1u);
    }
    return dedup ? n_act : A;
}

template <int W>
__device__ __forceinline__ bool cube_match(const uint64_t (&s)[W], const uint64_t* cv) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < W; ++k) ok &= ((s[k] & cv[k]) == cv[W + k]);
    return ok;
}

template <int W>
__device__ __forceinline__ bool attracting(const uint64_t (&s)[W], const uint64_t* cubes, int32_t H) {
    bool hit = false;
    for (int32_t h = 0; h < H && !hit; ++h) hit = cube_match<W>(s, cubes + (uint64_t)h * 2 * W);
    return hit;
}

// Mismatch count of a state against one cube: #cared bits that differ from the cube.
template <int W>
__device__ __forceinline__ uint32_t cube_mismatch(const uint64_t (&s)[W], const uint64_t* cv) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) m += (uint32_t)__popcll((s[k] & cv[k]) ^ cv[W + k]);
    return m;
}

template <int W, class P_t>
__device__ __forceinline__ bool attracting_plane(const P_t& P, const uint64_t* cubes, int32_t H) {
    uint64_t s[W];
    from_plane<W>(P, s);
    return attracting<W>(s, cubes, H);
}

__device__ __forceinline__ uint32_t has_zero_byte(uint32_t v) { return (v - 0x01010101u) & ~v & 0x80808080u; }

// Predictor choice within one 16-B row of compact thresholds (Thr32): how many of the four the draw word reaches.
__device__ __forceinline__ uint32_t cnt4(const uint4& t4, uint32_t a32) {
    return (a32 >= t4.x ? 1u : 0u) + (a32 >= t4.y ? 1u : 0u) + (a32 >= t4.z ? 1u : 0u) + (a32 >= t4.w ? 1u : 0u);
}

// Inclusive prefix sum over the wave's 64 lanes (row_shr 1/2/4/8 inside each 16-lane row, then
// row_bcast15 / row_bcast31 carry the row totals; lanes without a source add 0).
// Inclusive max over the wave (the same DPP pattern; lanes without a source take 0): lane 63 holds the max.
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false));
    return x;
}

__device__ __forceinline__ uint32_t wave_inclusive_add(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
    return x;
}
}  // namespace pbn
