// pbn_lane_env.hpp -- the shape the env kernels over a state set share (k_tenv_step, k_tenv_macro, k_env_set;
// DESIGN.md §12-§14), defined once. The kernels keep what differs: the per-env body.
//
// One lane per env in BLOCK-thread workgroups. LDS per workgroup: [network image][state planes]; the image is
// staged once per workgroup and the envs are taken in a grid-stride loop by a grid sized to what is resident
// (a cached occupancy query on the host), so the staging is not paid once per 256 envs. A lane keeps its env's
// state in registers (the set lookup's operand) and on its LDS plane (the node update's operand), and stores it
// only if it ends different from what was loaded. An env whose input is refused is skipped whole -- state and
// outputs untouched -- and noted in a sticky device flag.
//
// The helpers are shaped by what compiles to the code the hand-written loops gave (tools/kernel_isa_diff.py): a
// loop body passed as a lambda, or a loop-state object that owns the live flag, keeps that flag as a byte in a VGPR
// and moves the kernels' register counts, so the walk is a range type and the ragged loop shares its condition.
#pragma once
#include "pbn_device.hpp"

namespace pbn {

// Stages the image (L.bytes / 16 granules, every thread), waits for it, and returns this lane's plane at byte
// plane_off of the workgroup's LDS.
__device__ __forceinline__ Plane lane_env_begin(uint8_t* lds, const void* img, const NetLayout& L, uint32_t plane_off) {
    stage_image(reinterpret_cast<const uint4*>(img), L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    return Plane{reinterpret_cast<uint32_t*>(lds + plane_off) + threadIdx.x};
}

// for (uint64_t e : lane_envs(B)): the envs e < B this lane takes -- its global thread id, then on by the grid's
// threads.
struct LaneEnvs {
    uint64_t B;
    struct End {};
    struct It {
        uint64_t e, B, stride;
        __device__ __forceinline__ uint64_t operator*() const { return e; }
        __device__ __forceinline__ void operator++() { e += stride; }
        __device__ __forceinline__ bool operator!=(End) const { return e < B; }
    };
    __device__ __forceinline__ It begin() const {
        const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
        return It{(uint64_t)blockIdx.x * BLOCK + threadIdx.x, B, stride};
    }
    __device__ __forceinline__ End end() const { return End{}; }
};
__device__ __forceinline__ LaneEnvs lane_envs(uint64_t B) { return LaneEnvs{B}; }

// Flips bit i (< 64 W) of s if `on`: a select per word, no register indexing (the state words must stay in VGPRs,
// pbn_device.hpp "packed state").
template <int W>
__device__ __forceinline__ void xor_bit(uint64_t (&s)[W], uint32_t i, bool on) {
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] ^= (((uint32_t)k == (i >> 6)) & on) ? 1ull << (i & 63u) : 0ull;
}

// The env's write-back: s, unless it equals s0, what was loaded from dst.
template <int W>
__device__ __forceinline__ void store_if_changed(uint64_t* __restrict__ dst, const uint64_t (&s)[W],
                                                 const uint64_t (&s0)[W]) {
    uint64_t diff = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) diff |= s[k] ^ s0[k];
    if (diff != 0ull) store_state<W>(dst, s);
}

// Lanes of a wave run different numbers of inner rounds:
//     for (uint32_t i = 0; rounds_left(i, cap, live); ++i) if (live) { ...; live = <goes on>; }
// The round counter i is kept wave-uniform -- what the body derives from it alone (Philox counter words, table
// indices) stays scalar -- and the wave leaves the loop when the ballot of live lanes is empty; a lane that has
// stopped sits the remaining rounds of its wave out with its results frozen.
__device__ __forceinline__ bool rounds_left(uint32_t i, uint32_t cap, bool live) {
    return i < cap && __ballot(live) != 0ull;
}

}  // namespace pbn
