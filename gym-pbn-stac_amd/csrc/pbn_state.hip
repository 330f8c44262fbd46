// pbn_state.hip -- kernels that set, flip and unpack env states outside an update: k_init, k_flip, k_unpack.
//
// Reference semantics implemented (file:line in the reference):
//   k_init    Graph.genRandState base.py:368-370 / PBN.reset(None) pbn.py:105-118 /
//             PBNTargetMultiEnv.reset pbn_target_multi.py:237-249 (Philox streams)
//   k_flip    Graph.flipNode base.py:280-284 over a multi-action row (pbn_target_multi.py:120-131)
#include <hip/hip_runtime.h>

#include "pbn_device.hpp"
#include "pbn_env_device.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"

namespace pbn {

// ------------------------------------------------------------------ init / reset
template <int W>
__global__ __launch_bounds__(BLOCK) void k_init(InitArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.B) return;
    if (a.mask && !a.mask[e]) return;
    const uint64_t g = a.env_base + e;
    uint64_t s[W];
#pragma unroll
    for (int m = 0; 2 * m < W; ++m) {
        uint32_t w[4];
        philox_draw(a.seed, (uint32_t)m + (a.cube_care ? 1u : 0u), a.reset_count, g,
                    a.cube_care ? STREAM_RESET : STREAM_INIT, w);
        s[2 * m] = ((uint64_t)w[1] << 32) | w[0];
        if (2 * m + 1 < W) s[2 * m + 1] = ((uint64_t)w[3] << 32) | w[2];
    }
    if (a.cube_care) {
        uint32_t w[4];
        philox_draw(a.seed, 0u, a.reset_count, g, STREAM_RESET, w);
        const uint32_t c = __umulhi(w[0], (uint32_t)a.n_cubes);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t care = a.cube_care[(uint64_t)c * W + k];
            s[k] = (a.cube_value[(uint64_t)c * W + k] & care) | (s[k] & ~care);
        }
    }
    const int r = a.n_nodes & 63;
    if (r) s[W - 1] &= (((uint64_t)1 << r) - 1);
    if (a.kind == KIND_PROB_TABLE) s[0] &= ~(uint64_t)1;  // pbn.py:118 state[0] = 0
    store_state<W>(a.state + e * W, s);
    if (a.n_steps) a.n_steps[e] = 0;
}

template <int W>
__global__ __launch_bounds__(BLOCK) void k_flip(FlipArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.B) return;
    uint64_t s[W];
    load_state<W>(a.state + e * W, s);
    bool bad = false;
    apply_actions<W>(s, a.actions + e * (uint64_t)a.A, a.A, a.offset, a.dedup, a.n_nodes, &bad);
    if (bad) {
        atomicOr(a.error, 1);
        return;  // leave this env untouched
    }
    store_state<W>(a.state + e * W, s);
}

int launch_init(int W, const InitArgs& a, int grid, void* stream) {
    InitArgs c = a;
    return launch(by_words<8>(W, [](auto w) { return (void*)k_init<w>; }), grid, BLOCK, 0, stream, &c);
}

int launch_flip(int W, const FlipArgs& a, int grid, void* stream) {
    FlipArgs c = a;
    return launch(by_words<8>(W, [](auto w) { return (void*)k_flip<w>; }), grid, BLOCK, 0, stream, &c);
}

// Packed state words [B][W] -> one byte per node [B][N] (Graph.getState as bytes, base.py:320-324):
// one thread per output byte, so consecutive lanes write consecutive bytes (the rows of N bytes
// are not 4-byte aligned) and read the same few words through L1/L2.
__global__ __launch_bounds__(BLOCK) void k_unpack(const uint64_t* __restrict__ words, uint8_t* __restrict__ out,
                                                  uint64_t total, uint32_t N, uint32_t W) {
    if (total <= 0xFFFFFFFFull) {  // 32-bit index math (a 64-bit divide is a long software sequence)
        for (uint32_t k = blockIdx.x * BLOCK + threadIdx.x; k < (uint32_t)total; k += gridDim.x * BLOCK) {
            const uint32_t e = k / N, n = k - e * N;
            out[k] = (uint8_t)((words[(uint64_t)e * W + (n >> 6)] >> (n & 63u)) & 1u);
        }
        return;
    }
    for (uint64_t k = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; k < total; k += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t e = k / N;
        const uint32_t n = (uint32_t)(k - e * N);
        out[k] = (uint8_t)((words[e * W + (n >> 6)] >> (n & 63u)) & 1u);
    }
}

int launch_unpack(const uint64_t* words, uint8_t* out, uint64_t B, uint32_t N, uint32_t W, int grid, void* stream) {
    const uint64_t total = B * N;
    void* kargs[] = {(void*)&words, (void*)&out, (void*)&total, (void*)&N, (void*)&W};
    return (int)hipLaunchKernel((const void*)k_unpack, dim3((unsigned)grid), dim3(BLOCK), kargs, 0,
                                (hipStream_t)stream);
}

}  // namespace pbn
