// pbn_stg.hip -- the exact transition graph of a state set: for every state of the set and every node,
// the mass with which the node flips there and the row of the state that flip leads to.
//
// Reference semantics implemented (file:line in the reference):
//   k_stg_rows  Graph.getNextStates base.py:221-242 (and genSTG :199-218 over it): per node the probability of each next
//               value from Node.getStateProbs (:68-87); PBN._compute_next_states pbn.py:186-199 and
//               PBCN._async_compute_next_states pbcn.py:72-93 for truth tables (prob_true of the node's table entry).
//               The reference returns {next_state: prob}; here the mass is the exact integer of pbn_mass_rule.hpp and
//               the next state is named by its row in the set (pbn_stateset.hpp), so a graph is two dense arrays.
#include "pbn_device.hpp"
#include "pbn_launch.hpp"
#include "pbn_mass_rule.hpp"
#include "pbn_stateset.hpp"

namespace pbn {

namespace {

// Mapping: one lane per cell (row, node), cells in row-major order, so lane l of a wave holds cell base + l and both
// stores of a wave are contiguous along the node axis and across rows: 512 B of mass and 256 B of succ per wave
// instruction whatever N is (k_unstable's wave per state would leave 36 of 64 lanes idle at N = 28). A wave then
// covers at most ceil(64 / N) + 1 rows; each lane loads its own row's W words, which for the lanes of one row is
// one address. The image is staged in LDS as in k_unstable. A lane whose mass is 0 makes no probe.
template <int W, int KIND>
__global__ __launch_bounds__(BLOCK) void k_stg_rows(StgArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    const uint32_t N = (uint32_t)a.L.n_nodes;
    uint32_t leaks = 0;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < a.n_cells; c += stride) {
        const uint32_t local = (uint32_t)c / N, i = (uint32_t)c - local * N;  // n_cells <= 2^31
        const uint32_t row = a.first_row + local;
        uint64_t s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = a.states[(uint64_t)row * W + k];
        const uint64_t m =
            edge_mass<KIND>([&](uint32_t j) { return getbit<W>(s, j); }, i, a.first_node, lds, a.L);
        int32_t to = (int32_t)row;
        if (m) {
            const uint64_t bit = (uint64_t)1 << (i & 63u);
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] ^= bit & (uint64_t)(int64_t)(int32_t)lane_mask(i >> 6, (uint32_t)k);
            to = stateset_lookup<W>(s, a.set.meta, a.set.keys, a.set.slots);
            leaks += to < 0 ? 1u : 0u;
        }
        a.mass[c] = m;
        a.succ[c] = to;
    }
    // the leak tally: summed over the wave first (every lane is here: the cell loop has ended), one add per wave
    for (int d = 32; d >= 1; d >>= 1) leaks += __shfl_xor(leaks, d);
    if ((threadIdx.x & 63u) == 0u && leaks)
        __hip_atomic_fetch_add(a.leaks, (unsigned long long)leaks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// ------------------------------------------------------------------ dispatch
void* stg_rows_kernel(int W, int kind) {
    if (kind == KIND_PREDICTOR_MIX)
        return by_words<MAX_WORDS>(W, [](auto w) { return (void*)k_stg_rows<w, KIND_PREDICTOR_MIX>; });
    if (kind == KIND_PROB_TABLE)
        return by_words<MAX_WORDS>(W, [](auto w) { return (void*)k_stg_rows<w, KIND_PROB_TABLE>; });
    return nullptr;
}

int launch_stg_rows(void* kernel, const StgArgs& a, int grid, void* stream) {
    StgArgs c = a;
    return launch(kernel, grid, BLOCK, a.L.bytes, stream, &c);
}

int max_blocks_stg_rows(void* kernel, uint32_t image_bytes, int* blocks_per_cu) {
    return occupancy(kernel, BLOCK, image_bytes, blocks_per_cu);
}

}  // namespace pbn
