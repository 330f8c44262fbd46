// pbn_tenv.hip -- the PBN-v0 env (truth-table networks) on the device: membership in an exact state set, the
// fused env step and the reset over a table of states. DESIGN.md §12.
//
// Reference semantics implemented (file:line in the reference):
//   k_tenv_step   PBNEnv.step pbn_env.py:125-154 (flip node `action` :141-142, one PBN.step pbn.py:129-133) and
//                 PBNEnv._get_reward :156-188 (membership in target_nodes, expanded at :57-59)
//   k_tenv_reset  a state of the attracting set, node 0 cleared (PBN.reset pbn.py:96-119); the draw is this
//                 library's own Philox stream (STREAM_TENV_RESET)
//   k_set_lookup  `state in set` for a whole batch (the host envs' Python sets of tuples)
// The set's layout and walk are defined once, in pbn_stateset.hpp, for these kernels and the host.
#include <hip/hip_runtime.h>

#include "pbn_device.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"
#include "pbn_stateset.hpp"

namespace pbn {

// ------------------------------------------------------------------ membership
// One lane per env. The set is read-only for the whole launch: plain loads, no atomics. Lanes of a wave walk
// independently (a walk is one probe for most states at load <= 1/2); the wave pays its longest walk.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_set_lookup(SetLookupArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.B) return;
    uint64_t s[W];
    load_state<W>(a.words + e * W, s);
    a.labels[e] = stateset_lookup<W>(s, a.set.meta, a.set.keys, a.set.slots);
}

// ------------------------------------------------------------------ fused env step
// LDS per workgroup: [network image][state planes], as k_step's truth-table path. One lane per env, envs taken in
// a grid-stride loop by a grid sized to what is resident, so the image is staged once per workgroup and not once
// per 256 envs. Per env: flip node a (a != 0), one PBN.step update with the draw pbn_step makes for update
// `update` of env env_base + e, store the state if either changed it, then the target lookup, reward and flags.
// An env whose action names no node is skipped whole (state and outputs untouched) and noted in *error.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_tenv_step(TenvArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    const Plane P{reinterpret_cast<uint32_t*>(lds + a.L.plane_off) + threadIdx.x};
    const uint32_t N = (uint32_t)a.L.n_nodes;
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < a.B; e += stride) {
        uint64_t s[W];
        load_state<W>(a.state + e * W, s);
        const int32_t act = a.actions[e];
        // the draw depends on (seed, update, env id) only: computed while the loads are in flight
        uint32_t nw, cw;
        step_words(a.seed, a.update, a.env_base + e, nw, cw);
        const uint32_t i = philox_node<KIND_PROB_TABLE>(nw, N);
        if ((uint32_t)act >= N) {  // negative values too
            atomicOr(a.error, 1);
            continue;
        }
        const uint32_t av = (uint32_t)act;
        const uint64_t am = av ? 1ull << (av & 63u) : 0ull;
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] ^= (uint32_t)k == (av >> 6) ? am : 0ull;
        to_plane<W>(P, s);
        const uint32_t y = table_eval_lds(P, i, u32_k53(cw), lds, a.L);
        const uint32_t old = P.bit(i);
        const uint64_t um = y != old ? 1ull << (i & 63u) : 0ull;
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] ^= (uint32_t)k == (i >> 6) ? um : 0ull;
        if (av != 0u || um != 0ull) store_state<W>(a.state + e * W, s);
        if (a.obs) store_state<W>(a.obs + e * W, s);
        const int32_t label = stateset_lookup<W>(s, a.target.meta, a.target.keys, a.target.slots);
        const bool term = label >= 0;
        a.reward[e] = term ? a.reward_target : -(a.step_cost + (av != 0u ? a.action_cost : 0));
        a.flags[e] = term ? (uint8_t)1 : (uint8_t)0;  // PBN_FLAG_TERMINATED; PBN-v0 never truncates
        if (a.labels) a.labels[e] = label;
    }
}

// ------------------------------------------------------------------ reset
// Envs with mask[e] != 0 (null: all) take row mulhi(w[0], n_states) of `states`, node 0 cleared.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_tenv_reset(TenvResetArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.B) return;
    if (a.mask && !a.mask[e]) return;
    uint32_t w[4];
    philox_draw(a.seed, 0u, a.reset_count, a.env_base + e, STREAM_TENV_RESET, w);
    const uint32_t row = __umulhi(w[0], a.n_states);
    uint64_t s[W];
    load_state<W>(a.states + (uint64_t)row * W, s);
    s[0] &= ~(uint64_t)1;  // pbn.py:118 state[0] = 0
    store_state<W>(a.state + e * W, s);
}

// ------------------------------------------------------------------ dispatch
static int grid_all(uint64_t items) { return (int)((items + BLOCK - 1) / BLOCK); }

int launch_set_lookup(int W, const SetLookupArgs& a, void* stream) {
    SetLookupArgs c = a;
    return launch(by_words<8>(W, [](auto w) { return (void*)k_set_lookup<w>; }), grid_all(a.B), BLOCK, 0, stream, &c);
}

static void* tenv_step_kernel(int W) {
    return by_words<8>(W, [](auto w) { return (void*)k_tenv_step<w>; });
}

int launch_tenv_step(int W, const TenvArgs& a, int grid, void* stream) {
    TenvArgs c = a;
    return launch(tenv_step_kernel(W), grid, BLOCK, step_lds_bytes(W, a.L.plane_off, BLOCK), stream, &c);
}

int max_blocks_tenv(int W, uint32_t image_bytes, int* blocks_per_cu) {
    return occupancy(tenv_step_kernel(W), BLOCK, step_lds_bytes(W, image_bytes, BLOCK), blocks_per_cu);
}

int launch_tenv_reset(int W, const TenvResetArgs& a, void* stream) {
    TenvResetArgs c = a;
    return launch(by_words<8>(W, [](auto w) { return (void*)k_tenv_reset<w>; }), grid_all(a.B), BLOCK, 0, stream, &c);
}

}  // namespace pbn
