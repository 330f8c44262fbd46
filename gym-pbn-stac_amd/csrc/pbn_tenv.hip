// pbn_tenv.hip -- the PBN-v0 env (truth-table networks) on the device: membership in an exact state set and the
// fused env step. DESIGN.md §12. Its reset is k_env_set_reset (pbn_env_set.hip) over one attractor.
//
// Reference semantics implemented (file:line in the reference):
//   k_tenv_step   PBNEnv.step pbn_env.py:125-154 (flip node `action` :141-142, one PBN.step pbn.py:129-133) and
//                 PBNEnv._get_reward :156-188 (membership in target_nodes, expanded at :57-59)
//   k_set_lookup  `state in set` for a whole batch (the host envs' Python sets of tuples)
// The set's layout and walk are defined once, in pbn_stateset.hpp, for these kernels and the host.
#include <hip/hip_runtime.h>

#include "pbn_lane_env.hpp"
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
// The lane-per-env shape of pbn_lane_env.hpp, planes at L.plane_off as k_step's truth-table path. Per env: flip node
// a (a != 0), one PBN.step update with the draw pbn_step makes for update `update` of env env_base + e, store the
// state if either changed it, then the target lookup, reward and flags.
// An env whose action names no node is skipped whole (state and outputs untouched) and noted in *error.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_tenv_step(TenvArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const Plane P = lane_env_begin(lds, a.img, a.L, a.L.plane_off);
    const uint32_t N = (uint32_t)a.L.n_nodes;
    for (uint64_t e : lane_envs(a.B)) {
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
        xor_bit<W>(s, av, av != 0u);
        to_plane<W>(P, s);
        const uint32_t y = table_eval_lds(P, i, u32_k53(cw), lds, a.L);
        const bool moved = y != P.bit(i);
        xor_bit<W>(s, i, moved);
        if (av != 0u || moved) store_state<W>(a.state + e * W, s);
        if (a.obs) store_state<W>(a.obs + e * W, s);
        const int32_t label = stateset_lookup<W>(s, a.target.meta, a.target.keys, a.target.slots);
        const bool term = label >= 0;
        a.reward[e] = term ? a.reward_target : -(a.step_cost + (av != 0u ? a.action_cost : 0));
        a.flags[e] = term ? (uint8_t)1 : (uint8_t)0;  // PBN_FLAG_TERMINATED; PBN-v0 never truncates
        if (a.labels) a.labels[e] = label;
    }
}

// ------------------------------------------------------------------ dispatch
int launch_set_lookup(int W, const SetLookupArgs& a, void* stream) {
    SetLookupArgs c = a;
    const int grid = (int)((a.B + BLOCK - 1) / BLOCK);
    return launch(by_words<8>(W, [](auto w) { return (void*)k_set_lookup<w>; }), grid, BLOCK, 0, stream, &c);
}

void* tenv_step_kernel(int W) {
    return by_words<8>(W, [](auto w) { return (void*)k_tenv_step<w>; });
}

// The one launcher and occupancy query of the lane-per-env kernels, whichever file picked `kernel`.
int launch_lane_env(void* kernel, int W, uint32_t plane_off, int grid, void* stream, void* args) {
    return launch(kernel, grid, BLOCK, step_lds_bytes(W, plane_off, BLOCK), stream, args);
}

int max_blocks_lane_env(void* kernel, int W, uint32_t plane_off, int* blocks_per_cu) {
    return occupancy(kernel, BLOCK, step_lds_bytes(W, plane_off, BLOCK), blocks_per_cu);
}

}  // namespace pbn
