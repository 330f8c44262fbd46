// pbn_census.hip -- the state census: every env walks n_updates updates and counts the full (or projected) state it
// is in at the sample points, in an exact device table of visit counts. DESIGN.md §15.
//
// Reference semantics implemented (file:line in the reference):
//   k_census  statistical_attractors pbn_target.py:538-560, pbn_target_multi.py:465-487: `state_log[tuple(state)] += 1`
//             before every step of every reset's trajectory. The trajectories are the batch's own: update i of the call
//             is the draw pbn_step makes for update `update + i` of the env (step_words), so the state after the call is
//             bit for bit pbn_step(n_updates)'s.
#include <hip/hip_runtime.h>

#include "pbn_device.hpp"
#include "pbn_lane_env.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"
#include "pbn_census.hpp"

namespace pbn {

// The lane-per-env shape of pbn_lane_env.hpp, planes at L.bytes. The round loop is uniform -- every lane runs
// n_updates rounds -- so the round counter, the Philox counter words and the sample-point test stay scalar.
//
// The pending run (CensusRun) is what keeps the table off the hot path: an async update leaves the state as it was
// most of the time, and a sample point whose key equals the last one only bumps a register. Memory is touched when
// the key changes (one add of the finished run, one find-or-insert of the new key) and once at the end of the env.
template <int W, int KIND>
__global__ __launch_bounds__(BLOCK) void k_census(CensusArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const Plane P = lane_env_begin(lds, a.img, a.L, a.L.bytes);
    const uint32_t N = (uint32_t)a.L.n_nodes;
    uint64_t lane_dropped = 0, lane_adds = 0;
    uint32_t spare = CENSUS_NONE;  // a reserved entry this lane did not publish, kept for its next insert
    for (uint64_t e : lane_envs(a.B)) {
        uint64_t s0[W], s[W], key[W];
        load_state<W>(a.state + e * W, s0);
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = s0[k];
        to_plane<W>(P, s);
        const uint64_t g = a.env_base + e;
        CensusRun<W> run;
#pragma unroll
        for (int k = 0; k < W; ++k) run.key[k] = 0;
        run.entry = CENSUS_NONE;
        run.pending = 0u;
        CensusSampler sample{a.first, a.stride};
        if (sample.hit(0u)) {  // the state as loaded (the reference logs before it steps)
#pragma unroll
            for (int k = 0; k < W; ++k) key[k] = s[k] & a.mask[k];
            census_visit<W>(a, run, key, spare, lane_dropped, lane_adds);
        }
        for (uint32_t i = 0; i < a.n_updates; ++i) {
            uint32_t nw, cw;
            step_words(a.seed, a.update + i, g, nw, cw);
            const uint32_t node = philox_node<KIND>(nw, N);
            uint32_t changed;
            if constexpr (KIND == KIND_PREDICTOR_MIX)
                changed = predictor_update_lds(P, node, u32_k53(cw), lds, a.L);
            else
                changed = table_update_lds(P, node, u32_k53(cw), lds, a.L);
            xor_bit<W>(s, node, changed != 0u);
            if (sample.hit(i + 1u)) {
#pragma unroll
                for (int k = 0; k < W; ++k) key[k] = s[k] & a.mask[k];
                census_visit<W>(a, run, key, spare, lane_dropped, lane_adds);
            }
        }
        census_flush<W>(a, run, lane_dropped, lane_adds);
        store_if_changed<W>(a.state + e * W, s, s0);
    }
    if (spare != CENSUS_NONE) census_retire(a, spare);
    // the two tallies: summed over the wave first (every lane is here: the env loop has ended), one add per wave
    for (int d = 32; d >= 1; d >>= 1) {
        lane_dropped += __shfl_xor(lane_dropped, d);
        lane_adds += __shfl_xor(lane_adds, d);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (lane_dropped) __hip_atomic_fetch_add(a.dropped, (unsigned long long)lane_dropped, KEYTABLE_RLX, KEYTABLE_AGENT);
        if (lane_adds) __hip_atomic_fetch_add(a.adds, (unsigned long long)lane_adds, KEYTABLE_RLX, KEYTABLE_AGENT);
    }
}

// ------------------------------------------------------------------ dispatch
void* census_kernel(int W, int kind) {
    if (kind == KIND_PREDICTOR_MIX)
        return by_words<8>(W, [](auto w) { return (void*)k_census<w, KIND_PREDICTOR_MIX>; });
    if (kind == KIND_PROB_TABLE)
        return by_words<8>(W, [](auto w) { return (void*)k_census<w, KIND_PROB_TABLE>; });
    return nullptr;
}

}  // namespace pbn
