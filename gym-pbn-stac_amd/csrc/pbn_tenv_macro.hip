// pbn_tenv_macro.hip -- the macro-action envs of truth-table networks on the device: one launch runs every env's
// whole macro step, up to t_max rounds of flip + PBN.step + target lookup + reward. DESIGN.md §13.
//
// Reference semantics implemented (file:line in the reference):
//   TENV_MACRO_INTERVAL  PBNSampledDataEnv.step sampled_data.py:52-88: `interval` rounds, the rewards summed
//   TENV_MACRO_TRIGGER   PBNSelfTriggeringEnv.step self_triggering.py:56-92: rounds until uniform(0, 1) <= prob or
//                        T of them, the rewards discounted by gamma ** i
// Both flip node `action - 1` (sampled_data.py:62, self_triggering.py:67; PBN-v0 flips node `action`) before every
// round, and both take PBNEnv._get_reward (pbn_env.py:156-188) of every round's state.
#include <hip/hip_runtime.h>

#include "pbn_lane_env.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"
#include "pbn_stateset.hpp"

namespace pbn {

// total + g * r as the reference computes it: one IEEE multiply, one IEEE add. A fused multiply-add rounds once and
// would differ from Python's `total_reward += (self.gamma ** i) * reward` in the last bit.
__device__ __forceinline__ double discounted_add(double total, double g, int32_t r) {
#pragma clang fp contract(off)
    const double p = g * (double)r;
    return total + p;
}

// The lane-per-env shape of pbn_lane_env.hpp, planes at L.plane_off, with ragged inner rounds: round i is update
// `update + i` of every env, so update + i, the Philox counter words and gpow[i] stay scalar.
// An env with an invalid action or limit never goes live: state and outputs untouched, the sticky flag set.
//
// The draws are philox_draw's: the compiler hoists their round keys out of the round loop and keeps the SGPRs that
// no longer fit in VGPR lanes (no scratch). philox_draw_sk removes those spills and measured slower.
template <int W, int MODE>
__global__ __launch_bounds__(BLOCK) void k_tenv_macro(TenvMacroArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const Plane P = lane_env_begin(lds, a.img, a.L, a.L.plane_off);
    const uint32_t N = (uint32_t)a.L.n_nodes;
    const uint32_t lim_max = MODE == TENV_MACRO_INTERVAL ? a.t_max : (uint32_t)TENV_MACRO_MAX_PROB;
    for (uint64_t e : lane_envs(a.B)) {
        uint64_t s0[W], s[W];
        load_state<W>(a.state + e * W, s0);
        const int32_t act = a.actions[e];
        const uint32_t lim = (uint32_t)a.limit[e];
        const uint64_t g = a.env_base + e;
        const bool valid = (uint32_t)act <= N && lim - 1u < lim_max;  // negative values too
        if (!valid) atomicOr(a.error, 1);
        uint64_t thr = 0;
        if constexpr (MODE == TENV_MACRO_TRIGGER) thr = a.stop_thr[valid ? lim : 0u];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = s0[k];
        to_plane<W>(P, s);
        // the flip of every round: node act - 1, as a mask over the state words and over its plane dword
        const uint32_t fn = act > 0 ? (uint32_t)act - 1u : 0u;
        const uint64_t fm = act > 0 ? 1ull << (fn & 63u) : 0ull;
        const uint32_t fm32 = act > 0 ? 1u << (fn & 31u) : 0u;
        const int32_t miss = -(a.step_cost + (act != 0 ? a.action_cost : 0));
        int32_t total_i = 0, label = -1, first_hit = -1, rounds = 0;
        double total_f = 0.0;
        bool live = valid;
        for (uint32_t i = 0; rounds_left(i, a.t_max, live); ++i) if (live) {
            const uint64_t u = a.update + i;
            uint32_t nw, cw;
            step_words(a.seed, u, g, nw, cw);
            const uint32_t node = philox_node<KIND_PROB_TABLE>(nw, N);
            // the two word selects are written out here, not xor_bit: in this loop xor_bit's and-ed condition selects
            // other instructions than the nested select, and measured 0.6 us per macro step slower at 65,536 envs
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] ^= (uint32_t)k == (fn >> 6) ? fm : 0ull;
            P.put(fn >> 5, P.get(fn >> 5) ^ fm32);
            const uint32_t y = table_eval_lds(P, node, u32_k53(cw), lds, a.L);
            const uint32_t self = P.get(node >> 5);
            const uint32_t um32 = (y ^ (self >> (node & 31u))) & 1u ? 1u << (node & 31u) : 0u;
            P.put(node >> 5, self ^ um32);
            const uint64_t um = um32 ? 1ull << (node & 63u) : 0ull;
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] ^= (uint32_t)k == (node >> 6) ? um : 0ull;
            label = stateset_lookup<W>(s, a.target.meta, a.target.keys, a.target.slots);
            const bool term = label >= 0;
            const int32_t r = term ? a.reward_target : miss;
            first_hit = term && first_hit < 0 ? (int32_t)i : first_hit;
            rounds = (int32_t)i + 1;
            if constexpr (MODE == TENV_MACRO_INTERVAL) {
                total_i += r;
                live = i + 1u < lim;
            } else {
                total_f = discounted_add(total_f, a.gpow[i], r);
                uint32_t w[4];
                philox_draw(a.seed, (uint32_t)u, (uint32_t)(u >> 32), g, STREAM_TENV_TRIGGER, w);
                live = !(k53_of(w[0], w[1]) <= thr || i + 1u == a.t_max);
            }
        }
        if (!valid) continue;
        store_if_changed<W>(a.state + e * W, s, s0);
        if (a.obs) store_state<W>(a.obs + e * W, s);
        if constexpr (MODE == TENV_MACRO_INTERVAL)
            a.reward_i32[e] = total_i;
        else
            a.reward_f64[e] = total_f;
        a.flags[e] = label >= 0 ? (uint8_t)1 : (uint8_t)0;  // PBN_FLAG_TERMINATED: the last round's; never truncated
        if (a.interval) a.interval[e] = rounds;
        if (a.first_hit) a.first_hit[e] = first_hit;
        if (a.labels) a.labels[e] = label;
    }
}

// ------------------------------------------------------------------ dispatch
void* tenv_macro_kernel(int W, int mode) {
    if (mode == TENV_MACRO_INTERVAL)
        return by_words<8>(W, [](auto w) { return (void*)k_tenv_macro<w, TENV_MACRO_INTERVAL>; });
    if (mode == TENV_MACRO_TRIGGER)
        return by_words<8>(W, [](auto w) { return (void*)k_tenv_macro<w, TENV_MACRO_TRIGGER>; });
    return nullptr;
}

}  // namespace pbn
