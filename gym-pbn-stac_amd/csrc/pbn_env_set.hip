// pbn_env_set.hip -- the until-attractor multi-flip env over an exact labelled state set: k_env's env step with
// "attracting" read as "member of the set", a target label per env, and the reset that draws from a per-env source
// attractor. DESIGN.md §14.
//
// Reference semantics implemented (file:line in the reference):
//   k_env_set        PBNTargetMultiEnv.step pbn_target_multi.py:119-154, with `tuple(state) in self.attracting_states`
//                    (:437-455, :489-492) as the lookup in a state set labelled by attractor, and the target as the
//                    attractor drawn per episode (`target_attractor_id`, :232-235) instead of all_attractors[-1][0]
//   k_env_set_reset  a state of attractor `state_attractor_id` (:232-249), or of the one table of states the PBN-v0
//                    env resets from (PBN.reset pbn.py:96-119); the draw is this library's own Philox stream
//                    (STREAM_TENV_RESET)
// Per env the step is oracle/pbn_oracle.c orc_env_step_multi in Philox mode: the draws are k_env's (STREAM_ENV, counter
// {used >> 1, env call count, global env id}), so a call interleaves with pbn_env_step_multi_device calls.
#include <hip/hip_runtime.h>

#include "pbn_env_device.hpp"
#include "pbn_lane_env.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"
#include "pbn_stateset.hpp"

namespace pbn {

// The lane-per-env shape of pbn_lane_env.hpp, planes at L.bytes, with ragged inner updates: the update index `used`
// is wave-uniform, so the Philox counter word used >> 1 and the choice of the call's half stay scalar.
//
// The membership test costs a table probe only when it can succeed and can differ from the last one:
//   hull     a state that differs from every member in a node all members agree on is no member (two ANDs and an
//            XOR per word against scalar operands, no memory touched);
//   skip     an update that changes nothing leaves a state that was tested after the previous update. That holds
//            from update 3 on only: after update 1 the SNAPSHOT was tested (pbn_target_multi.py:134), not the state,
//            so update 2 looks up whether or not it changed anything.
// An env with an invalid action row never goes live: state, n_steps and outputs untouched, the sticky flag set (what
// k_env does with the same row).
template <int W, int KIND>
__global__ __launch_bounds__(BLOCK) void k_env_set(EnvSetArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const Plane P = lane_env_begin(lds, a.img, a.L, a.L.bytes);
    const uint32_t N = (uint32_t)a.L.n_nodes;
    uint64_t hall[W], hany[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        hall[k] = a.hull_all[k];
        hany[k] = a.hull_any[k];
    }
    auto member = [&](const uint64_t (&x)[W]) -> int32_t {
        if (stateset_hull_rejects<W>(x, hall, hany)) return -1;
        return stateset_lookup<W>(x, a.set.meta, a.set.keys, a.set.slots);
    };
    const bool snap_first = a.first_tested == 0;
    for (uint64_t e : lane_envs(a.B)) {
        uint64_t s0[W], s[W], o[W];
        load_state<W>(a.state + e * W, s0);
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = s0[k];
        bool bad = false;
        const int n_act = apply_actions<W>(s, a.actions + e * (uint64_t)a.A, a.A, a.offset, a.dedup, (int32_t)N, &bad);
        if (bad) atomicOr(a.error, 1);  // reference raises ValueError; the env step is skipped
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] = s[k];  // :133 the observation before the update
        to_plane<W>(P, s);
        const uint64_t g = a.env_base + e;
        uint32_t n_used = 0;
        int32_t label = -1;
        bool live = !bad;
        for (uint32_t used = 0; rounds_left(used, a.update_cap, live); ++used) if (live) {
            uint32_t w[4];
            philox_draw(a.seed, used >> 1, a.call_idx, g, STREAM_ENV, w);
            const bool odd = (used & 1u) != 0u;
            const uint32_t i = philox_node<KIND>(odd ? w[2] : w[0], N);
            const uint64_t k53 = u32_k53(odd ? w[3] : w[1]);
            uint32_t changed;
            if constexpr (KIND == KIND_PREDICTOR_MIX)
                changed = predictor_update_lds(P, i, k53, lds, a.L);
            else
                changed = table_update_lds(P, i, k53, lds, a.L);
            xor_bit<W>(s, i, changed != 0u);
            n_used = used + 1u;
            if (used == 0u && snap_first)
                label = member(o);  // :134 the first update is never tested: the test is on the snapshot
            else if (changed != 0u || used < 2u || a.always_lookup != 0)
                label = member(s);
            live = label < 0;
        }
        if (bad) continue;
        store_if_changed<W>(a.state + e * W, s, s0);
        const int64_t nst = a.n_steps[e] + 1;  // :123
        a.n_steps[e] = nst;
        // what was tested last: the snapshot up to update 1, the state from update 2 on
        if (!(n_used <= 1u && snap_first)) {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = s[k];
        }
        store_state<W>(a.obs + e * W, o);
        const int32_t target = a.target_labels ? a.target_labels[e] : a.target_label;
        const bool term = label >= 0 && label == target;
        a.reward[e] = (term ? a.reward_success : 0) - a.action_cost * n_act;  // :218-222
        a.flags[e] = (uint8_t)((term ? 1 : 0) | (nst == a.horizon ? 2 : 0) | (label < 0 ? 4 : 0));
        a.n_updates[e] = n_used;
        if (a.labels) a.labels[e] = label;
    }
}

// ------------------------------------------------------------------ reset
// Envs with mask[e] != 0 (null: all) take a row of their source attractor: row_off[src] + mulhi(w[0], rows of src).
// A null row_off is one attractor of n_rows rows (the PBN-v0 env's table of attracting states); a null n_steps is
// not written.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_env_set_reset(EnvSetResetArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.B) return;
    if (a.mask && !a.mask[e]) return;
    uint32_t lo = 0, n = a.n_rows;
    if (a.row_off) {
        const int32_t src = a.source_labels ? a.source_labels[e] : a.source_label;
        n = 0;
        if (src >= 0 && src < a.n_labels) {
            lo = a.row_off[src];
            n = a.row_off[src + 1] - lo;
        }
    }
    if (n == 0u) {  // no such attractor, or an empty one: the env is left as it is
        atomicOr(a.error, 1);
        return;
    }
    uint32_t w[4];
    philox_draw(a.seed, 0u, a.reset_count, a.env_base + e, STREAM_TENV_RESET, w);
    const uint32_t row = lo + __umulhi(w[0], n);
    uint64_t s[W];
    load_state<W>(a.rows + (uint64_t)row * W, s);
    if (a.clear_node0) s[0] &= ~(uint64_t)1;  // pbn.py:118 state[0] = 0
    store_state<W>(a.state + e * W, s);
    if (a.n_steps) a.n_steps[e] = 0;
}

// ------------------------------------------------------------------ dispatch
void* env_set_kernel(int W, int kind) {
    if (kind == KIND_PREDICTOR_MIX)
        return by_words<8>(W, [](auto w) { return (void*)k_env_set<w, KIND_PREDICTOR_MIX>; });
    if (kind == KIND_PROB_TABLE)
        return by_words<8>(W, [](auto w) { return (void*)k_env_set<w, KIND_PROB_TABLE>; });
    return nullptr;
}

int launch_env_set_reset(int W, const EnvSetResetArgs& a, void* stream) {
    EnvSetResetArgs c = a;
    const int grid = (int)((a.B + BLOCK - 1) / BLOCK);
    return launch(by_words<8>(W, [](auto w) { return (void*)k_env_set_reset<w>; }), grid, BLOCK, 0, stream, &c);
}

}  // namespace pbn
