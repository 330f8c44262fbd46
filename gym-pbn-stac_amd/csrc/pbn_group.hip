// pbn_group.hip -- group mode (G lanes per env): the env step k_env_grp and the rollout k_rollout_grp
// with the resolve machinery they share, reached from pbn_env.hip's and pbn_step.hip's dispatch through
// env_grp_kernel / rollout_grp_kernel. (One translation unit on purpose: compiled without k_env_grp
// beside it, k_rollout_grp<W, 4> and <W, 8> come out as different code -- tools/kernel_isa_diff.py.)
#include <hip/hip_runtime.h>

#include "pbn_device.hpp"
#include "pbn_env_device.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"

namespace pbn {

// ------------------------------------------------------------------ R6, group mode
// The same env step with G lanes per env: a block of G consecutive updates of one env is
// evaluated by the G lanes at once (parallel in time), so one env advances G updates per
// round trip instead of one. The draws of the block do not depend on the state (Philox
// counter = update index), so lane k knows its node i_k and predictor record up front;
// what it needs are the values of its 4 input nodes at time k, i.e. the output of the
// last update j < k in the block that wrote each input, or the block-start value. The
// writers are found from the byte-packed node list of the group; the outputs y_k are
// then the fixed point of y_k = tt_k(inputs from writers), a DAG of depth < G: every
// round that changes nothing is exact. Per-update mismatch deltas are prefix-summed
// across the group (packed byte counters, as in k_env), the first update whose counters
// hit a cube ends the env step, and the final writer of each node in the committed
// prefix sets its bit in the env's LDS row (ds_or / ds_and: distinct nodes, possibly one
// dword). Same Philox counters as k_env, so the results are bit-identical to lane mode.
//
// Used where the batch is small against the chip (BASELINE config 5: 131,072 envs per
// GPU): there lane mode is latency-bound on the tail of long until-attractor loops.
// Requirements: predictor mix, N <= 256 (byte-packed node list), fast byte counters.

template <int G>
__device__ __forceinline__ uint32_t grp_bcast(uint32_t v, uint32_t j) {
    static_assert(G == 2 || G == 4 || G == 8, "group size");
    if constexpr (G <= 4) {
        // quad_perm [j,j,j,j] (G == 2: lanes 0/1 and 2/3 of each quad form two groups)
        switch (j) {
            case 0: return G == 2 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xF, 0xF, false)   // [0,0,2,2]
                                  : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xF, 0xF, false);  // [0,0,0,0]
            case 1: return G == 2 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xF5, 0xF, 0xF, false)   // [1,1,3,3]
                                  : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x55, 0xF, 0xF, false);  // [1,1,1,1]
            case 2: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xAA, 0xF, 0xF, false);
            default: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xF, 0xF, false);
        }
    } else {
        // ds_swizzle bit-mask mode within 32 lanes: src = (lane & 0x18) | j
        switch (j) {
            case 0: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (0 << 5));
            case 1: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (1 << 5));
            case 2: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (2 << 5));
            case 3: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (3 << 5));
            case 4: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (4 << 5));
            case 5: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (5 << 5));
            case 6: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (6 << 5));
            default: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x18 | (7 << 5));
        }
    }
}

// value of lane (lane - n) of the same 16-lane row, 0 where that lane is outside the row
template <int N_>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x110 + N_, 0xF, 0xF, true);
}

// 0x80 in every byte of v that is zero (exact, no false positives)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) {
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// Byte-packed node list of a group (G <= 8: two words). match(x) -> 0x80 per byte j with i_j == x.
template <int G>
struct GroupNodes {
    uint32_t lo = 0, hi = 0;
    __device__ __forceinline__ explicit GroupNodes(uint32_t i) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const uint32_t v = grp_bcast<G>(i, (uint32_t)j);
            if (j < 4)
                lo |= v << (8 * j);
            else
                hi |= v << (8 * (j - 4));
        }
        if (G < 4) lo |= 0xFFFFFFFFu << (8 * G);  // unused bytes never match (node < 256)
        if (G <= 4) hi = 0xFFFFFFFFu;
    }
    // bytes j in [j0, j1) of the list equal to x, as a bit mask over j
    __device__ __forceinline__ uint32_t match(uint32_t x, uint32_t j0, uint32_t j1) const {
        const uint32_t xx = x * 0x01010101u;
        const uint32_t zl = zero_bytes(lo ^ xx), zh = zero_bytes(hi ^ xx);
        // compress 0x80 per byte to one bit per byte
        uint32_t m = ((zl >> 7) & 1u) | ((zl >> 14) & 2u) | ((zl >> 21) & 4u) | ((zl >> 28) & 8u);
        if (G > 4) m |= (((zh >> 7) & 1u) | ((zh >> 14) & 2u) | ((zh >> 21) & 4u) | ((zh >> 28) & 8u)) << 4;
        const uint32_t rng = ((1u << j1) - 1u) & ~((1u << j0) - 1u);
        return m & rng;
    }
};

// One block of G consecutive updates of a group's env, lane k holding update k: node i, its
// predictor record and the block-start values v of its operands (in0, in1, in2, self). Returns
// y (node i's new value) and old (its value right before update k), exact in every lane.
template <int G>
struct GrpBlock {
    uint32_t y = 0, old = 0;
    uint32_t ip = 0;  // G == 2: the partner lane's node
    GroupNodes<G> nodes;
    __device__ __forceinline__ explicit GrpBlock(uint32_t i) : nodes(G == 2 ? 0u : i) {}
    // update k is the last writer of node i among the first n_done updates of the block
    __device__ __forceinline__ bool last(uint32_t i, uint32_t k, uint32_t n_done) const {
        return G == 2 ? (k == 1 || n_done < 2 || ip != i) : nodes.match(i, k + 1, n_done) == 0u;
    }
};

template <int G>
__device__ __forceinline__ GrpBlock<G> grp_resolve(uint32_t i, uint64_t rec, const uint32_t (&in)[4],
                                                   const uint32_t (&v)[4], uint32_t k, uint32_t gbase,
                                                   uint32_t gmask) {
    GrpBlock<G> b(i);
    const uint32_t tt = (uint32_t)(rec >> 48);
    auto tt_of = [&](const uint32_t (&x)[4]) { return (tt >> ((x[0] << 3) | (x[1] << 2) | (x[2] << 1) | x[3])) & 1u; };
    if constexpr (G == 2) {
        // pairs: lane 1 depends on lane 0 only where an input is lane 0's node
        b.ip = (uint32_t)__builtin_amdgcn_mov_dpp((int)i, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
        const uint32_t y0 = tt_of(v);  // exact in lane 0
        const uint32_t yb = (uint32_t)__builtin_amdgcn_mov_dpp((int)y0, 0xA0, 0xF, 0xF, false);  // [0,0,2,2]
        uint32_t x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = (k == 1 && in[q] == b.ip) ? yb : v[q];
        b.y = tt_of(x);
        b.old = x[3];
    } else {
        int32_t wr[4];  // last writer j < k of each input, or -1
        bool dep = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t mm = b.nodes.match(in[q], 0, k);
            wr[q] = mm ? 31 - __clz((int)mm) : -1;
            dep |= mm != 0;
        }
        auto eval = [&](uint32_t Y, uint32_t* self_old) {
            uint32_t x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = wr[q] >= 0 ? (Y >> wr[q]) & 1u : v[q];
            *self_old = x[3];
            return tt_of(x);
        };
        b.y = eval(0u, &b.old);  // exact where no input has an in-block writer
        if (__ballot(dep) != 0) {
            // after round r lanes 0..r are exact, so round G - 1 at the latest changes nothing;
            // a round that changes nothing has `old` computed from the final outputs
#pragma unroll 1
            for (int r = 0; r < G; ++r) {
                const uint32_t Y = (uint32_t)(__ballot(b.y != 0u) >> gbase) & gmask;
                const uint32_t yn = eval(Y, &b.old);
                if (__ballot(yn != b.y) == 0) break;
                b.y = yn;
            }
        }
    }
    return b;
}
template <int W, int G>
__global__ __launch_bounds__(BLOCK) void k_env_grp(EnvArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    const uint32_t N = (uint32_t)a.L.n_nodes;
    const uint64_t* cubes = reinterpret_cast<const uint64_t*>(lds + a.off_cubes);
    const uint64_t* target = reinterpret_cast<const uint64_t*>(lds + a.off_target);
    const uint2* ndelta = reinterpret_cast<const uint2*>(lds + a.off_ndelta);
    const uint64_t* recs = reinterpret_cast<const uint64_t*>(lds + a.L.off_rec);
    const int32_t H = a.n_cubes;
    const uint32_t lane = __lane_id();
    const uint32_t k = lane & (G - 1);                     // position in the group = update slot
    const uint32_t gbase = lane & ~(uint32_t)(G - 1);
    const uint32_t gmask = (1u << G) - 1u;
    // the env's 2W dwords, one row per group (bank = group * 2W + dword: 8 groups of W = 4 fill 64 banks)
    uint32_t* row = reinterpret_cast<uint32_t*>(lds + a.off_gen) + (threadIdx.x / G) * (2 * W);

    // per-env registers, identical in every lane of the group
    int64_t e = -1;
    uint32_t t = 0;  // env step of this launch
    bool exhausted = false;
    uint64_t o0[W];
    uint32_t m_lo = 0, m_hi = 0, used = 0;
    bool hit0 = false;
    int64_t nst = 0;
    int n_act = 0;
    uint64_t gid = 0;

    // step t (or the first later step with a valid action row) of env e from state s; with no
    // step left, write the env back and free the group (as begin_steps in k_env)
    auto begin_steps = [&](uint64_t (&s)[W]) {
        for (; t < a.n_calls; ++t) {
            uint64_t f[W];
#pragma unroll
            for (int q = 0; q < W; ++q) f[q] = s[q];
            bool bad = false;
            n_act = apply_actions<W>(f, a.actions + ((uint64_t)t * a.B + (uint64_t)e) * (uint64_t)a.A, a.A,
                                     a.offset, a.dedup, (int32_t)N, &bad);
            if (bad) {  // reference raises ValueError; this env step is skipped, the env left untouched
                if (k == 0) atomicOr(a.error, 1);
                continue;
            }
            ++nst;  // :123
#pragma unroll
            for (int q = 0; q < W; ++q) o0[q] = f[q];  // :133 observation before the update
            if (k == 0) {
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    row[2 * q] = (uint32_t)f[q];
                    row[2 * q + 1] = (uint32_t)(f[q] >> 32);
                }
            }
            uint32_t m[2] = {0x01010101u, 0x01010101u};  // unused cubes: never zero
            for (int32_t h = 0; h < H; ++h) {
                const uint32_t c = cube_mismatch<W>(f, cubes + (uint64_t)h * 2 * W);
                const uint32_t sh = 8u * (uint32_t)(h & 3);
                m[h >> 2] = (m[h >> 2] & ~(0xFFu << sh)) | (c << sh);
            }
            m_lo = m[0];
            m_hi = m[1];
            hit0 = (has_zero_byte(m_lo) | has_zero_byte(m_hi)) != 0u;
            used = 0;
            return;
        }
        if (k == 0) {
            store_state<W>(a.state + (uint64_t)e * W, s);
            a.n_steps[e] = nst;
        }
        e = -1;
    };

    for (;;) {
        // ---- refill groups without an env: one atomic per wave, ranks over the groups' leaders
        const bool need = e < 0 && !exhausted;
        const uint64_t need_lead = __ballot(need && k == 0);
        if (need_lead) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)need_lead) - 1u;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(a.counter, (unsigned long long)__popcll(need_lead));
            base = __shfl(base, (int)leader);
            if (need) {
                const uint64_t ne = base + (uint64_t)__popcll(need_lead & ((1ull << gbase) - 1ull));
                if (ne >= a.B) {
                    exhausted = true;
                } else {
                    uint64_t s[W];
                    load_state<W>(a.state + ne * W, s);  // every lane of the group: one request
                    e = (int64_t)ne;
                    gid = a.env_base + ne;
                    t = 0;
                    nst = a.n_steps[ne];
                    begin_steps(s);
                }
            }
            wave_sync();
        }
        if (__ballot(e >= 0) == 0) {
            if (__ballot(!exhausted) == 0) break;
            continue;
        }

        // ---- one block: update used + k of this group's env in lane k (idle groups compute junk)
        // (a block starts at a multiple of G: lanes 2m and 2m + 1 share Philox call (used >> 1) + m)
        uint32_t w4[4];
        philox_draw(a.seed, (used + k) >> 1, a.call_idx + t, gid, STREAM_ENV, w4);
        const uint32_t i = philox_node<KIND_PREDICTOR_MIX>((k & 1u) ? w4[2] : w4[0], N);
        const uint64_t rec = recs[i * a.L.pmax + predictor_choice(i, u32_k53((k & 1u) ? w4[3] : w4[1]), lds, a.L)];
        const uint2 nd = ndelta[i];
        const uint32_t in[4] = {(uint32_t)rec & 0xFFFFu, (uint32_t)(rec >> 16) & 0xFFFFu,
                                (uint32_t)(rec >> 32) & 0xFFFFu, i};
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (row[in[q] >> 5] >> (in[q] & 31u)) & 1u;  // block-start values
        const GrpBlock<G> blk = grp_resolve<G>(i, rec, in, v, k, gbase, gmask);
        const uint32_t y = blk.y, old = blk.old;
        // mismatch counters after each update of the block (inclusive prefix over the group)
        const bool changed = y != old;
        uint32_t dl = changed ? (y ? nd.x : 0u - nd.x) : 0u;
        uint32_t dh = changed ? (y ? nd.y : 0u - nd.y) : 0u;
        {
            uint32_t tl = row_shr<1>(dl), th = row_shr<1>(dh);
            dl += k >= 1 ? tl : 0u;
            dh += k >= 1 ? th : 0u;
            if constexpr (G >= 4) {
                tl = row_shr<2>(dl);
                th = row_shr<2>(dh);
                dl += k >= 2 ? tl : 0u;
                dh += k >= 2 ? th : 0u;
            }
            if constexpr (G >= 8) {
                tl = row_shr<4>(dl);
                th = row_shr<4>(dh);
                dl += k >= 4 ? tl : 0u;
                dh += k >= 4 ? th : 0u;
            }
        }
        const uint32_t ml = m_lo + dl, mh = m_hi + dh;
        const bool valid = used + k < a.update_cap;
        const bool hit = (used + k == 0 && !a.first_tested) ? hit0 : (has_zero_byte(ml) | has_zero_byte(mh)) != 0u;
        const uint32_t SM = (uint32_t)(__ballot(valid && hit) >> gbase) & gmask;
        const uint32_t VM = (uint32_t)(__ballot(valid) >> gbase) & gmask;
        const uint32_t n_done = SM ? (uint32_t)__ffs((int)SM) : (uint32_t)__popc(VM);
        const bool done = SM != 0u || used + n_done >= a.update_cap;
        const bool capped = SM == 0u;  // only meaningful when done
        // commit: the last writer of each node among the first n_done updates sets its bit
        const bool last = blk.last(i, k, n_done);
        if (e >= 0 && k < n_done && y != v[3] && last) {
            if (y)
                atomicOr(&row[i >> 5], 1u << (i & 31u));
            else
                atomicAnd(&row[i >> 5], ~(1u << (i & 31u)));
        }
        uint32_t nl, nh;  // counters after the last committed update
        if constexpr (G == 2) {
            const uint32_t l1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)ml, 0xF5, 0xF, 0xF, false);  // [1,1,3,3]
            const uint32_t h1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)mh, 0xF5, 0xF, 0xF, false);
            const uint32_t l0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)ml, 0xA0, 0xF, 0xF, false);  // [0,0,2,2]
            const uint32_t h0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)mh, 0xA0, 0xF, 0xF, false);
            nl = n_done == 2 ? l1 : l0;
            nh = n_done == 2 ? h1 : h0;
        } else {
            const uint32_t src = gbase + (n_done ? n_done - 1u : 0u);
            nl = (uint32_t)__shfl((int)ml, (int)src);
            nh = (uint32_t)__shfl((int)mh, (int)src);
        }
        if (e >= 0 && n_done) {
            m_lo = nl;
            m_hi = nh;
        }
        wave_sync();
        if (e < 0) continue;
        used += n_done;
        if (!done) continue;

        // ---- finish: outputs of step() (:148-154) into step t's slot (group leader), next step
        uint64_t s[W];
#pragma unroll
        for (int q = 0; q < W; ++q) s[q] = (uint64_t)row[2 * q] | ((uint64_t)row[2 * q + 1] << 32);
        if (k == 0) {
            uint64_t o[W];
#pragma unroll
            for (int q = 0; q < W; ++q) o[q] = (used <= 1 && !a.first_tested) ? o0[q] : s[q];
            const uint64_t eo = (uint64_t)t * a.B + (uint64_t)e;
            store_state<W>(a.obs + eo * W, o);
            const bool term = cube_match<W>(o, target);  // :190-199 (target[0] only)
            a.reward[eo] = (term ? a.reward_success : 0) - a.action_cost * n_act;  // :218-222
            a.flags[eo] = (uint8_t)((term ? 1 : 0) | (nst == a.horizon ? 2 : 0) | (capped ? 4 : 0));
            a.n_updates[eo] = used;
        }
        wave_sync();  // every lane's row reads before the next step rewrites the row
        ++t;
        begin_steps(s);
        wave_sync();
    }
}

// ------------------------------------------------------------------ rollout, group mode
// k_rollout with G lanes per env (predictor mix, N <= 256): each block of G consecutive updates
// is resolved at once by grp_resolve (the same machinery as k_env_grp), the env's state kept as
// one LDS row per group. Same Philox counters as k_rollout, so the same states. For batches too
// small to give every SIMD several waves in lane mode (BASELINE config 2: 65,536 envs = one
// wave per SIMD), where one env per lane is latency-bound on its own update chain.
template <int W, int G>
__global__ __launch_bounds__(BLOCK) void k_rollout_grp(StepArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const Thr32 X = thr32_layout(a.L);  // the compact image (thresholds on the choice word)
    stage_image(reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.img) + a.L.bytes), X.bytes / 16,
                reinterpret_cast<uint4*>(lds));
    __syncthreads();
    const uint32_t N = (uint32_t)a.L.n_nodes;
    const uint32_t lane = __lane_id();
    const uint32_t k = lane & (G - 1);
    const uint32_t gbase = lane & ~(uint32_t)(G - 1);
    const uint32_t gmask = (1u << G) - 1u;
    uint32_t* row = reinterpret_cast<uint32_t*>(lds + a.L.plane_off) + (threadIdx.x / G) * (2 * W);
    const uint64_t groups = (uint64_t)gridDim.x * (BLOCK / G);
    // every group of a wave takes the same number of trips (ballots and wave syncs inside)
    for (uint64_t e = (uint64_t)blockIdx.x * (BLOCK / G) + threadIdx.x / G;; e += groups) {
        const bool live = e < a.B;
        if (__ballot(live) == 0) break;
        uint64_t s[W];
        if (live) {
            load_state<W>(a.state + e * W, s);
            if (k == 0) {
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    row[2 * q] = (uint32_t)s[q];
                    row[2 * q + 1] = (uint32_t)(s[q] >> 32);
                }
            }
        }
        wave_sync();
        const uint64_t g = a.env_base + e;
        for (uint32_t used = 0; used < a.T; used += G) {
            uint32_t nw, cw;
            step_words(a.seed, a.update_base + used + k, g, nw, cw);
            const uint32_t i = philox_node<KIND_PREDICTOR_MIX>(nw, N);
            const uint64_t rec = predictor_record32(i, cw, lds, X);
            const uint32_t in[4] = {(uint32_t)rec & 0xFFFFu, (uint32_t)(rec >> 16) & 0xFFFFu,
                                    (uint32_t)(rec >> 32) & 0xFFFFu, i};
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (row[in[q] >> 5] >> (in[q] & 31u)) & 1u;  // block-start values
            const GrpBlock<G> blk = grp_resolve<G>(i, rec, in, v, k, gbase, gmask);
            const uint32_t n_done = min((uint32_t)G, a.T - used);
            // the last writer of each node among the block's valid updates sets its bit
            if (live && k < n_done && blk.y != v[3] && blk.last(i, k, n_done)) {
                if (blk.y)
                    atomicOr(&row[i >> 5], 1u << (i & 31u));
                else
                    atomicAnd(&row[i >> 5], ~(1u << (i & 31u)));
            }
            wave_sync();
        }
        if (live && k == 0) {
            uint64_t out[W];
            bool diff = false;  // whole env, only if it differs (see k_step_single)
#pragma unroll
            for (int q = 0; q < W; ++q) {
                out[q] = (uint64_t)row[2 * q] | ((uint64_t)row[2 * q + 1] << 32);
                diff |= out[q] != s[q];
            }
            if (diff) store_state<W>(a.state + e * W, out);
        }
        wave_sync();  // the row is rewritten by the group's next env
    }
}

// ------------------------------------------------------------------ dispatch (W <= 4: N <= 256)
template <int G>
static void* rollout_grp_fn(int W) {
    return by_words<4>(W, [](auto w) { return (void*)k_rollout_grp<w, G>; });
}

void* rollout_grp_kernel(int W, int grp) {
    return grp == 2 ? rollout_grp_fn<2>(W) : grp == 4 ? rollout_grp_fn<4>(W) : grp == 8 ? rollout_grp_fn<8>(W) : nullptr;
}

template <int G>
static void* env_grp_fn(int W) {
    return by_words<4>(W, [](auto w) { return (void*)k_env_grp<w, G>; });
}

void* env_grp_kernel(int W, int grp) {
    return grp == 2 ? env_grp_fn<2>(W) : grp == 4 ? env_grp_fn<4>(W) : grp == 8 ? env_grp_fn<8>(W) : nullptr;
}

}  // namespace pbn
