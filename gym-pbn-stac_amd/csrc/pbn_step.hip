// pbn_step.hip -- the step / rollout kernels (k_step is the bench kernel) and their dispatch; the group-mode
// rollout k_rollout_grp is in pbn_group.hip.
//
// Mapping: one lane owns one env at a time; its state words are loaded into VGPRs and, for the
// node update, spread over the lane's column of LDS state planes. Each workgroup stages the
// network image (thresholds, predictor records or probability tables) into LDS once. Step mode
// (the bench kernel, k_step<.., 1024>): 1024-thread workgroups, two per CU, every thread owning
// one pair of envs (e, e + grid stride) at 1M envs (more pairs per thread, grid-stride, above);
// rollout: 256-thread workgroups sized to what is resident, walking envs in a grid-stride loop.
//
// Reference semantics implemented (file:line in the reference):
//   k_step    Graph.step base.py:306-312 (+ Node.Predstep :89-119) and
//             PBN.step common/pbn.py:129-133 (+ Node.compute_next_value common/node.py:34-38)
#include <hip/hip_runtime.h>

#include "pbn_device.hpp"
#include "pbn_launch.hpp"
#include "pbn_params.hpp"

namespace pbn {

#ifdef PBN_STAMPS
// Measurement builds only (tools/build_exp.sh -DPBN_STAMPS): per-wave s_memrealtime stamps (100 MHz)
// of the step kernel's phases, kept in registers and written once at the end of the wave.
__device__ uint64_t g_stamps[16384 * 8];
#endif

// ------------------------------------------------------------------ step
// Layout per workgroup in LDS: [network image][state planes]. The state planes
// hold, for the env each lane is working on, its 2W dwords in planar order
// (dword d of lane l at plane d, column l), so reading node i of the own env is
// one conflict-free ds_read_b32 at plane (i >> 5) and an update is one
// read-modify-write of one dword -- instead of ~20 VALU selects per bit when the
// words sit in VGPRs. Columns are lane-private: no barrier is needed around them.
//
// Each thread walks envs e0, e0 + stride, ... with the next env's state load in
// flight while the current env is computed (software pipeline), so HBM traffic
// of one env overlaps the Philox/LDS work of the previous one.
//
// SB (threads per workgroup) trades LDS staging traffic against scheduling
// granularity: the image is staged once per workgroup, so 1024-thread groups
// read it from L2 4x less often than 256-thread groups.
// One update per env (T == 1), Philox. Envs are taken in pairs (e, e + stride); at the
// bench sizes every thread owns exactly one pair. The pair's draws and (for predictor
// networks) its predictor records depend only on (seed, update counter, env id), so
// they are computed while the pair's state loads are in flight.
template <int W, int KIND, int STORE, int SB, bool PRE = false>
__device__ __forceinline__ void k_step_single(const StepArgs& a, uint8_t* lds, uint64_t e, uint64_t stride,
                                              uint64_t (&cur)[W], uint32_t N, uint64_t (*pre_nxt)[W] = nullptr) {
    // graph replays read the batch's update counter from device memory (k_bump advances it)
    const uint64_t u = a.update_base + (a.ubase_dev ? *a.ubase_dev : 0ull);
    const uint64_t po = stride;  // second env of the pair (adjacent envs measured slower: 8.2 vs 7.8 us)
    uint64_t nxt[W];
    uint32_t i0 = 0, i1 = 0;
    uint64_t q0 = 0, q1 = 0;
    // envs 2m / 2m + 1 share a Philox call (pbn_device.hpp): with an even env base, lane parity is
    // env parity and the lane pair computes one call per env pair each (step_words_paired). A
    // partner lane that has left the loop holds envs >= B only, so the words it no longer sends
    // belong to envs that are not applied.
    const bool paired = (a.env_base & 1u) == 0u;
    const bool odd = (threadIdx.x & 1u) != 0u;
    auto draws = [&](uint64_t ea) {
        const uint64_t g0 = a.env_base + ea, g1 = g0 + po;
        uint32_t n0, c0, n1, c1;
        if (paired) {
            step_words_paired(a.seed, u, g0, g1, odd, n0, c0, n1, c1);
        } else {
            step_words(a.seed, u, g0, n0, c0);
            step_words(a.seed, u, g1, n1, c1);
        }
        i0 = philox_node<KIND>(n0, N);
        i1 = philox_node<KIND>(n1, N);
        // predictor mix: the choice word itself (compact image, thresholds on the word); tables: k53
        q0 = KIND == KIND_PREDICTOR_MIX ? (uint64_t)c0 : u32_k53(c0);
        q1 = KIND == KIND_PREDICTOR_MIX ? (uint64_t)c1 : u32_k53(c1);
    };
#ifdef PBN_STAMPS
    uint64_t st[8] = {__builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0, 0, 0, 0};
#endif
    const Thr32 X = thr32_layout(a.L);
    if constexpr (PRE) {  // image staged and both loads issued by the caller (k_step)
#pragma unroll
        for (int k = 0; k < W; ++k) nxt[k] = (*pre_nxt)[k];
        draws(e);
#ifdef PBN_STAMPS
        st[2] = st[0];  // the caller's barrier was passed on entry here
        st[1] = __builtin_amdgcn_s_memrealtime();
#endif
    } else {
    if (e + po < a.B) load_state<W>(a.state + (e + po) * W, nxt);
    draws(e);
#ifdef PBN_STAMPS
    st[1] = __builtin_amdgcn_s_memrealtime();
#endif
    if constexpr (KIND == KIND_PREDICTOR_MIX)  // the compact image (thresholds on the choice word)
        stage_image(reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.img) + a.L.bytes), X.bytes / 16,
                    reinterpret_cast<uint4*>(lds));
    else
        stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    }
#ifdef PBN_STAMPS
    st[2] = __builtin_amdgcn_s_memrealtime();
#endif
    const PlaneT<SB> P{reinterpret_cast<uint32_t*>(lds + a.L.plane_off) + threadIdx.x};
    while (e < a.B) {
        const uint64_t e1 = e + po;
        uint64_t r0 = 0, r1 = 0;
        if constexpr (KIND == KIND_PREDICTOR_MIX) {  // state-independent: before the loads land
            r0 = predictor_record32(i0, (uint32_t)q0, lds, X);
            r1 = predictor_record32(i1, (uint32_t)q1, lds, X);
        }
#ifdef PBN_STAMPS
        if (!st[3]) {
            __builtin_amdgcn_s_waitcnt(0);  // records read and state landed (measurement build)
            st[3] = __builtin_amdgcn_s_memrealtime();
        }
#endif
        if constexpr (STORE != STORE_FULL) {
            // Both envs evaluated first (plane writes and reads of env 1 issued right behind env 0's;
            // LDS runs a wave's operations in order, so reusing the column needs no wait), then both
            // stores: with env 0's store issued before env 1's loads were consumed, the compiler
            // waited for that store to complete (vmcnt(0)) before env 1's plane writes.
            // Env 1 is evaluated unconditionally (past B: junk from a clamped or skipped load,
            // never stored).
            // the plane's last dword holds nodes >= 64W - 32 only: it is written only if N reaches it
            // (Bittner-200: 7 of the 8 dwords, one LDS write of eight saved per env)
            const bool last_dw = N > 64u * W - 32u;
            auto eval = [&](const uint64_t (&s)[W], uint32_t i, uint64_t r, uint64_t q, uint32_t& self) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    P.put(2 * k, (uint32_t)s[k]);
                    if (k + 1 < W || last_dw) P.put(2 * k + 1, (uint32_t)(s[k] >> 32));
                }
                self = P.get(i >> 5);
                if constexpr (KIND == KIND_PREDICTOR_MIX)
                    return predictor_apply(P, i, self, r);
                else
                    return table_eval_lds(P, i, q, lds, a.L);
            };
            uint32_t self0, self1;
            const uint32_t y0 = eval(cur, i0, r0, q0, self0);
            const uint32_t y1 = eval(nxt, i1, r1, q1, self1);
            // An env is stored only if its bit changed: whole (STORE_DIRTY, 32 B at W = 4) or, STORE_HALF,
            // just the 16-B half that holds node i. Which one is the host's choice by batch size
            // (step_half_store, pbn_step_plan.hpp): the half store wins while the whole batch is resident
            // at once (1M Bittner-200 envs: 9.5 -> 8.8 us per step) and loses from 2M envs on, where
            // half-written 32-B sectors cost more than the bytes saved (8M: 55.5 -> 59.2 us). The env's
            // words are still in registers: bit i is flipped there (store_changed) rather than written
            // to the plane and all 2W dwords read back
            auto put = [&](const uint64_t (&s)[W], uint64_t eh, uint32_t i) {
                store_changed<W, STORE == STORE_HALF>(a.state + eh * W, s, i);
            };
            if (((self0 >> (i0 & 31u)) & 1u) != y0) put(cur, e, i0);
            if (e1 < a.B && ((self1 >> (i1 & 31u)) & 1u) != y1) put(nxt, e1, i1);
        } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint64_t eh = h ? e1 : e;
            if (eh >= a.B) break;
            uint64_t(&s)[W] = h ? nxt : cur;
            const uint32_t i = h ? i1 : i0;
            const uint32_t d = i >> 5, sh = i & 31u;
            to_plane<W>(P, s);
            const uint32_t self = P.get(d);
            uint32_t y;
            if constexpr (KIND == KIND_PREDICTOR_MIX)
                y = predictor_apply(P, i, self, h ? r1 : r0);
            else
                y = table_eval_lds(P, i, h ? q1 : q0, lds, a.L);
            const uint32_t nv = (self & ~(1u << sh)) | (y << sh);
            P.put(d, nv);
            uint64_t out[W];
            from_plane<W>(P, out);
            store_state<W>(a.state + eh * W, out);
        }
        }
#ifdef PBN_STAMPS
        if (!st[4]) st[4] = __builtin_amdgcn_s_memrealtime();  // the first pair's stores issued
#endif
        e += 2 * stride;
        if (e < a.B) {
            load_state<W>(a.state + e * W, cur);
            if (e + po < a.B) load_state<W>(a.state + (e + po) * W, nxt);
            draws(e);
        }
    }
#ifdef PBN_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    st[5] = __builtin_amdgcn_s_memrealtime();  // every store of the wave done
    const uint32_t wv = blockIdx.x * (SB / 64) + threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0 && wv < 16384) {
        st[6] = blockIdx.x;
        st[7] = __smid();
        for (int k = 0; k < 8; ++k) g_stamps[wv * 8 + k] = st[k];
    }
#endif
}

// The bench shape: every thread owns exactly one env pair (B <= 2 x grid x SB), image staged and both
// loads issued by k_step. Straight-line, so both envs' threshold rows are read in one LDS round trip
// and both records in a second (the looped form read env 0's row, its record, env 1's row, its
// record: three dependent round trips, the uniform tp4 == 4 branch between them), and env 0's plane
// work waits only for env 0's loads.
template <int W, int STORE, int SB>
__device__ __forceinline__ void k_step_pair(const StepArgs& a, uint8_t* lds, uint64_t e, uint64_t stride,
                                            const uint64_t (&cur)[W], const uint64_t (&nxt)[W], uint32_t N) {
    const uint64_t u = a.update_base + (a.ubase_dev ? *a.ubase_dev : 0ull);
    const uint64_t e1 = e + stride, g0 = a.env_base + e, g1 = g0 + stride;
    uint32_t n0, c0, n1, c1;
    if ((a.env_base & 1u) == 0u) {  // envs 2m / 2m + 1 share a Philox call (k_step_single)
        step_words_paired(a.seed, u, g0, g1, (threadIdx.x & 1u) != 0u, n0, c0, n1, c1);
    } else {
        step_words(a.seed, u, g0, n0, c0);
        step_words(a.seed, u, g1, n1, c1);
    }
    const uint32_t i0 = philox_node<KIND_PREDICTOR_MIX>(n0, N), i1 = philox_node<KIND_PREDICTOR_MIX>(n1, N);
    const Thr32 X = thr32_layout(a.L);
    uint32_t j0, j1;
    if (X.tp4 == 4u) {
        const uint4 t0 = reinterpret_cast<const uint4*>(lds)[i0];
        const uint4 t1 = reinterpret_cast<const uint4*>(lds)[i1];
        j0 = (c0 >= t0.x ? 1u : 0u) + (c0 >= t0.y ? 1u : 0u) + (c0 >= t0.z ? 1u : 0u) + (c0 >= t0.w ? 1u : 0u);
        j1 = (c1 >= t1.x ? 1u : 0u) + (c1 >= t1.y ? 1u : 0u) + (c1 >= t1.z ? 1u : 0u) + (c1 >= t1.w ? 1u : 0u);
    } else {
        j0 = predictor_choice32(i0, c0, lds, X.tp4);
        j1 = predictor_choice32(i1, c1, lds, X.tp4);
    }
    const uint64_t* rec = reinterpret_cast<const uint64_t*>(lds + X.rec_off);
    const uint64_t r0 = rec[__umul24(i0, X.rs) + j0], r1 = rec[__umul24(i1, X.rs) + j1];
    const PlaneT<SB> P{reinterpret_cast<uint32_t*>(lds + a.L.plane_off) + threadIdx.x};
    const bool last_dw = N > 64u * W - 32u;  // the plane's last dword holds nodes >= 64W - 32 only
    auto eval = [&](const uint64_t (&s)[W], uint32_t i, uint64_t r, uint32_t& self) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            P.put(2 * k, (uint32_t)s[k]);
            if (k + 1 < W || last_dw) P.put(2 * k + 1, (uint32_t)(s[k] >> 32));
        }
        self = P.get(i >> 5);
        return predictor_apply(P, i, self, r);
    };
    auto put = [&](const uint64_t (&s)[W], uint64_t eh, uint32_t i) {  // bit i flipped (store_changed)
        store_changed<W, STORE == STORE_HALF>(a.state + eh * W, s, i);
    };
    uint32_t self0, self1;
    const uint32_t y0 = eval(cur, i0, r0, self0);
    // env 0 is stored before env 1 is evaluated; env 1's loads (issued right behind env 0's) are waited
    // for first: after a store that may not have been issued, the compiler can only wait vmcnt(0)
#pragma unroll
    for (int k = 0; k < W; ++k) asm volatile("" ::"v"(nxt[k]));
    if (e < a.B && ((self0 >> (i0 & 31u)) & 1u) != y0) put(cur, e, i0);
    const uint32_t y1 = eval(nxt, i1, r1, self1);  // past B: junk from a clamped load, never stored
    if (e1 < a.B && ((self1 >> (i1 & 31u)) & 1u) != y1) put(nxt, e1, i1);
}

// Step mode (T == 1, Philox; REPLAY == 0) and replay mode (REPLAY == 1: T updates from the
// caller's draws). Rollout (T > 1, Philox) is its own kernel, k_rollout, so that neither
// path's code shapes the other's register allocation and schedule (sharing one kernel cost
// the step path 0.6 us per launch at 1M envs).
template <int W, int KIND, int STORE, int REPLAY, int SB>
// 1024-thread groups, W <= 4: two workgroups per CU = 8 waves per SIMD, so at most 64 VGPRs (every
// instance this bound applies to -- both kinds, both store modes, Philox only: SB = 1024 is never
// launched in replay mode -- compiles without scratch, `make asm`; the stamps build keeps the bound)
__global__ __launch_bounds__(SB, (SB == 1024 && W <= 4) ? 8 : 1)
void k_step(StepArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint64_t stride = (uint64_t)gridDim.x * SB;
    uint64_t e = (uint64_t)blockIdx.x * SB + threadIdx.x;
    const uint32_t N = (uint32_t)a.L.n_nodes;
    uint64_t cur[W];
    if constexpr (!REPLAY && KIND == KIND_PREDICTOR_MIX && SB == 1024) {
        // The image's granule (one per thread) is loaded first, then both envs of the pair
        // (unconditional loads, clamped addresses, so the granule's wait counts only itself:
        // vmcnt(4)); the granule is written and the barrier passed while the state is in flight,
        // and the draws follow the barrier. Staged after the draws instead, the barrier waited
        // for every wave's Philox burst and the state loads: 9.21 -> 8.98 us per launch at 1M envs
        // (profiles/r02_step_stage_first_ab.txt; phase stamps r02_step_stamps.json)
        const Thr32 X = thr32_layout(a.L);
        const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.img) + a.L.bytes);
        const uint32_t n16 = X.bytes / 16;
        uint4 g = make_uint4(0, 0, 0, 0);
        if (threadIdx.x < n16) g = src[threadIdx.x];
        uint64_t nx[W];
        const uint64_t ec = e < a.B ? e : 0, en = e + stride < a.B ? e + stride : 0;
        load_state<W>(a.state + ec * W, cur);
        load_state<W>(a.state + en * W, nx);
        if (threadIdx.x < n16) reinterpret_cast<uint4*>(lds)[threadIdx.x] = g;
        for (uint32_t k = threadIdx.x + SB; k < n16; k += SB) reinterpret_cast<uint4*>(lds)[k] = src[k];
        __syncthreads();
        if (STORE != STORE_FULL && 2u * stride >= a.B)
            k_step_pair<W, STORE, SB>(a, lds, e, stride, cur, nx, N);  // one pair per thread (the bench shape)
        else
            k_step_single<W, KIND, STORE, SB, true>(a, lds, e, stride, cur, N, &nx);
        return;
    }
    if (e < a.B) load_state<W>(a.state + e * W, cur);
    if constexpr (!REPLAY) {
        // Step mode: the draws depend on (seed, update counter, env id) only, so every
        // draw this thread needs is computed while its state loads are in flight.
        k_step_single<W, KIND, STORE, SB>(a, lds, e, stride, cur, N);
    } else {
        stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
        __syncthreads();
        const PlaneT<SB> P{reinterpret_cast<uint32_t*>(lds + a.L.bytes) + threadIdx.x};
        while (e < a.B) {
            const uint64_t en = e + stride;
            uint64_t nxt[W];
            if (en < a.B) load_state<W>(a.state + en * W, nxt);  // prefetch the next env
            to_plane<W>(P, cur);
            for (uint32_t t = 0; t < a.T; ++t) {
                const uint32_t i = a.replay_node[(uint64_t)t * a.B + e];
                uint64_t k53;
                if (a.replay_k53) {
                    k53 = a.replay_k53[(uint64_t)t * a.B + e];
                } else {
                    // forced node (Graph.step(i=k), base.py:306-308): the node is the caller's, the
                    // choice word is the env's own Philox step draw of update update_base + t
                    uint32_t wn, wc;
                    step_words(a.seed, a.update_base + t, a.env_base + e, wn, wc);
                    k53 = u32_k53(wc);
                }
                if constexpr (KIND == KIND_PREDICTOR_MIX)
                    predictor_update_lds(P, i, k53, lds, a.L);
                else
                    table_update_lds(P, i, k53, lds, a.L);
            }
            uint64_t out[W];
            from_plane<W>(P, out);
            store_state<W>(a.state + e * W, out);
#pragma unroll
            for (int k = 0; k < W; ++k) cur[k] = nxt[k];
            e = en;
        }
    }
}

// Rollout: T Philox updates per env per launch with the env's state in its LDS plane column;
// the state is read once and written once (only if it changed).
template <int W, int KIND, int SB>
__global__ __launch_bounds__(SB) void k_rollout(StepArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint64_t stride = (uint64_t)gridDim.x * SB;
    uint64_t e = (uint64_t)blockIdx.x * SB + threadIdx.x;
    const uint32_t N = (uint32_t)a.L.n_nodes;
    uint64_t cur[W];
    if (e < a.B) load_state<W>(a.state + e * W, cur);
    const Thr32 X = thr32_layout(a.L);
    if constexpr (KIND == KIND_PREDICTOR_MIX)  // the compact image (thresholds on the choice word)
        stage_image(reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.img) + a.L.bytes), X.bytes / 16,
                    reinterpret_cast<uint4*>(lds));
    else
        stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    const PlaneT<SB> P{reinterpret_cast<uint32_t*>(lds + a.L.plane_off) + threadIdx.x};
    // Envs 2m / 2m + 1 share their Philox calls (pbn_device.hpp). With an even env base the lane
    // pair holds such a pair, and for updates t, t + 1 the even lane computes the call of t, the
    // odd lane that of t + 1, and they swap the two words the other needs: one call per lane
    // per two updates. Every lane of a wave takes the same trips (lanes past B compute junk
    // and store nothing), so a partner is never missing.
    const bool paired = (a.env_base & 1u) == 0u;
    const bool odd = (threadIdx.x & 1u) != 0u;
    for (;;) {
        const bool live = e < a.B;
        if (__ballot(live) == 0) break;
        const uint64_t en = e + stride;
        uint64_t nxt[W];
        if (en < a.B) load_state<W>(a.state + en * W, nxt);  // prefetch the next env
        to_plane<W>(P, cur);
        uint32_t changed = 0;
        const uint64_t g = a.env_base + e;
        // node / choice words of updates t and t + 1 of this lane's env
        auto words2 = [&](uint32_t t, uint32_t& na, uint32_t& ca, uint32_t& nb, uint32_t& cb) {
            const uint64_t u = a.update_base + t;
            if (paired) {
                uint32_t w[4];
                philox_draw(a.seed, (uint32_t)(u + (odd ? 1u : 0u)), (uint32_t)((u + (odd ? 1u : 0u)) >> 32), g >> 1,
                            STREAM_STEP, w);
                const uint32_t r0 = swap_pair_lanes(odd ? w[0] : w[2]), r1 = swap_pair_lanes(odd ? w[1] : w[3]);
                na = odd ? r0 : w[0];
                ca = odd ? r1 : w[1];
                nb = odd ? w[2] : r0;
                cb = odd ? w[3] : r1;
            } else {
                step_words(a.seed, u, g, na, ca);
                step_words(a.seed, u + 1u, g, nb, cb);
            }
        };
        if constexpr (KIND == KIND_PREDICTOR_MIX) {
            // software pipeline: the draws and predictor records of updates t + 2, t + 3
            // (state-independent) are computed while updates t, t + 1 run -- one env per lane
            // leaves a wave alone on its SIMD at small batches (65,536 envs: one wave per SIMD)
            uint32_t ia, ib;
            uint64_t ra, rb;
            auto draw2 = [&](uint32_t t) {
                uint32_t na, ca, nb, cb;
                words2(t, na, ca, nb, cb);
                ia = philox_node<KIND>(na, N);
                ib = philox_node<KIND>(nb, N);
                ra = predictor_record32(ia, ca, lds, X);
                rb = predictor_record32(ib, cb, lds, X);
            };
            auto apply = [&](uint32_t i, uint64_t rec) {
                const uint32_t d = i >> 5, sh = i & 31u;
                const uint32_t self = P.get(d);
                const uint32_t y = predictor_apply(P, i, self, rec);
                const uint32_t nv = (self & ~(1u << sh)) | (y << sh);
                P.put(d, nv);
                changed |= nv != self;
            };
            draw2(0);
            for (uint32_t t = 0; t < a.T; t += 2) {
                const uint32_t i0 = ia, i1 = ib;
                const uint64_t r0 = ra, r1 = rb;
                draw2(t + 2);  // unconditional (past T: junk, unused): no branch before the plane reads
                apply(i0, r0);
                if (t + 1 < a.T) apply(i1, r1);
            }
        } else {
            for (uint32_t t = 0; t < a.T; t += 2) {
                uint32_t na, ca, nb, cb;
                words2(t, na, ca, nb, cb);
                changed |= table_update_lds(P, philox_node<KIND>(na, N), u32_k53(ca), lds, a.L);
                if (t + 1 < a.T) changed |= table_update_lds(P, philox_node<KIND>(nb, N), u32_k53(cb), lds, a.L);
            }
        }
        uint64_t out[W];
        from_plane<W>(P, out);
        bool diff = false;  // whole env, only if it differs (see k_step_single)
#pragma unroll
        for (int k = 0; k < W; ++k) diff |= out[k] != cur[k];
        if (live && changed && diff) store_state<W>(a.state + e * W, out);
#pragma unroll
        for (int k = 0; k < W; ++k) cur[k] = nxt[k];
        e = en;
    }
}

// ------------------------------------------------------------------ dispatch
template <int W, int KIND>
static void* step_fn(int store, int replay, int sb, int rollout, int grp) {
    if (replay) return (void*)k_step<W, KIND, STORE_FULL, 1, BLOCK>;
    if (grp > 1) return rollout && KIND == KIND_PREDICTOR_MIX ? rollout_grp_kernel(W, grp) : nullptr;
    if (rollout) return sb == 1024 ? (void*)k_rollout<W, KIND, 1024> : (void*)k_rollout<W, KIND, BLOCK>;
    if (sb != 1024 && store == STORE_HALF) store = STORE_DIRTY;  // the half store: 1024-thread kernels only
    if constexpr (W % 2 == 0 && W >= 4)
        if (store == STORE_HALF) return (void*)k_step<W, KIND, STORE_HALF, 0, 1024>;
    if (store == STORE_HALF) store = STORE_DIRTY;  // W odd or < 4: the whole env is the write-back
    if (sb == 1024)
        return store == STORE_DIRTY ? (void*)k_step<W, KIND, STORE_DIRTY, 0, 1024>
                                    : (void*)k_step<W, KIND, STORE_FULL, 0, 1024>;
    return store == STORE_DIRTY ? (void*)k_step<W, KIND, STORE_DIRTY, 0, BLOCK>
                                : (void*)k_step<W, KIND, STORE_FULL, 0, BLOCK>;
}

template <int KIND>
static void* step_fn_w(int W, int store, int replay, int sb, int rollout, int grp) {
    return by_words<8>(W, [=](auto w) { return step_fn<w, KIND>(store, replay, sb, rollout, grp); });
}

uint32_t step_lds_bytes(int W, uint32_t image_bytes, int sb, int grp) {
    if (grp > 1) return image_bytes + 8u * (uint32_t)W * (BLOCK / (uint32_t)grp);  // one row per group
    return image_bytes + 8u * (uint32_t)W * (uint32_t)sb;
}

static void* step_kernel(int W, int kind, int store_mode, int replay, int sb, int rollout, int grp) {
    if (replay) sb = BLOCK;
    return kind == KIND_PREDICTOR_MIX ? step_fn_w<KIND_PREDICTOR_MIX>(W, store_mode, replay, sb, rollout, grp)
                                      : step_fn_w<KIND_PROB_TABLE>(W, store_mode, replay, sb, rollout, grp);
}

int launch_step(int W, const StepArgs& a, int store_mode, int replay, int sb, int grid, void* stream) {
    if (replay) sb = BLOCK;
    const bool rollout = !replay && a.T > 1;
    const int grp = rollout && a.grp > 1 ? a.grp : 1;
    if (grp > 1) sb = BLOCK;
    StepArgs c = a;
    return launch(step_kernel(W, a.L.kind, store_mode, replay, sb, rollout, grp), grid, sb,
                  step_lds_bytes(W, replay ? a.L.bytes : a.L.plane_off, sb, grp), stream, &c);
}

int max_blocks_step(int W, int kind, uint32_t lds_bytes, int sb, int* blocks_per_cu, int rollout, int grp) {
    if (grp > 1) sb = BLOCK;
    return occupancy(step_kernel(W, kind, STORE_FULL, 0, sb, rollout, grp), sb, step_lds_bytes(W, lds_bytes, sb, grp),
                     blocks_per_cu);
}

#ifdef PBN_STAMPS
int step_stamps_clear() {
    static uint64_t z[16384 * 8];
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z, 0, hipMemcpyHostToDevice);
}
}  // namespace pbn
extern "C" int pbn_exp_stamps(void* out, size_t bytes) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pbn::g_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
extern "C" int pbn_exp_stamps_clear() {
    int rc = pbn::step_stamps_clear();
    if (!rc) rc = pbn::env_stamps_clear();
    return rc;
}
namespace pbn {
#endif

// Advances the device-side update counter by k at the end of a captured run of step launches.
__global__ void k_bump(uint64_t* p, uint64_t k) {
    if (threadIdx.x == 0) p[threadIdx.x] += k;
}

int launch_bump(uint64_t* p, uint64_t k, void* stream) {
    void* kargs[] = {(void*)&p, (void*)&k};
    return (int)hipLaunchKernel((const void*)k_bump, dim3(1), dim3(64), kargs, 0, (hipStream_t)stream);
}

// Sets the device-side update counters p[0 .. n) (one per launch chain, n <= 64) to v in front of a call's
// graph replays.
__global__ void k_set_counters(uint64_t* p, uint64_t v, uint32_t n) {
    if (threadIdx.x < n) p[threadIdx.x] = v;
}

int launch_set_counters(uint64_t* p, uint64_t v, uint32_t n, void* stream) {
    if (n > 64u) return (int)hipErrorInvalidValue;
    void* kargs[] = {(void*)&p, (void*)&v, (void*)&n};
    return (int)hipLaunchKernel((const void*)k_set_counters, dim3(1), dim3(64), kargs, 0, (hipStream_t)stream);
}

}  // namespace pbn
