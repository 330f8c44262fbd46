// pbn_reach.hip -- attractor discovery on the support graph of a network.
//
// Predictor mix: the support graph has an edge x -> x ^ (1 << i) iff some live predictor of node i outputs
// 1 - x_i at x (the support of the reference's getNextStates, base.py:221-242: it keeps an edge when prob > 0;
// base.py:398-399 findAttractors takes the terminal strongly connected components). A predictor is live
// iff its selection interval on the 53-bit grid is non-empty, so the rule is defined on the 53-bit
// thresholds of the network image, not on the 32-bit grid of the Philox stream.
// Truth tables: the edge exists iff the table entry of node i at x lets it leave x_i (threshold > 0 from 0,
// < 2^53 from 1), over nodes first_node .. N-1: 0 for the graph of PBN._compute_next_states, 1 for the graph
// PBN.step walks. Both rules are defined once, for the kernels and the host, in pbn_reach_rule.hpp; the
// kernels that evaluate them are templated on the network kind.
//
// Mapping: one wave per state, lanes over nodes. All the work of a state (N table-row reads, up to N
// set operations) is then one wave's, the state words are wave-uniform registers, and the set operations
// of a wave hit N different slots; one lane per state would serialise N dependent hash probes per lane.
//
// The set is wait-free: no lane ever waits for another lane's progress. Every loop is bounded by the table
// size, and a full table / key array / max_states only raises the overflow word.
#include "pbn_device.hpp"
#include "pbn_keytable.hpp"
#include "pbn_lane_env.hpp"
#include "pbn_launch.hpp"
#include "pbn_reach_rule.hpp"

namespace pbn {

namespace {

// 1 iff node i can flip at state s (pbn_reach_rule.hpp), the state words read out of registers.
template <int W, int KIND>
__device__ __forceinline__ uint32_t can_flip_at(const uint64_t (&s)[W], uint32_t i, const uint8_t* tbl,
                                                const ReachArgs& a) {
    return can_flip<KIND>([&](uint32_t j) { return getbit<W>(s, j); }, i, a.first_node, tbl, a.L);
}

// Entry index of state s, or REACH_NONE. INSERT: add it if absent (REACH_NONE then means overflow). The walk and its
// protocol are keytable_walk's (pbn_keytable.hpp); what is the reach set's own -- an entry comes from the free ring,
// else from the end of keys; a publish is counted and appended to the queue (the next frontier); an entry that was not
// published is marked dead and pushed onto the free ring; no entry or no slot raises the overflow word -- is ReachTable.
template <int W, bool INSERT>
__device__ uint32_t reach_find(const ReachArgs& a, const uint64_t (&s)[W]) {
    return keytable_walk<W, INSERT>(KeytableDeviceMem{a.table, reinterpret_cast<unsigned long long*>(a.keys)},
                                    ReachTable<KeytableDeviceCtl>{a}, a.tmask, s);
}

__device__ __forceinline__ const uint8_t* stage(const ReachArgs& a, uint8_t* lds) {
    stage_image(reinterpret_cast<const uint4*>(a.img), a.L.bytes / 16, reinterpret_cast<uint4*>(lds));
    __syncthreads();
    return lds;
}

// ---- unstable: masks of the nodes that can flip, one wave per state, a ballot per 64 nodes
template <int W, int KIND>
__global__ __launch_bounds__(BLOCK) void k_unstable(ReachArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint8_t* tbl = stage(a, lds);
    const uint32_t N = (uint32_t)a.L.n_nodes, lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (BLOCK / 64);
    for (uint64_t e = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); e < a.n_in; e += n_waves) {
        uint64_t s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = a.in[e * W + k];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint32_t i = 64u * k + lane;
            const uint64_t m = __ballot(i < N && can_flip_at<W, KIND>(s, i, tbl, a));
            if (lane == 0) a.out[e * W + k] = m;
        }
    }
}

// ---- seeds: one lane per seed state
template <int W>
__global__ __launch_bounds__(BLOCK) void k_reach_seed(ReachArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.n_in) return;
    uint64_t s[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = a.in[e * W + k];
    (void)reach_find<W, true>(a, s);
}

// ---- forward expansion of the frontier queue[lo, hi): entries the launch publishes are appended past hi
template <int W, int KIND>
__global__ __launch_bounds__(BLOCK) void k_reach_expand(ReachArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint8_t* tbl = stage(a, lds);
    const uint32_t N = (uint32_t)a.L.n_nodes, lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * (BLOCK / 64);
    for (uint32_t f = a.lo + blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); f < a.hi; f += n_waves) {
        const uint32_t e = a.queue[f];  // written by an earlier launch, as are the entry's words
        uint64_t s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = a.keys[(uint64_t)e * W + k];
        for (uint32_t i = lane; i < N; i += 64u) {
            if (!can_flip_at<W, KIND>(s, i, tbl, a)) continue;
            uint64_t t[W];
#pragma unroll
            for (int k = 0; k < W; ++k) t[k] = s[k];
            xor_bit<W>(t, i, true);
            (void)reach_find<W, true>(a, t);
        }
    }
}

// ---- backward marking: start entry
template <int W>
__global__ __launch_bounds__(64) void k_reach_back_start(ReachArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t s[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = a.in[k];
    const uint32_t j = reach_find<W, false>(a, s);
    if (j == REACH_NONE) {
        KeytableDeviceCtl::raise(a.ctl + REACH_MISSING);
        return;
    }
    a.mark[j] = a.epoch;
    a.queue[0] = j;
    a.ctl[REACH_QTAIL] = 1;
}

// ---- backward marking of the frontier queue[lo, hi): x = y ^ (1 << i) is marked iff it is in the set,
// unmarked, and node i can flip at x (the edge x -> y). Lookups only. A node below first_node has no edge:
// can_flip_at says so after the lookup, as for any other node that cannot move.
template <int W, int KIND>
__global__ __launch_bounds__(BLOCK) void k_reach_back(ReachArgs a) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint8_t* tbl = stage(a, lds);
    const uint32_t N = (uint32_t)a.L.n_nodes, lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * (BLOCK / 64);
    for (uint32_t f = a.lo + blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); f < a.hi; f += n_waves) {
        const uint32_t y = a.queue[f];  // written by an earlier launch, as are the entry's words
        uint64_t s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = a.keys[(uint64_t)y * W + k];
        for (uint32_t i = lane; i < N; i += 64u) {
            uint64_t x[W];
#pragma unroll
            for (int k = 0; k < W; ++k) x[k] = s[k];
            xor_bit<W>(x, i, true);
            const uint32_t j = reach_find<W, false>(a, x);
            if (j == REACH_NONE || keytable_ld32(a.mark + j) == a.epoch) continue;
            if (!can_flip_at<W, KIND>(x, i, tbl, a)) continue;
            if (__hip_atomic_exchange(a.mark + j, a.epoch, KEYTABLE_RLX, KEYTABLE_AGENT) != a.epoch) {
                const uint32_t p = KeytableDeviceCtl::add(a.ctl + REACH_QTAIL);
                if (p < a.key_cap) a.queue[p] = j;  // one append per entry: p < live entries <= key_cap
            }
        }
    }
}

// ---- hull: AND and OR over the live entries keys[0, hi)
template <int W>
__global__ __launch_bounds__(BLOCK) void k_reach_hull(ReachArgs a) {
    uint64_t all[W], any[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        all[k] = ~0ull;
        any[k] = 0;
    }
    for (uint32_t e = blockIdx.x * BLOCK + threadIdx.x; e < a.hi; e += gridDim.x * BLOCK) {
        if (a.mark[e] == REACH_DEAD) continue;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t w = a.keys[(uint64_t)e * W + k];
            all[k] &= w;
            any[k] |= w;
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        // wave reduction first: one atomic pair per wave and word
        for (int d = 32; d >= 1; d >>= 1) {
            all[k] &= __shfl_xor(all[k], d);
            any[k] |= __shfl_xor(any[k], d);
        }
        if ((threadIdx.x & 63u) == 0) {
            __hip_atomic_fetch_and(a.hull + k, (unsigned long long)all[k], KEYTABLE_RLX, KEYTABLE_AGENT);
            __hip_atomic_fetch_or(a.hull + W + k, (unsigned long long)any[k], KEYTABLE_RLX, KEYTABLE_AGENT);
        }
    }
}

}  // namespace

// The kernels that evaluate the edge rule, by words and network kind.
#define REACH_BY_KIND(kernel)                                                                                     \
    (a.L.kind == KIND_PROB_TABLE ? by_words<MAX_WORDS>(W, [](auto w) { return (void*)kernel<w, KIND_PROB_TABLE>; }) \
                                 : by_words<MAX_WORDS>(W, [](auto w) { return (void*)kernel<w, KIND_PREDICTOR_MIX>; }))

int launch_reach(int W, int which, const ReachArgs& a, int grid, void* stream) {
    ReachArgs c = a;
    void* fn = nullptr;
    int block = BLOCK;
    uint32_t lds = a.L.bytes;
    switch (which) {
        case REACH_K_UNSTABLE: fn = REACH_BY_KIND(k_unstable); break;
        case REACH_K_SEED:
            fn = by_words<MAX_WORDS>(W, [](auto w) { return (void*)k_reach_seed<w>; });
            lds = 0;
            break;
        case REACH_K_EXPAND: fn = REACH_BY_KIND(k_reach_expand); break;
        case REACH_K_BACK_START:
            fn = by_words<MAX_WORDS>(W, [](auto w) { return (void*)k_reach_back_start<w>; });
            lds = 0;
            block = 64;
            break;
        case REACH_K_BACK: fn = REACH_BY_KIND(k_reach_back); break;
        case REACH_K_HULL:
            fn = by_words<MAX_WORDS>(W, [](auto w) { return (void*)k_reach_hull<w>; });
            lds = 0;
            break;
        default: break;
    }
    return launch(fn, grid, block, lds, stream, &c);
}

}  // namespace pbn
