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
#include "pbn_launch.hpp"
#include "pbn_reach_rule.hpp"

namespace pbn {

namespace {

// Words another wave may read within the same launch go through 8-byte (4-byte for counters and marks)
// agent-scope atomics on both sides: per-XCD L2s are not coherent and an L1 is not refreshed by other
// CUs' stores.
#define RLX __ATOMIC_RELAXED
#define AGENT __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ unsigned long long ld64(const unsigned long long* p) {
    return __hip_atomic_load(p, RLX, AGENT);
}
__device__ __forceinline__ uint32_t ld32(const uint32_t* p) { return __hip_atomic_load(p, RLX, AGENT); }
__device__ __forceinline__ void raise_flag(uint32_t* p) { __hip_atomic_store(p, 1u, RLX, AGENT); }

// 1 iff node i can flip at state s (pbn_reach_rule.hpp), the state words read out of registers.
template <int W, int KIND>
__device__ __forceinline__ uint32_t can_flip_at(const uint64_t (&s)[W], uint32_t i, const uint8_t* tbl,
                                                const ReachArgs& a) {
    return can_flip<KIND>([&](uint32_t j) { return getbit<W>(s, j); }, i, a.first_node, tbl, a.L);
}

template <int W>
__device__ __forceinline__ void flip_bit(uint64_t (&s)[W], uint32_t i) {
    const uint64_t bit = (uint64_t)1 << (i & 63u);
    const uint32_t wi = i >> 6;
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] ^= bit & (uint64_t)(int64_t)(int32_t)lane_mask(wi, (uint32_t)k);
}

template <int W>
__device__ __forceinline__ uint64_t reach_hash(const uint64_t (&s)[W]) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        h = (h ^ s[k]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}

// Entry index of state s, or REACH_NONE. INSERT: add it if absent (REACH_NONE then means overflow).
// Protocol: an inserter that reaches an empty slot reserves an entry (from the free ring, else an atomic add
// on the key array), writes its words with write-through stores, waits for them, and publishes with one CAS
// of the slot from 0; the publisher appends the entry to the queue (the next frontier). A loser reads the
// winner's slot: same tag and same words -> the state is present and the loser's entry is dead (flagged,
// pushed onto the free ring for later levels); otherwise it probes on with its entry in hand. A slot never
// changes once written, so a probe sequence only moves forward and ends after at most tmask + 1 slots.
__device__ __forceinline__ void reach_drop(const ReachArgs& a, uint32_t e) {
    a.mark[e] = REACH_DEAD;  // marks and ring entries are read by later launches only
    a.free_ring[__hip_atomic_fetch_add(a.ctl + REACH_FREE_TAIL, 1u, RLX, AGENT) & a.fmask] = e;
}

template <int W, bool INSERT>
__device__ uint32_t reach_find(const ReachArgs& a, const uint64_t (&s)[W]) {
    const uint64_t h = reach_hash<W>(s);
    const uint32_t tag = (uint32_t)(h >> 32);
    uint32_t slot = (uint32_t)h & a.tmask, mine = REACH_NONE;
    for (uint32_t probe = 0; probe <= a.tmask; ++probe, slot = (slot + 1u) & a.tmask) {
        unsigned long long v = ld64(a.table + slot);
        if (v == 0) {
            if constexpr (!INSERT) return REACH_NONE;
            if (mine == REACH_NONE) {
                if (ld32(a.ctl + REACH_COUNT) >= a.max_states) {
                    // the count may have just been raised by this very state's publish: look again, after the
                    // count, before calling it an overflow. Order: the publisher adds to the count only once
                    // its CAS has returned (the add is behind a branch on the CAS result), and this second
                    // slot load is issued only once the count's value is here (it is behind a branch on it);
                    // both words are served at agent scope. Were the order ever lost, the outcome is a
                    // spurious complete = 0, never a wrong set.
                    v = ld64(a.table + slot);
                    if (v == 0) {
                        raise_flag(a.ctl + REACH_OVERFLOW);
                        return REACH_NONE;
                    }
                } else {
                    if (a.free_any) {
                        const uint32_t q = __hip_atomic_fetch_add(a.ctl + REACH_FREE_HEAD, 1u, RLX, AGENT);
                        if ((int32_t)(a.free_limit - q) > 0) mine = a.free_ring[q & a.fmask];
                    }
                    if (mine == REACH_NONE) mine = __hip_atomic_fetch_add(a.ctl + REACH_KEYS, 1u, RLX, AGENT);
                    if (mine >= a.key_cap) {  // nothing of this entry exists: nothing to drop
                        raise_flag(a.ctl + REACH_OVERFLOW);
                        return REACH_NONE;
                    }
                    unsigned long long* kw = reinterpret_cast<unsigned long long*>(a.keys) + (uint64_t)mine * W;
#pragma unroll
                    for (int k = 0; k < W; ++k) __hip_atomic_store(kw + k, (unsigned long long)s[k], RLX, AGENT);
                    a.mark[mine] = 0;  // read by later launches only
                    // Publish order without a release fence (an agent-scope release writes back the whole
                    // L2, ~1.7 us per insert): the key words above are agent-scope atomic stores, i.e.
                    // write-through past this XCD's L2, and vmcnt(0) holds the wave until they are
                    // acknowledged -- only then is the CAS below issued. The "memory" clobber keeps the
                    // compiler from moving either side across it. A reader takes the entry index out of the
                    // slot word it loaded, so its key loads (agent-scope atomic loads, which bypass L1)
                    // cannot be issued before that slot load has returned.
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            }
            if (v == 0) {
                unsigned long long expect = 0;
                const unsigned long long want = ((unsigned long long)tag << 32) | (unsigned long long)(mine + 1u);
                if (__hip_atomic_compare_exchange_strong(a.table + slot, &expect, want, RLX, RLX, AGENT)) {
                    __hip_atomic_fetch_add(a.ctl + REACH_COUNT, 1u, RLX, AGENT);
                    const uint32_t p = __hip_atomic_fetch_add(a.ctl + REACH_QTAIL, 1u, RLX, AGENT);
                    if (p < a.key_cap) a.queue[p] = mine;  // one append per live entry: p < key_cap
                    return mine;
                }
                v = expect;
            }
        }
        if ((uint32_t)(v >> 32) == tag) {
            const uint32_t j = (uint32_t)v - 1u;
            const unsigned long long* kw = reinterpret_cast<const unsigned long long*>(a.keys) + (uint64_t)j * W;
            bool same = true;
#pragma unroll
            for (int k = 0; k < W; ++k) same &= ld64(kw + k) == (unsigned long long)s[k];
            if (same) {
                if (mine != REACH_NONE) reach_drop(a, mine);
                return j;
            }
        }
    }
    if constexpr (INSERT) {  // every slot taken by other states
        raise_flag(a.ctl + REACH_OVERFLOW);
        if (mine != REACH_NONE) reach_drop(a, mine);
    }
    return REACH_NONE;
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
            flip_bit<W>(t, i);
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
        raise_flag(a.ctl + REACH_MISSING);
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
            flip_bit<W>(x, i);
            const uint32_t j = reach_find<W, false>(a, x);
            if (j == REACH_NONE || ld32(a.mark + j) == a.epoch) continue;
            if (!can_flip_at<W, KIND>(x, i, tbl, a)) continue;
            if (__hip_atomic_exchange(a.mark + j, a.epoch, RLX, AGENT) != a.epoch) {
                const uint32_t p = __hip_atomic_fetch_add(a.ctl + REACH_QTAIL, 1u, RLX, AGENT);
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
            __hip_atomic_fetch_and(a.hull + k, (unsigned long long)all[k], RLX, AGENT);
            __hip_atomic_fetch_or(a.hull + W + k, (unsigned long long)any[k], RLX, AGENT);
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
