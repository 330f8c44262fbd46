// pbn_keytable.hpp -- the find-or-insert walk of the device hash tables that kernels insert into while other lanes
// read them: the reach set (pbn_reach.hip) and the state census (pbn_census.hpp).
//
// One definition for the kernels and for the host models of both tables (ReachModel below, CensusModel in
// pbn_census.hpp; tests/host/keytable_check.cpp, tests/host/census_check.cpp): this part includes no HIP header,
// and the walk reaches memory and the table's bookkeeping only through two policies.
//
// Layout:
//   table [tmask + 1] u64  open addressing, linear probing from the low hash bits: 0 = empty, else
//                          hash tag << 32 | entry + 1. A slot is written once, by a CAS from 0, and never changes.
//   keys  [entries][W] u64 entry e's words, written by the one lane that holds e before it publishes e.
//
// Protocol. An inserter that reaches an empty slot takes an entry nobody else knows of (take), writes its words,
// waits for them and publishes with one CAS of the slot from 0 (published). A loser reads the winner's slot word:
// same tag and same words -> the key is present, the loser returns the winner's entry and hands its own back
// (unused); otherwise it probes on with its entry in hand. Slots never change once written, so a walk only moves
// forward and ends after at most tmask + 1 slots (full). No lane waits for another; every loop is bounded.
//
// Ordering on the device, without a release fence (an agent-scope release writes back the whole L2, ~1.7 us per
// insert). Words another lane may read or write within the same launch go through agent-scope atomics on both
// sides: the per-XCD L2s are not coherent with each other and an L1 is not refreshed by other CUs' stores.
//   - Writer: the key words are agent-scope atomic stores, i.e. written through past this XCD's L2, and
//     s_waitcnt vmcnt(0) holds the wave until they are acknowledged; only then is the CAS issued. The "memory"
//     clobber keeps the compiler from moving either side across the wait.
//   - Reader: it takes the entry index out of the slot word it loaded, so its key loads (agent-scope atomic loads,
//     which bypass L1) cannot be issued before that slot load has returned.
//   - No entry to insert with (take() == NONE): the last entry may have gone to this very key a moment ago, so the
//     slot is read a second time before the walk gives up (none). For a limit kept in a counter (the reach set's
//     count) the order holds: a publisher adds to the counter only once its CAS has returned, and the second slot
//     load is behind a branch on the counter's value; both words are served at agent scope. A publish that lands
//     after the second look is missed: the reach set then reports a spurious complete = 0 and the census drops a
//     visit of a state it holds -- never a wrong set, never a count above the true one. The second look is taken
//     whatever made take() fail; the reach set once raised overflow at once for an entry past its key array.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <type_traits>
#include <utility>
#include <vector>

#include "pbn_params.hpp"

#ifndef PBN_HD  // as in pbn_reach_rule.hpp
#if defined(__HIPCC__)  // the compiler's own attributes: no HIP header needed for them
#define PBN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PBN_HD inline
#endif
#endif

namespace pbn {

constexpr uint32_t KEYTABLE_NONE = 0xFFFFFFFFu;  // no entry (REACH_NONE, CENSUS_NONE)

// The power of two >= x, at least 64: slot counts (x = 2 max_states: load <= 1/2) and ring capacities.
constexpr uint32_t keytable_pow2(uint64_t x) {
    uint64_t s = 64;
    while (s < x) s *= 2;
    return (uint32_t)s;  // callers keep x <= 2^31
}

// The hash of every state table here, the read-only set of pbn_stateset.hpp included.
template <int W>
PBN_HD uint64_t stateset_hash(const uint64_t (&s)[W]) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < W; ++k) {
        h = (h ^ s[k]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}

// Entry index of key s, or KEYTABLE_NONE. INSERT: add it if absent (KEYTABLE_NONE: it could not be added).
//   Mem: load_slot(slot), store_key(e, s) (returns once the words are visible), cas_slot(slot, want, found) (true:
//        published; else found = the word that is there), load_key(e, W, k).
//   Tab: take()           an entry nobody else knows of, or KEYTABLE_NONE
//        none()           take() gave none and the slot, read again, is still empty
//        published(mine)  this lane's CAS won
//        unused(mine)     an entry in hand was not published: the key is held under another entry, or no slot is left
//        full()           an insert walk found every slot taken by other keys
template <int W, bool INSERT, class Mem, class Tab>
PBN_HD uint32_t keytable_walk(Mem&& m, Tab&& t, uint32_t tmask, const uint64_t (&s)[W]) {
    const uint64_t h = stateset_hash<W>(s);
    const uint32_t tag = (uint32_t)(h >> 32);
    uint32_t slot = (uint32_t)h & tmask, mine = KEYTABLE_NONE;
    for (uint32_t probe = 0; probe <= tmask; ++probe, slot = (slot + 1u) & tmask) {
        uint64_t v = m.load_slot(slot);
        if (v == 0) {
            if constexpr (!INSERT) return KEYTABLE_NONE;
            if (mine == KEYTABLE_NONE) {
                mine = t.take();
                if (mine == KEYTABLE_NONE) {
                    v = m.load_slot(slot);
                    if (v == 0) {
                        t.none();
                        return KEYTABLE_NONE;
                    }
                } else {
                    m.store_key(mine, s);
                }
            }
            if (v == 0) {
                const uint64_t want = ((uint64_t)tag << 32) | (uint64_t)(mine + 1u);
                // `want` before the call and `found` a word of its own: with `want` built in the argument list, or v
                // itself handed to the hook, the kernels' VGPR counts go up (4 to 9 in k_census, 1 to 2 in k_reach_seed
                // and k_reach_expand) and occupancy drops at some W (tools/kernel_isa_diff.py)
                uint64_t found = 0;
                if (m.cas_slot(slot, want, found)) {
                    t.published(mine);
                    return mine;
                }
                v = found;
            }
        }
        if ((uint32_t)(v >> 32) == tag) {
            const uint32_t j = (uint32_t)v - 1u;
            bool same = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < W; ++k) same &= m.load_key(j, W, k) == s[k];
            if (same) {
                if (mine != KEYTABLE_NONE) t.unused(mine);
                return j;
            }
        }
    }
    if constexpr (INSERT) {
        t.full();
        if (mine != KEYTABLE_NONE) t.unused(mine);
    }
    return KEYTABLE_NONE;
}

// ---------------------------------------------------------------- the host side: one visitor at a time
// Memory policy over vectors. `rival`, if set, runs once between this walk's look at an empty slot and its CAS: a
// test lets another lane publish there first.
struct KeytableHostMem {
    std::vector<uint64_t>&table, &keys;
    std::function<void()> rival;
    uint64_t load_slot(uint32_t slot) const { return table[slot]; }
    template <int W>
    void store_key(uint32_t e, const uint64_t (&s)[W]) {
        for (int k = 0; k < W; ++k) keys[(size_t)e * W + k] = s[k];
    }
    bool cas_slot(uint32_t slot, uint64_t want, uint64_t& found) {
        if (rival) std::exchange(rival, nullptr)();
        found = table[slot];
        if (found == 0) table[slot] = want;
        return found == 0;
    }
    uint64_t load_key(uint32_t e, int W, int k) const { return keys[(size_t)e * W + k]; }
};

struct KeytableHostCtl {  // counters: sequential
    static uint32_t ld(const uint32_t* p) { return *p; }
    static uint32_t add(uint32_t* p) { return (*p)++; }
    static void raise(uint32_t* p) { *p = 1u; }
};

// The reach set's bookkeeping (ReachArgs, pbn_params.hpp), for the kernels and the model; Ctl: how the counters are
// reached. Marks, ring entries and queue entries are read by later launches only: plain stores.
template <class Ctl>
struct ReachTable {
    const ReachArgs& a;
    PBN_HD uint32_t take() const {
        if (Ctl::ld(a.ctl + REACH_COUNT) >= a.max_states) return KEYTABLE_NONE;
        uint32_t mine = KEYTABLE_NONE;
        if (a.free_any) {
            const uint32_t q = Ctl::add(a.ctl + REACH_FREE_HEAD);
            if ((int32_t)(a.free_limit - q) > 0) mine = a.free_ring[q & a.fmask];
        }
        if (mine == KEYTABLE_NONE) mine = Ctl::add(a.ctl + REACH_KEYS);
        if (mine >= a.key_cap) return KEYTABLE_NONE;  // nothing of this entry exists: nothing to drop
        a.mark[mine] = 0;
        return mine;
    }
    PBN_HD void none() const { Ctl::raise(a.ctl + REACH_OVERFLOW); }
    PBN_HD void full() const { Ctl::raise(a.ctl + REACH_OVERFLOW); }
    PBN_HD void published(uint32_t mine) const {  // counted, and appended to the queue: the next frontier
        Ctl::add(a.ctl + REACH_COUNT);
        const uint32_t p = Ctl::add(a.ctl + REACH_QTAIL);
        if (p < a.key_cap) a.queue[p] = mine;  // one append per live entry: p < key_cap
    }
    PBN_HD void unused(uint32_t mine) const {  // dead: flagged, and on the free ring for later levels
        a.mark[mine] = REACH_DEAD;
        a.free_ring[Ctl::add(a.ctl + REACH_FREE_TAIL) & a.fmask] = mine;
    }
};

// Run-time words per state -> compile-time (host side; the kernels' dispatch is by_words, pbn_launch.hpp).
template <class F>
inline auto stateset_by_words(int W, F&& f) {
    switch (W) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

// The walk of a host model: key [W] into an array of compile-time length, then keytable_walk.
template <bool INSERT, class Tab>
inline uint32_t keytable_find_host(int W, KeytableHostMem& m, Tab&& t, uint32_t tmask, const uint64_t* key) {
    return stateset_by_words(W, [&](auto w) -> uint32_t {
        constexpr int WW = decltype(w)::value;
        uint64_t s[WW];
        for (int k = 0; k < WW; ++k) s[k] = key[k];
        return keytable_walk<WW, INSERT>(m, t, tmask, s);
    });
}

// Sequential model of the reach set: the layout, counters and level protocol of pbn_reach_closure, one walk at a time.
struct ReachModel {
    int W = 0;
    ReachArgs a{};  // the table policy's view: pointers into the vectors below
    std::vector<uint64_t> table, keys;
    std::vector<uint32_t> mark, queue, free_ring;
    uint32_t ctl[REACH_CTL_WORDS] = {};

    void init(int n_words, uint32_t max_states, uint32_t key_cap) {
        W = n_words;
        a = ReachArgs{};
        a.max_states = max_states;
        a.key_cap = key_cap;
        a.tmask = keytable_pow2(2ull * max_states) - 1u;
        a.fmask = keytable_pow2(key_cap) - 1u;
        table.assign((size_t)a.tmask + 1, 0);
        keys.assign((size_t)key_cap * W, 0);
        mark.assign(key_cap, 0);
        queue.assign(key_cap, 0);
        free_ring.assign((size_t)a.fmask + 1, 0);
        for (uint32_t& c : ctl) c = 0;
        a.mark = mark.data();
        a.queue = queue.data();
        a.free_ring = free_ring.data();
        a.ctl = ctl;
    }
    // Between two levels: takers that ran past the last level's limit took nothing; what the last level pushed is
    // complete now and may be taken.
    void next_level() {
        if ((int32_t)(ctl[REACH_FREE_HEAD] - a.free_limit) > 0) ctl[REACH_FREE_HEAD] = a.free_limit;
        a.free_limit = ctl[REACH_FREE_TAIL];
        a.free_any = a.free_limit != ctl[REACH_FREE_HEAD];
    }
    template <bool INSERT>
    uint32_t find(const uint64_t* key, std::function<void()> rival = nullptr) {
        KeytableHostMem m{table, keys, std::move(rival)};
        return keytable_find_host<INSERT>(W, m, ReachTable<KeytableHostCtl>{a}, a.tmask, key);
    }
};

}  // namespace pbn

// ---------------------------------------------------------------- the device side
#if defined(__HIPCC__)
namespace pbn {

#define KEYTABLE_RLX __ATOMIC_RELAXED
#define KEYTABLE_AGENT __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ unsigned long long keytable_ld64(const unsigned long long* p) {
    return __hip_atomic_load(p, KEYTABLE_RLX, KEYTABLE_AGENT);
}
__device__ __forceinline__ uint32_t keytable_ld32(const uint32_t* p) {
    return __hip_atomic_load(p, KEYTABLE_RLX, KEYTABLE_AGENT);
}

struct KeytableDeviceMem {  // see "Ordering on the device" above
    unsigned long long *table, *keys;
    __device__ __forceinline__ uint64_t load_slot(uint32_t slot) const { return keytable_ld64(table + slot); }
    template <int W>
    __device__ __forceinline__ void store_key(uint32_t e, const uint64_t (&s)[W]) const {
        unsigned long long* kw = keys + (uint64_t)e * W;
#pragma unroll
        for (int k = 0; k < W; ++k) __hip_atomic_store(kw + k, (unsigned long long)s[k], KEYTABLE_RLX, KEYTABLE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __device__ __forceinline__ bool cas_slot(uint32_t slot, unsigned long long want, uint64_t& found) const {
        unsigned long long expect = 0;
        if (__hip_atomic_compare_exchange_strong(table + slot, &expect, want, KEYTABLE_RLX, KEYTABLE_RLX, KEYTABLE_AGENT))
            return true;
        found = expect;
        return false;
    }
    __device__ __forceinline__ uint64_t load_key(uint32_t e, int W, int k) const {
        return keytable_ld64(keys + (uint64_t)e * W + k);
    }
};

struct KeytableDeviceCtl {  // counters: agent-scope atomics
    static __device__ __forceinline__ uint32_t ld(const uint32_t* p) { return keytable_ld32(p); }
    static __device__ __forceinline__ uint32_t add(uint32_t* p) {
        return __hip_atomic_fetch_add(p, 1u, KEYTABLE_RLX, KEYTABLE_AGENT);
    }
    static __device__ __forceinline__ void raise(uint32_t* p) { __hip_atomic_store(p, 1u, KEYTABLE_RLX, KEYTABLE_AGENT); }
};

}  // namespace pbn
#endif  // __HIPCC__
