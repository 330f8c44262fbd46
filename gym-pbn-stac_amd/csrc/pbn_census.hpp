// pbn_census.hpp -- the state census: an exact multiset of packed states that kernels feed.
//
// The reference counts visits of full states in a defaultdict keyed by the state tuple (statistical_attractors,
// pbn_target.py:538-560, pbn_target_multi.py:465-487). Here the dict is a device table: one u64 count per distinct
// state, found or inserted without any lane waiting for another.
//
// Layout (the table and keys of pbn_keytable.hpp, where the find-or-insert walk and its ordering argument are, plus
// counts):
//   table  [slots] u64   slots = the power of two >= 2 max_states, at least 64; unchanged until a clear.
//   keys   [key_cap][W] u64   entry e's words; key_cap = max_states + CENSUS_SLACK. An entry is LIVE once a slot
//                        names it, DEAD while it is reserved and unpublished: its inserter lost the publish to an
//                        equal key or found no slot.
//   counts [key_cap] u64      bits 0..62: visits of entry e; bit 63 (CENSUS_OVER): the entry was published after
//                        max_states others. Only a live entry is ever added to, and the lane that publishes an
//                        entry counts at least one visit on it before its launch ends: between launches an entry is
//                        live iff its visits are not 0. The read-out's compaction (census_compact) relies on that.
//   ring   [2][ring_cap] u32  dead entries between launches. Within a launch a lane keeps its dead entry as a spare
//                        for its own next insert, so a launch holds at most one dead entry per lane (<= CENSUS_SLACK
//                        lanes: the host caps the grid), however many lanes race for one new key. A lane that ends
//                        with a spare pushes it onto ring `parity`; inserters take from ring `parity ^ 1`, whose
//                        tail no lane of this launch moves, so what a taker reads was written by an earlier launch.
//                        Every dead entry is thus in a lane's hands or on a ring, and a ring's entries go back into
//                        use before the end of keys does.
//   ctl    CENSUS_CTL_WORDS u32, then dropped (u64) and adds (u64): see the enum.
//
// max_states is kept without a lane ever holding a place it may not use: the winner of a publish draws its rank from
// CENSUS_COUNT after the CAS, and a rank >= max_states sets CENSUS_OVER on the entry's count. The state stays in
// the table, so later visits find it and no lane inserts it twice, but the read-out reports the max_states entries
// of rank < max_states only and adds the visits of the others to `dropped`. A reservation taken before the CAS
// instead would be held by every loser of a race for one key, and 300 lanes inserting 8 states would fill a table of
// 64. The slack entries bound the states past max_states that can be held this way; beyond them, and for a walk that
// finds every slot taken, the visit is dropped on the device.
//
// This part includes no HIP header: sizing, the sample-point rule, a sequential model of the same layout and the
// compaction run on the host (pbn_abi_census.cpp, tests/host/census_check.cpp). What the kernels run is below the
// __HIPCC__ guard.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pbn_keytable.hpp"
#include "pbn_params.hpp"
#include "pbn_stateset.hpp"

namespace pbn {

constexpr uint64_t CENSUS_MAX_STATES = STATESET_MAX_STATES;  // 2^24: what a StateSet takes
constexpr uint32_t CENSUS_MAX_UPDATES = 65536;  // per launch (the TENV_MACRO_MAX_T precedent): a launch stays bounded
constexpr uint32_t CENSUS_NONE = KEYTABLE_NONE;
// entries past max_states, one for every lane of a launch to hold dead: 2,048 workgroups of BLOCK lanes, which is
// what 256 CUs keep resident at most (8 workgroups of 256 threads each)
constexpr uint32_t CENSUS_SLACK = 1u << 19;
constexpr int CENSUS_MAX_GRID = (int)(CENSUS_SLACK / BLOCK);
constexpr uint64_t CENSUS_OVER = 1ull << 63;  // in a count word: published past max_states, not reported

enum {
    CENSUS_KEYS = 0,    // entries taken from the end of keys (may run past key_cap by the lanes in flight: clamped)
    CENSUS_COUNT = 1,   // live entries: ranks drawn by successful publishes
    CENSUS_HEAD0 = 2,   // ring 0: entries taken
    CENSUS_HEAD1 = 3,
    CENSUS_TAIL0 = 4,   // ring 0: entries pushed
    CENSUS_TAIL1 = 5,
    CENSUS_CTL_WORDS = 8,
    // after the u32 words, two u64 counters
    CENSUS_CTL_BYTES = 4 * CENSUS_CTL_WORDS + 16
};

constexpr uint32_t census_slots(uint64_t max_states) {
    return keytable_pow2(2 * max_states);  // max_states <= 2^24: at most 2^25
}

constexpr uint32_t census_key_cap(uint64_t max_states, uint32_t slack = CENSUS_SLACK) {
    return (uint32_t)max_states + slack;
}

constexpr uint32_t census_ring_cap(uint32_t key_cap) { return keytable_pow2(key_cap); }  // every entry fits at once

// Sample points: "the state after i updates" is counted for i = first, first + stride, ... <= n_updates.
constexpr uint64_t census_samples(uint32_t n_updates, uint32_t first, uint32_t stride) {
    return first > n_updates || stride == 0 ? 0 : (uint64_t)(n_updates - first) / stride + 1;
}

// The same rule as the kernel walks it: hit(i) for i = 0, 1, 2, ... in order.
struct CensusSampler {
    uint64_t next;  // 64 bits: first + k * stride passes 2^32 before it passes n_updates for a large stride
    uint32_t stride;
    PBN_HD bool hit(uint32_t i) {
        if ((uint64_t)i != next) return false;
        next += stride;
        return true;
    }
};

struct CensusArgs {
    uint64_t* state;  // [B][W]
    const void* img;  // network image (either kind)
    NetLayout L;
    uint64_t B, env_base, seed;
    uint64_t update;  // the batch's update counter: update i of the call is update `update + i` of every env
    uint32_t n_updates, first, stride;
    uint32_t parity;  // ring pushed onto by this launch; the other one is taken from
    uint64_t mask[MAX_WORDS];  // the projection (the first W words are read); all ones: the full state
    unsigned long long* table;
    uint64_t* keys;
    unsigned long long* counts;
    uint32_t* ring;  // [2][ring_mask + 1]
    uint32_t* ctl;
    unsigned long long* dropped;  // visits of states that were absent and could not be inserted
    unsigned long long* adds;     // count adds issued (measurement: 1 - adds / sample points = the pending-run hit rate)
    uint32_t tmask, key_cap, max_states, ring_mask;
};

void* census_kernel(int W, int kind);  // pbn_census.hip; launched by launch_lane_env with planes at L.bytes

// ---------------------------------------------------------------- compaction (the read-out)
// Reported entries of keys / counts [n_entries] in entry order: states [n][W], counts [n]. Dead entries (no visits)
// are skipped; the visits of entries past max_states (CENSUS_OVER) go to *over_visits. Returns n; writes nothing
// past `cap` rows (a return above cap: the caller's arrays were too small).
inline uint64_t census_compact(const uint64_t* keys, const uint64_t* counts, uint64_t n_entries, int W,
                               uint64_t* states, uint64_t* out_counts, uint64_t cap, uint64_t* over_visits = nullptr) {
    uint64_t n = 0, over = 0;
    for (uint64_t e = 0; e < n_entries; ++e) {
        const uint64_t visits = counts[e] & ~CENSUS_OVER;
        if (visits == 0) continue;
        if (counts[e] & CENSUS_OVER) {
            over += visits;
            continue;
        }
        if (n < cap) {
            if (states)
                for (int k = 0; k < W; ++k) states[n * (uint64_t)W + k] = keys[e * (uint64_t)W + k];
            if (out_counts) out_counts[n] = visits;
        }
        n++;
    }
    if (over_visits) *over_visits = over;
    return n;
}

// ---------------------------------------------------------------- sequential model of the device table
// One visitor at a time over the same slot / entry layout and the same reserve order (ring first, then the end of
// keys). lose_next_publish() stands for a lane that lost a publish race and ended with its entry as a spare: it
// reserves an entry and pushes it onto the launch's ring.
struct CensusModel {
    int W = 0;
    uint32_t tmask = 0, key_cap = 0, max_states = 0, ring_mask = 0, parity = 0;
    std::vector<uint64_t> table, keys, counts;
    std::vector<uint32_t> ring;
    uint32_t ctl[CENSUS_CTL_WORDS] = {};
    uint64_t dropped = 0, visits = 0;

    void init(int n_words, uint64_t n_max_states, uint32_t slack) {
        W = n_words;
        max_states = (uint32_t)n_max_states;
        key_cap = census_key_cap(n_max_states, slack);
        tmask = census_slots(n_max_states) - 1u;
        ring_mask = census_ring_cap(key_cap) - 1u;
        table.assign((size_t)tmask + 1, 0);
        keys.assign((size_t)key_cap * W, 0);
        counts.assign(key_cap, 0);
        ring.assign(2 * ((size_t)ring_mask + 1), 0);
        for (uint32_t& c : ctl) c = 0;
        dropped = visits = 0;
        parity = 0;
    }
    void next_launch() { parity ^= 1u; }
    uint32_t n_entries() const { return ctl[CENSUS_KEYS] < key_cap ? ctl[CENSUS_KEYS] : key_cap; }

    uint32_t reserve() {
        const uint32_t t = parity ^ 1u;
        if ((int32_t)(ctl[CENSUS_TAIL0 + t] - ctl[CENSUS_HEAD0 + t]) > 0)
            return ring[(size_t)t * (ring_mask + 1) + (ctl[CENSUS_HEAD0 + t]++ & ring_mask)];
        if (ctl[CENSUS_KEYS] < key_cap) return ctl[CENSUS_KEYS]++;
        return CENSUS_NONE;
    }
    void retire(uint32_t e) { ring[(size_t)parity * (ring_mask + 1) + (ctl[CENSUS_TAIL0 + parity]++ & ring_mask)] = e; }
    void lose_next_publish() {
        const uint32_t e = reserve();
        if (e != CENSUS_NONE) retire(e);
    }
    // A lane that reached an empty slot together with others and lost the publish: an entry taken in vain, now its
    // spare (a lane that holds one already takes no second).
    void lose_race(uint32_t* spare) {
        if (*spare == CENSUS_NONE) *spare = reserve();
    }

    // The census' bookkeeping, as CensusTable has it on the device. spare: the lane's spare entry (used first; an
    // entry taken in vain comes back into it; a walk that takes none leaves it alone).
    struct Table {
        CensusModel& m;
        uint32_t& spare;
        uint32_t take() const { return spare != CENSUS_NONE ? std::exchange(spare, CENSUS_NONE) : m.reserve(); }
        void none() const {}
        void full() const {}
        void published(uint32_t mine) const {
            if (m.ctl[CENSUS_COUNT]++ >= m.max_states) m.counts[mine] |= CENSUS_OVER;
        }
        void unused(uint32_t mine) const { spare = mine; }
    };
    // Entry of key (W words), inserted if absent; CENSUS_NONE: absent, and no entry or no slot is left: keytable_walk,
    // one lane at a time. rival: another lane publishes the key between this lane's look at the empty slot and its
    // CAS (that lane's walk ends at this very slot), so this lane, entry in hand, loses and adopts.
    uint32_t find(const uint64_t* key, uint32_t* spare = nullptr, bool rival = false) {
        uint32_t none = CENSUS_NONE;
        if (!spare) spare = &none;  // a lane of its own without a spare
        KeytableHostMem mem{table, keys, nullptr};
        if (rival) mem.rival = [this, key] { (void)find(key); };
        return keytable_find_host<true>(W, mem, Table{*this, *spare}, tmask, key);
    }
    void visit(const uint64_t* key, uint64_t n = 1, uint32_t* spare = nullptr, bool rival = false) {
        visits += n;
        const uint32_t e = find(key, spare, rival);
        if (e == CENSUS_NONE)
            dropped += n;
        else
            counts[e] += n;
    }
    // The end of a lane's work: its spare goes onto the launch's ring.
    void end_lane(uint32_t* spare) {
        if (*spare != CENSUS_NONE) retire(*spare);
        *spare = CENSUS_NONE;
    }
};

}  // namespace pbn

// ---------------------------------------------------------------- the device side
#if defined(__HIPCC__)
namespace pbn {

// An entry nobody else knows of, or CENSUS_NONE. No loop: at most one add (and one add back) on the ring's head, one
// add on the key array. The ring taken from is not pushed onto in this launch, so its tail is fixed and a position
// below it holds an entry an earlier launch wrote. A lane draws a position with fetch_add; a position at or past the
// tail is no entry, and the lane takes its 1 back. The head is thus head0 + positions handed out + draws in vain not
// yet taken back: it reaches the tail only once every entry of the ring has been handed out, it never falls to a
// position that was handed out, and at the end of the launch it is head0 + entries taken, never past the tail. So a
// lane goes on to the end of keys only when the ring has nothing left, whatever the contention.
// The key counter is read before it is added to: once it has reached key_cap no lane adds again, so it passes
// key_cap by at most the lanes in flight.
__device__ __forceinline__ uint32_t census_reserve(const CensusArgs& a) {
    const uint32_t t = a.parity ^ 1u;
    const uint32_t tail = keytable_ld32(a.ctl + CENSUS_TAIL0 + t);
    if ((int32_t)(tail - keytable_ld32(a.ctl + CENSUS_HEAD0 + t)) > 0) {
        const uint32_t h = __hip_atomic_fetch_add(a.ctl + CENSUS_HEAD0 + t, 1u, KEYTABLE_RLX, KEYTABLE_AGENT);
        if ((int32_t)(tail - h) > 0) return keytable_ld32(a.ring + (size_t)t * (a.ring_mask + 1u) + (h & a.ring_mask));
        __hip_atomic_fetch_sub(a.ctl + CENSUS_HEAD0 + t, 1u, KEYTABLE_RLX, KEYTABLE_AGENT);
    }
    if (keytable_ld32(a.ctl + CENSUS_KEYS) < a.key_cap) {
        const uint32_t e = __hip_atomic_fetch_add(a.ctl + CENSUS_KEYS, 1u, KEYTABLE_RLX, KEYTABLE_AGENT);
        if (e < a.key_cap) return e;
    }
    return CENSUS_NONE;
}

// A lane's spare at the end of its work: onto this launch's ring, for later launches (its count is 0 and stays 0).
__device__ __forceinline__ void census_retire(const CensusArgs& a, uint32_t e) {
    const uint32_t p = __hip_atomic_fetch_add(a.ctl + CENSUS_TAIL0 + a.parity, 1u, KEYTABLE_RLX, KEYTABLE_AGENT);
    a.ring[(size_t)a.parity * (a.ring_mask + 1u) + (p & a.ring_mask)] = e;  // read by later launches only
}

// The census' bookkeeping for keytable_walk. `spare`: the lane's dead entry from an earlier call, used first and handed
// back if this call takes an entry it does not publish (a walk that meets no empty slot -- the common case, a key
// already held -- takes none and leaves the spare as it was). Nothing is flagged when no entry or no slot is left: the
// caller counts the visit as dropped.
struct CensusTable {
    const CensusArgs& a;
    uint32_t& spare;
    __device__ __forceinline__ uint32_t take() const {
        const uint32_t mine = spare != CENSUS_NONE ? spare : census_reserve(a);
        spare = CENSUS_NONE;
        return mine;
    }
    __device__ __forceinline__ void none() const {}
    __device__ __forceinline__ void full() const {}
    // the rank: past max_states the entry is kept (so that nobody inserts the state again) but marked, and the
    // read-out counts its visits as dropped
    __device__ __forceinline__ void published(uint32_t mine) const {
        if (KeytableDeviceCtl::add(a.ctl + CENSUS_COUNT) >= a.max_states)
            __hip_atomic_fetch_or(a.counts + mine, (unsigned long long)CENSUS_OVER, KEYTABLE_RLX, KEYTABLE_AGENT);
    }
    __device__ __forceinline__ void unused(uint32_t mine) const { spare = mine; }
};

// Entry index of key s, inserted if absent; CENSUS_NONE: absent and not insertable -- no entry is left, or every
// slot of the walk holds another key.
template <int W>
__device__ uint32_t census_find(const CensusArgs& a, const uint64_t (&s)[W], uint32_t& spare) {
    return keytable_walk<W, true>(KeytableDeviceMem{a.table, reinterpret_cast<unsigned long long*>(a.keys)},
                                  CensusTable{a, spare}, a.tmask, s);
}

// A lane's pending run: the entry of the last counted key and how many visits of it are not in memory yet.
template <int W>
struct CensusRun {
    uint64_t key[W];
    uint32_t entry;    // CENSUS_NONE: the key could not be inserted, its visits are dropped
    uint32_t pending;  // 0: no key yet
};

// One add for the whole run (or the run's visits onto the lane's dropped count).
template <int W>
__device__ __forceinline__ void census_flush(const CensusArgs& a, CensusRun<W>& r, uint64_t& dropped, uint64_t& adds) {
    if (r.pending == 0u) return;
    const bool held = r.entry != CENSUS_NONE;
    if (held) __hip_atomic_fetch_add(a.counts + r.entry, (unsigned long long)r.pending, KEYTABLE_RLX, KEYTABLE_AGENT);
    // both tallies move by a select, outside the branch: with one 64-bit tally bumped on each side of it the compiler
    // picks the tally by address and keeps the two in scratch
    adds += held ? 1u : 0u;
    dropped += held ? 0u : r.pending;
    r.pending = 0u;
}

// Counts one visit of k: the same key as the run's touches no memory.
template <int W>
__device__ __forceinline__ void census_visit(const CensusArgs& a, CensusRun<W>& r, const uint64_t (&k)[W],
                                             uint32_t& spare, uint64_t& dropped, uint64_t& adds) {
    uint64_t diff = 0;
#pragma unroll
    for (int q = 0; q < W; ++q) diff |= k[q] ^ r.key[q];
    if (r.pending != 0u && diff == 0ull) {
        r.pending++;
        return;
    }
    census_flush<W>(a, r, dropped, adds);
#pragma unroll
    for (int q = 0; q < W; ++q) r.key[q] = k[q];
    r.entry = census_find<W>(a, k, spare);
    r.pending = 1u;
}

}  // namespace pbn
#endif  // __HIPCC__
