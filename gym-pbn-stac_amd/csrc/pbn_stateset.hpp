// pbn_stateset.hpp -- an exact, read-only set of packed states that a kernel can query.
//
// One definition for the host builder, the host lookup (pbn_stateset_lookup, tests/host/stateset_check.cpp) and
// the kernels of pbn_tenv.hip: this header includes no HIP header, and its functions take the table as plain
// pointers, so the same walk runs over host vectors and over device memory.
//
// Layout: open addressing with linear probing over `slots` = the power of two >= 2 S (at least 64) slots, two
// arrays addressed by the slot number alone:
//   meta [slots]     u32: 0 = empty, else label + 1
//   keys [slots][W]  u64: the member's words (zero in an empty slot)
// Both loads of a probe depend only on the slot, so a probe is one memory round trip (the reach set of
// pbn_reach.hip reads a tag word and then the entry it points at: two). A keys row is 8 W bytes: at W = 4 one
// 32-B sector.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pbn_keytable.hpp"  // PBN_HD, stateset_hash, keytable_pow2, stateset_by_words

namespace pbn {

constexpr uint64_t STATESET_MAX_STATES = 1ull << 24;  // 2^25 slots: 128 MiB of meta + 256 MiB of keys at W = 1
constexpr int STATESET_MAX_WORDS = 8;

constexpr uint32_t stateset_slots(uint64_t n_states) {
    return keytable_pow2(2 * n_states);  // n_states <= 2^24: at most 2^25
}

// Label of state s, or -1. The walk starts at the state's home slot and ends at an empty slot, at the member,
// or after `slots` probes (a full table). The key words are loaded before the meta word is tested: an empty
// slot's row is in bounds (and zero), and the two loads go out together.
template <int W>
PBN_HD int32_t stateset_lookup(const uint64_t (&s)[W], const uint32_t* meta, const uint64_t* keys, uint32_t slots,
                                  uint32_t* probes = nullptr) {
    const uint32_t mask = slots - 1u;
    uint32_t slot = (uint32_t)stateset_hash<W>(s) & mask;
    for (uint32_t probe = 0; probe < slots; ++probe, slot = (slot + 1u) & mask) {
        const uint32_t m = meta[slot];
#if defined(__HIP_DEVICE_COMPILE__)  // device tables start on an allocation: an even-W row is 16-B aligned
        const uint64_t* row =
            static_cast<const uint64_t*>(__builtin_assume_aligned(keys + (uint64_t)slot * W, W % 2 == 0 ? 16 : 8));
#else
        const uint64_t* row = keys + (uint64_t)slot * W;
#endif
        uint64_t diff = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < W; ++k) diff |= row[k] ^ s[k];
        if (probes) *probes = probe + 1u;
        if (m == 0) return -1;
        if (diff == 0) return (int32_t)(m - 1u);
    }
    return -1;
}

// The host copy of a set: what the builder makes, the host lookup reads and the upload copies.
struct StateSetTable {
    int n_nodes = 0, W = 0;
    uint32_t slots = 0;
    uint32_t max_probe = 0;  // the longest walk of any member (1 = at home); 0 for the empty set
    uint64_t n_states = 0;   // distinct members
    int32_t max_label = -1;  // the largest label (-1 for the empty set)
    std::vector<uint32_t> meta;
    std::vector<uint64_t> keys;
    // AND / OR over the members' words ([W] each; the empty set: the N-bit mask / 0). care = ~(all ^ any) names the
    // nodes every member agrees on: a state with (s ^ all) & care != 0 is no member (stateset_hull_rejects), which
    // k_env_set (pbn_env_set.hip) tests before it touches the table.
    std::vector<uint64_t> hull_all, hull_any;
};

// The hull pre-filter: true only for states that differ from every member in a node all members agree on.
template <int W>
PBN_HD bool stateset_hull_rejects(const uint64_t (&s)[W], const uint64_t (&all)[W], const uint64_t (&any)[W]) {
    uint64_t d = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < W; ++k) d |= (s[k] ^ all[k]) & ~(all[k] ^ any[k]);
    return d != 0;
}

enum {
    STATESET_OK = 0,
    STATESET_E_SHAPE = 1,      // n_nodes outside [1, 64 * 8], or more than STATESET_MAX_STATES rows
    STATESET_E_STRAY_BITS = 2, // a row has a bit set past node N - 1
    STATESET_E_LABEL = 3,      // a label < 0
    STATESET_E_CONFLICT = 4    // one state under two labels
};

inline bool stateset_canonical(const uint64_t* row, int n_nodes, int W) {
    const int r = n_nodes & 63;
    return !r || !(row[W - 1] & ~((1ull << r) - 1ull));
}

// Sequential, in input order: each row goes into the first empty slot of its walk, so the layout is a function
// of the input alone. A row already present under the same label is dropped. *bad_row names the offending row.
inline int stateset_build(int n_nodes, const uint64_t* states, const int32_t* labels, uint64_t n_rows,
                          StateSetTable* t, uint64_t* bad_row = nullptr) {
    if (n_nodes < 1 || n_nodes > 64 * STATESET_MAX_WORDS || n_rows > STATESET_MAX_STATES) return STATESET_E_SHAPE;
    const int W = (n_nodes + 63) / 64;
    t->n_nodes = n_nodes;
    t->W = W;
    t->slots = stateset_slots(n_rows);
    t->max_probe = 0;
    t->n_states = 0;
    t->max_label = -1;
    t->hull_all.assign(W, ~0ull);
    if (n_nodes & 63) t->hull_all[W - 1] = (1ull << (n_nodes & 63)) - 1ull;
    t->hull_any.assign(W, 0ull);
    t->meta.assign(t->slots, 0u);
    t->keys.assign((size_t)t->slots * W, 0ull);
    const uint32_t mask = t->slots - 1u;
    return stateset_by_words(W, [&](auto w) -> int {
        constexpr int WW = decltype(w)::value;
        for (uint64_t r = 0; r < n_rows; ++r) {
            if (bad_row) *bad_row = r;
            uint64_t s[WW];
            for (int k = 0; k < WW; ++k) s[k] = states[r * WW + k];
            if (!stateset_canonical(s, n_nodes, WW)) return STATESET_E_STRAY_BITS;
            const int32_t label = labels ? labels[r] : 0;
            if (label < 0) return STATESET_E_LABEL;
            uint32_t slot = (uint32_t)stateset_hash<WW>(s) & mask;
            for (uint32_t probe = 1;; ++probe, slot = (slot + 1u) & mask) {  // load <= 1/2: an empty slot exists
                if (t->meta[slot] == 0) {
                    t->meta[slot] = (uint32_t)label + 1u;
                    for (int k = 0; k < WW; ++k) t->keys[(size_t)slot * WW + k] = s[k];
                    for (int k = 0; k < WW; ++k) {
                        t->hull_all[k] &= s[k];
                        t->hull_any[k] |= s[k];
                    }
                    t->n_states++;
                    if (label > t->max_label) t->max_label = label;
                    if (probe > t->max_probe) t->max_probe = probe;
                    break;
                }
                bool same = true;
                for (int k = 0; k < WW; ++k) same = same && t->keys[(size_t)slot * WW + k] == s[k];
                if (same) {
                    if (t->meta[slot] != (uint32_t)label + 1u) return STATESET_E_CONFLICT;
                    break;
                }
            }
        }
        return STATESET_OK;
    });
}

// labels [n] of states [n][W] over the host copy; a query with stray bits is no member (-1).
inline void stateset_lookup_host(const StateSetTable& t, const uint64_t* states, uint64_t n, int32_t* labels) {
    stateset_by_words(t.W, [&](auto w) -> int {
        constexpr int WW = decltype(w)::value;
        for (uint64_t r = 0; r < n; ++r) {
            uint64_t s[WW];
            for (int k = 0; k < WW; ++k) s[k] = states[r * WW + k];
            labels[r] = stateset_lookup<WW>(s, t.meta.data(), t.keys.data(), t.slots);
        }
        return 0;
    });
}

}  // namespace pbn
