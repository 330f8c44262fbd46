// keytable_check.cpp -- the find-or-insert walk of the device tables (csrc/pbn_keytable.hpp) on the CPU, under
// ASan + UBSan (`make keytablecheck`).
//
// No HIP, no GPU, no library: the header alone. keytable_walk is what reach_find and census_find run; here it runs
// over ReachModel -- the reach set's layout and ReachTable, its bookkeeping on both sides -- against a std::map:
// exact membership, one queue append per live entry, entries lost to a publish race marked dead and handed out again
// by the next level, and every way an insert can fail (max_states, the end of keys, a full table).
#include "pbn_keytable.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

using namespace pbn;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

using Row = std::vector<uint64_t>;
using Oracle = std::map<Row, uint32_t>;  // member -> its entry

// few distinct values per word: rows share words and differ in one of them
static Row random_row(int W) {
    Row r(W);
    for (int k = 0; k < W; k++) r[k] = rnd() % 3 ? rnd() % 7 : 0x8000000000000000ull | (rnd() % 7);
    return r;
}

static std::vector<Row> distinct_rows(int W, size_t n, const Oracle* avoid = nullptr) {
    std::set<Row> seen;
    std::vector<Row> out;
    while (out.size() < n) {
        Row r = random_row(W);
        if (W == 1) r[0] = rnd();  // 14 values per word are too few for one word
        if ((avoid && avoid->count(r)) || !seen.insert(r).second) continue;
        out.push_back(r);
    }
    return out;
}

static uint32_t home_slot(int W, const Row& r, uint32_t tmask) {
    return stateset_by_words(W, [&](auto w) -> uint32_t {
        constexpr int WW = decltype(w)::value;
        uint64_t s[WW];
        for (int k = 0; k < WW; ++k) s[k] = r[k];
        return (uint32_t)stateset_hash<WW>(s) & tmask;
    });
}

// The set is the oracle's: the count, one queue append per live entry, every member found under its entry with its
// words, no dead entry among them, and no other key found.
static void check_set(ReachModel& m, const Oracle& ref) {
    CHECK(m.ctl[REACH_COUNT] == ref.size() && m.ctl[REACH_QTAIL] == ref.size());
    std::set<uint32_t> queued(m.queue.begin(), m.queue.begin() + m.ctl[REACH_QTAIL]), live;
    for (auto& kv : ref) {
        CHECK(m.find<false>(kv.first.data()) == kv.second);
        CHECK(kv.second < m.a.key_cap && m.mark[kv.second] != REACH_DEAD);
        for (int k = 0; k < m.W; k++) CHECK(m.keys[(size_t)kv.second * m.W + k] == kv.first[k]);
        CHECK(live.insert(kv.second).second);  // no entry under two keys
    }
    CHECK(queued == live);  // each live entry exactly once: QTAIL appends, as many distinct entries
    for (const Row& r : distinct_rows(m.W, 50, &ref)) CHECK(m.find<false>(r.data()) == REACH_NONE);
}

// Every entry on the free ring's positions [from, tail) is dead, distinct and no member's.
static std::set<uint32_t> ring_entries(const ReachModel& m, uint32_t from, const Oracle& ref) {
    std::set<uint32_t> dead, live;
    for (auto& kv : ref) live.insert(kv.second);
    for (uint32_t q = from; q != m.ctl[REACH_FREE_TAIL]; q++) {
        const uint32_t e = m.free_ring[q & m.a.fmask];
        CHECK(e < m.a.key_cap && m.mark[e] == REACH_DEAD && !live.count(e));
        CHECK(dead.insert(e).second);
    }
    return dead;
}

// An insert that loses the publish to a rival inserting the same key: the rival's entry is adopted.
static uint32_t insert_losing(ReachModel& m, const Row& r) {
    uint32_t rival = REACH_NONE;
    const uint32_t e = m.find<true>(r.data(), [&] { rival = m.find<true>(r.data()); });
    CHECK(rival != REACH_NONE && e == rival);
    return e;
}

static void check_inserts(int W, bool rivals) {
    ReachModel m;
    m.init(W, 4096, 4096 + 64);
    CHECK(m.a.tmask + 1 == 8192 && m.a.fmask + 1 == 8192);
    const std::vector<Row> rows = distinct_rows(W, 40);
    Oracle ref;
    uint32_t losses = 0;
    for (size_t i = 0; i < rows.size(); i++) {  // every 7th first insert loses its publish
        const bool lose = rivals && i % 7 == 6;
        ref[rows[i]] = lose ? insert_losing(m, rows[i]) : m.find<true>(rows[i].data());
        losses += lose;
        CHECK(ref[rows[i]] != REACH_NONE);
    }
    for (int v = 0; v < 3000; v++) {  // 3,000 inserts of the 40 keys; a rival has no empty slot to act at
        const Row& r = rows[rnd() % rows.size()];
        bool ran = false;
        CHECK(m.find<true>(r.data(), v % 7 == 6 ? std::function<void()>([&] { ran = true; }) : nullptr) == ref[r]);
        CHECK(!ran);
    }
    CHECK(m.ctl[REACH_COUNT] == 40 && m.ctl[REACH_OVERFLOW] == 0);
    CHECK(m.ctl[REACH_KEYS] == 40 + losses && m.ctl[REACH_FREE_TAIL] == losses && m.ctl[REACH_FREE_HEAD] == 0);
    check_set(m, ref);
    const std::set<uint32_t> dead = ring_entries(m, 0, ref);  // each loser's entry: dead, and on the ring
    CHECK(dead.size() == losses && (rivals ? losses == 5 : losses == 0));
    if (!rivals) return;

    // the next level: the ring's entries go back into use before the end of keys does, and the key array does not
    // grow while the ring has any; what this level drops is past free_limit and stays on the ring
    m.next_level();
    CHECK(m.a.free_any == 1 && m.a.free_limit == losses);
    const uint32_t keys0 = m.ctl[REACH_KEYS];
    const std::vector<Row> more = distinct_rows(W, 8, &ref);
    for (size_t i = 0; i < more.size(); i++) {
        const uint32_t e = i == 2 ? insert_losing(m, more[i]) : m.find<true>(more[i].data());
        ref[more[i]] = e;
        // insert 2 takes two entries (the loser's and the rival's): ring positions 2 and 3
        const uint32_t taken = (uint32_t)i + 1 + (i >= 2);
        if (taken <= losses) {
            CHECK(dead.count(e) && m.mark[e] == 0 && m.ctl[REACH_KEYS] == keys0);
        } else {
            CHECK(!dead.count(e) && m.ctl[REACH_KEYS] == keys0 + (taken - losses));
        }
    }
    CHECK(m.ctl[REACH_FREE_TAIL] == losses + 1 && m.ctl[REACH_OVERFLOW] == 0);
    check_set(m, ref);
    CHECK(ring_entries(m, losses, ref).size() == 1);  // this level's loser
    m.next_level();  // takers ran past the limit: the head comes back to it, the one new entry may be taken
    CHECK(m.ctl[REACH_FREE_HEAD] == losses && m.a.free_limit == losses + 1 && m.a.free_any == 1);
}

// More distinct keys than max_states: overflow is raised, the count stops at max_states, and what the set holds is
// right -- a key is held once, a refused key is absent, a held key is still found by a later insert.
static void check_max_states(int W) {
    ReachModel m;
    m.init(W, 16, 16 + 8);
    Oracle ref;
    std::set<Row> refused;
    for (const Row& r : distinct_rows(W, 64)) {
        const uint32_t e = m.find<true>(r.data());
        CHECK(m.ctl[REACH_COUNT] <= 16);
        CHECK((e == REACH_NONE) == (ref.size() == 16));
        CHECK((m.ctl[REACH_OVERFLOW] != 0) == (e == REACH_NONE || !refused.empty()));
        if (e == REACH_NONE)
            refused.insert(r);
        else
            ref[r] = e;
    }
    CHECK(ref.size() == 16 && refused.size() == 48 && m.ctl[REACH_OVERFLOW] == 1);
    CHECK(m.ctl[REACH_KEYS] == 16 && m.ctl[REACH_FREE_TAIL] == 0);  // a refused insert took no entry
    for (auto& kv : ref) CHECK(m.find<true>(kv.first.data()) == kv.second);
    for (const Row& r : refused) CHECK(m.find<false>(r.data()) == REACH_NONE);
    check_set(m, ref);
}

// The end of keys before max_states: overflow, and nothing is dropped -- no entry exists to drop.
static void check_key_cap(int W) {
    ReachModel m;
    m.init(W, 64, 10);
    Oracle ref;
    for (const Row& r : distinct_rows(W, 20)) {
        const uint32_t e = m.find<true>(r.data());
        CHECK((e == REACH_NONE) == (ref.size() == 10));
        if (e != REACH_NONE) ref[r] = e;
        CHECK((m.ctl[REACH_OVERFLOW] != 0) == (e == REACH_NONE));
    }
    CHECK(ref.size() == 10 && m.ctl[REACH_KEYS] == 20 && m.ctl[REACH_FREE_TAIL] == 0);
    check_set(m, ref);
}

// A full table: a walk that took an entry at an empty home slot, lost the slot to another key and then finds every
// slot taken raises overflow and drops its entry once; walks end after tmask + 1 probes.
static void check_full_table(int W) {
    ReachModel m;
    m.init(W, 32, 48);
    const std::vector<Row> rows = distinct_rows(W, 9);
    const Row& other = rows[0];
    size_t pick = 1;  // a key whose home slot is not `other`'s
    while (pick < 8 && home_slot(W, rows[pick], m.a.tmask) == home_slot(W, other, m.a.tmask)) pick++;
    const Row& key = rows[pick];
    const uint32_t held = m.find<true>(other.data());
    const uint32_t home = home_slot(W, key, m.a.tmask);
    // every slot names `other`'s entry under a tag that is not `key`'s: tmask + 1 other keys, once the home slot goes
    const uint64_t foreign = ((uint64_t)0xABCDu << 32) | (uint64_t)(held + 1u);
    for (uint32_t s = 0; s <= m.a.tmask; s++)
        if (s != home && m.table[s] == 0) m.table[s] = foreign;
    CHECK(m.table[home] == 0);
    bool ran = false;
    CHECK(m.find<true>(key.data(), [&] { m.table[home] = foreign, ran = true; }) == REACH_NONE);
    CHECK(ran && m.ctl[REACH_OVERFLOW] == 1 && m.ctl[REACH_COUNT] == 1);
    CHECK(m.ctl[REACH_KEYS] == 2 && m.ctl[REACH_FREE_TAIL] == 1);  // one entry taken, dropped once
    const uint32_t e = m.free_ring[0];
    CHECK(e != held && m.mark[e] == REACH_DEAD && m.mark[held] == 0);
    CHECK(m.find<false>(key.data()) == REACH_NONE && m.find<false>(other.data()) == held);
    CHECK(m.find<true>(key.data()) == REACH_NONE && m.ctl[REACH_FREE_TAIL] == 1);  // no empty slot: no entry taken
}

int main() {
    CHECK(keytable_pow2(0) == 64 && keytable_pow2(64) == 64 && keytable_pow2(65) == 128);
    CHECK(keytable_pow2(1ull << 25) == 1u << 25 && keytable_pow2((1ull << 25) + 1) == 1u << 26);
    CHECK(keytable_pow2(1ull << 31) == 1u << 31);
    for (int W : {1, 2, 5, 8}) {
        check_inserts(W, false);
        check_inserts(W, true);
        check_max_states(W);
        check_key_cap(W);
        check_full_table(W);
    }
    printf("keytable_check ok\n");
    return 0;
}
