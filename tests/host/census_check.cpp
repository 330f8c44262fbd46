// census_check.cpp -- the state census' host part (csrc/pbn_census.hpp) on the CPU, under ASan + UBSan
// (`make censuscheck`).
//
// No HIP, no GPU, no library: the header alone. Table sizing, the sample-point rule the kernel walks against a
// restatement with a modulus, the sequential model of the device table's slot / entry layout against a std::map over
// every word count -- exact counts, overflow accounting, entries lost to a publish race and handed out again by a later
// launch -- and the read-out's compaction.
#include "pbn_census.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>

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

// few distinct values per word: rows share words and differ in one of them
static Row random_row(int W, uint64_t variety) {
    Row r(W);
    for (int k = 0; k < W; k++) r[k] = rnd() % 3 ? rnd() % variety : 0x8000000000000000ull | (rnd() % variety);
    return r;
}

static void check_sizing() {
    CHECK(census_slots(1) == 64 && census_slots(32) == 64 && census_slots(33) == 128);
    CHECK(census_slots(1ull << 22) == 1u << 23 && census_slots(CENSUS_MAX_STATES) == 1u << 25);
    for (uint64_t m : {1ull, 2ull, 31ull, 32ull, 33ull, 100ull, 4096ull, 4097ull, 1ull << 24}) {
        const uint32_t s = census_slots(m);
        CHECK((s & (s - 1)) == 0 && s >= 64 && s >= 2 * m && (s == 64 || s / 2 < 2 * m));
        const uint32_t kc = census_key_cap(m);
        CHECK(kc == m + CENSUS_SLACK && CENSUS_SLACK >= (uint32_t)CENSUS_MAX_GRID * BLOCK);  // a spare per lane
        const uint32_t r = census_ring_cap(kc);
        CHECK((r & (r - 1)) == 0 && r >= kc && r / 2 < kc);
    }
}

// The kernel's walk (CensusSampler::hit(i) for i = 0 .. n_updates) against "i >= first and (i - first) % stride == 0".
static void check_sample_rule() {
    const uint32_t ns[] = {0, 1, 2, 7, 33, 64, 1000};
    const uint32_t strides[] = {1, 2, 3, 4, 33, 34, 1000, 1001, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t n : ns)
        for (uint32_t stride : strides)
            for (uint32_t first = 0; first <= n; first = first < 40 ? first + 1 : first + 97) {
                CensusSampler s{first, stride};
                uint64_t hits = 0;
                for (uint32_t i = 0; i <= n; i++) {
                    const bool want = i >= first && (i - first) % stride == 0;
                    CHECK(s.hit(i) == want);
                    hits += want;
                }
                CHECK(hits == census_samples(n, first, stride));
                CHECK(hits >= 1);
            }
    CHECK(census_samples(33, 0, 1) == 34 && census_samples(33, 3, 4) == 8 && census_samples(33, 33, 1) == 1);
    CHECK(census_samples(0, 0, 1) == 1 && census_samples(5, 6, 1) == 0 && census_samples(5, 0, 0) == 0);
    CHECK(census_samples(65536, 0, 1) == 65537 && census_samples(65536, 0, 0xFFFFFFFFu) == 1);
}

// The reported states and counts; *dropped: the model's dropped visits plus those of entries past max_states.
static std::map<Row, uint64_t> read_out(const CensusModel& m, uint64_t* dropped = nullptr) {
    const uint64_t ne = m.n_entries();
    std::vector<uint64_t> states((size_t)ne * m.W + 1), counts(ne + 1);
    uint64_t over = 0;
    const uint64_t n = census_compact(m.keys.data(), m.counts.data(), ne, m.W, states.data(), counts.data(), ne, &over);
    CHECK(n <= ne);
    CHECK(n == (m.ctl[CENSUS_COUNT] < m.max_states ? m.ctl[CENSUS_COUNT] : m.max_states));  // the first max_states ranks
    CHECK((over > 0) == (m.ctl[CENSUS_COUNT] > m.max_states));
    if (dropped) *dropped = m.dropped + over;
    std::map<Row, uint64_t> out;
    for (uint64_t r = 0; r < n; r++) {
        Row row(states.begin() + r * m.W, states.begin() + (r + 1) * m.W);
        CHECK(!out.count(row));  // a state is held once
        CHECK(counts[r] > 0);
        out[row] = counts[r];
    }
    return out;
}

// Visits of `distinct`-ish states in runs (the kernel's pending runs add n > 1 at once), a race loser every `lose`
// inserts, a new launch every `launch` visits.
static void check_model(int W, uint64_t max_states, uint64_t variety, int n_visits, int lose, int launch) {
    const uint32_t slack = 8;  // small, so that dead entries can use the key array up as well
    CensusModel m;
    m.init(W, max_states, slack);
    CHECK(m.tmask + 1 == census_slots(max_states) && m.key_cap == max_states + slack);
    std::map<Row, uint64_t> ref;
    uint64_t visits = 0;
    for (int v = 0; v < n_visits; v++) {
        if (launch && v % launch == launch - 1) m.next_launch();
        if (lose && v % lose == lose - 1) m.lose_next_publish();
        const Row r = random_row(W, variety);
        const uint64_t n = rnd() % 5 == 0 ? 1 + rnd() % 70000 : 1;  // runs past 2^16, sums past 2^32 below
        m.visit(r.data(), n);
        ref[r] += n;
        visits += n;
    }
    uint64_t dropped = 0;
    const auto got = read_out(m, &dropped);
    uint64_t sum = 0;
    for (auto& kv : got) sum += kv.second;
    CHECK(m.visits == visits);
    CHECK(got.size() <= max_states);                         // (a)
    CHECK(sum + dropped == visits);                          // (b)
    for (auto& kv : got) {
        auto it = ref.find(kv.first);
        CHECK(it != ref.end());
        CHECK(dropped == 0 ? kv.second == it->second : kv.second <= it->second);  // (c), (d)
        // a state is dropped on the device only once no entry is left, and is never inserted after that in this
        // sequential model (entries do not come back within a launch): short of that its count is exact
        if (m.dropped == 0) CHECK(kv.second == it->second);
    }
    if (dropped == 0) CHECK(got.size() == ref.size());
    if (ref.size() > max_states) CHECK(dropped > 0 && (lose || got.size() == max_states));
    if (ref.size() <= max_states && ref.size() + (lose ? n_visits / lose : 0) <= m.key_cap) CHECK(dropped == 0);
    // every dead entry is on a ring: reserved = live + ring contents
    const uint32_t on_rings = (m.ctl[CENSUS_TAIL0] - m.ctl[CENSUS_HEAD0]) + (m.ctl[CENSUS_TAIL1] - m.ctl[CENSUS_HEAD1]);
    CHECK(m.n_entries() == m.ctl[CENSUS_COUNT] + on_rings);
}

// Dead entries go back into use: with a loser before every insert and a new launch per visit, S distinct states take
// S + 1 entries, not 2 S: each launch's loser is handed the entry the last launch's loser left on the ring.
static void check_dead_entries_are_reused(int W) {
    const uint64_t S = 40;
    CensusModel m;
    m.init(W, S, 1);
    std::map<Row, uint64_t> ref;
    while (ref.size() < S) {
        const Row r = random_row(W, 1ull << 40);
        if (ref.count(r)) continue;
        m.next_launch();
        m.lose_next_publish();
        m.visit(r.data(), 3);
        ref[r] = 3;
    }
    CHECK(m.dropped == 0 && m.ctl[CENSUS_COUNT] == S && m.n_entries() == S + 1);
    CHECK(read_out(m) == ref);
    // compaction skips the dead entry in the middle of the array and keeps entry order
    std::vector<uint64_t> keys = {10, 11, 12, 13}, counts = {5, 0, 7, 0}, s(4), c(4);
    CHECK(census_compact(keys.data(), counts.data(), 4, 1, s.data(), c.data(), 4) == 2);
    CHECK(s[0] == 10 && s[1] == 12 && c[0] == 5 && c[1] == 7);
    // a short capacity: the count is still returned, nothing is written past it
    s.assign(4, 99);
    CHECK(census_compact(keys.data(), counts.data(), 4, 1, s.data(), nullptr, 1) == 2 && s[0] == 10 && s[1] == 99);
    CHECK(census_compact(keys.data(), counts.data(), 0, 1, nullptr, nullptr, 0) == 0);
}

// The spare hand-off of census_find, lane by lane: L lanes race for one key, all but the winner are left with an entry
// taken in vain; then every lane hits keys that are already held (walks that meet no empty slot: the spare must
// survive them), then inserts a key of its own (from the spare, no new entry), loses one more race and ends. Entries
// taken from the end of keys stay within live + L, and the next launch's inserts come off the ring.
static void check_spares(int W) {
    const uint32_t L = 50;
    CensusModel m;
    m.init(W, 4096, L);
    std::map<Row, uint64_t> ref;
    std::vector<uint32_t> spare(L, CENSUS_NONE);
    const Row k0 = random_row(W, 1ull << 40), k1 = random_row(W, 1ull << 40);
    m.visit(k0.data(), 1, &spare[0]);  // the winner
    m.visit(k1.data(), 1, &spare[0]);
    ref[k0] += 1;
    ref[k1] += 1;
    CHECK(spare[0] == CENSUS_NONE && m.n_entries() == 2);
    for (uint32_t l = 1; l < L; l++) {
        m.lose_race(&spare[l]);
        CHECK(spare[l] != CENSUS_NONE);
    }
    CHECK(m.n_entries() == 2 + (L - 1));
    for (uint32_t l = 1; l < L; l++) {
        const uint32_t held = spare[l];
        m.visit(k0.data(), 2, &spare[l]);  // direct hits: no empty slot on the walk
        m.visit(k1.data(), 3, &spare[l]);
        ref[k0] += 2;
        ref[k1] += 3;
        CHECK(spare[l] == held);  // the spare survives a walk that takes no entry
    }
    CHECK(m.n_entries() == 2 + (L - 1));
    // the rival path of find itself: lane 1 and another lane reach the empty slot of a new key, the other publishes
    const Row k2 = random_row(W, 1ull << 40);
    {
        const uint32_t held = spare[1];
        m.visit(k2.data(), 5, &spare[1], true);
        ref[k2] += 5;
        CHECK(spare[1] == held);  // used for the attempt, back after the loss
        CHECK(m.n_entries() == 2 + (L - 1) + 1);  // the rival's entry
    }
    for (uint32_t l = 1; l < L; l++) {
        Row own = random_row(W, 1ull << 40);
        while (ref.count(own)) own = random_row(W, 1ull << 40);
        const uint32_t held = spare[l];
        m.visit(own.data(), 7, &spare[l]);
        ref[own] += 7;
        CHECK(spare[l] == CENSUS_NONE);  // the insert used the spare ...
        CHECK(m.counts[held] == 7);      // ... and no entry of the key array
    }
    CHECK(m.n_entries() == 3 + (L - 1));
    for (uint32_t l = 1; l < L; l++) m.lose_race(&spare[l]);
    const uint32_t taken = m.n_entries();
    CHECK(taken == 3 + 2 * (L - 1) && taken <= m.ctl[CENSUS_COUNT] + L);  // live + one dead entry per lane at most
    for (uint32_t l = 0; l < L; l++) m.end_lane(&spare[l]);
    CHECK(m.ctl[CENSUS_TAIL0 + m.parity] - m.ctl[CENSUS_HEAD0 + m.parity] == L - 1);
    // the next launch: L - 1 new keys come off the ring, the key array does not grow
    m.next_launch();
    for (uint32_t l = 1; l < L; l++) {
        Row own = random_row(W, 1ull << 40);
        while (ref.count(own)) own = random_row(W, 1ull << 40);
        m.visit(own.data(), 1, &spare[l]);
        ref[own] += 1;
    }
    CHECK(m.n_entries() == taken && m.dropped == 0);
    CHECK(m.ctl[CENSUS_TAIL0 + (m.parity ^ 1u)] == m.ctl[CENSUS_HEAD0 + (m.parity ^ 1u)]);  // the ring is used up
    CHECK(read_out(m) == ref);
}

// A full table, every slot another key: the walk ends after `slots` probes, the visit is dropped.
static void check_full_table_terminates() {
    CensusModel m;
    m.init(1, 64, 4);
    for (uint32_t k = 0; k <= m.tmask; k++) m.table[k] = ((uint64_t)0xABCDu << 32) | 1u;  // all name entry 0, key 0
    m.keys[0] = 0xFFFF;
    const uint64_t key = 5;
    m.visit(&key);
    CHECK(m.dropped == 1 && m.ctl[CENSUS_COUNT] == 0);
}

int main() {
    check_sizing();
    check_sample_rule();
    for (int W = 1; W <= 8; W++) {
        check_model(W, 4096, 40, 3000, 0, 0);        // far below capacity: exact
        check_model(W, 4096, 40, 3000, 7, 50);       // with race losers and launches
        check_model(W, 16, 4, 2000, 0, 0);           // overflow: more distinct states than entries
        check_model(W, 16, 4, 2000, 5, 40);          // overflow with dead entries eating capacity
        check_model(W, 1, 2, 300, 3, 10);            // one entry
        check_model(W, 33, 3, 2000, 11, 100);        // either side of a table doubling
        check_dead_entries_are_reused(W);
        check_spares(W);
    }
    check_full_table_terminates();
    printf("census_check ok\n");
    return 0;
}
