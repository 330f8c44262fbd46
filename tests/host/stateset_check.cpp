// stateset_check.cpp -- the exact state set (csrc/pbn_stateset.hpp) on the CPU, under ASan + UBSan
// (`make statesetcheck`).
//
// No HIP, no GPU, no library: the header alone. The builder and the walk the kernels run are checked against a
// std::map over every word count, the set sizes either side of a table doubling, members that differ in one bit or
// in the last word only, the duplicate rules, the stray-bit refusal, and walks that wrap past the table's end.
#include "pbn_stateset.hpp"

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

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

using Row = std::vector<uint64_t>;

static uint64_t top_mask(int N) { return N % 64 ? (1ull << (N % 64)) - 1 : ~0ull; }

static Row random_row(int N) {
    const int W = (N + 63) / 64;
    Row r(W);
    // few distinct values per word, so that rows share words and differ in one of them
    for (int k = 0; k < W; k++) r[k] = (rnd() % 4 ? rnd() : rnd() % 3) & (k == W - 1 ? top_mask(N) : ~0ull);
    return r;
}

static int32_t lookup1(const StateSetTable& t, const Row& r) {
    int32_t out = -2;
    stateset_lookup_host(t, r.data(), 1, &out);
    return out;
}

// The hash restated without the template (the kernels and the host share the header's; this one is the issue's text).
static uint64_t hash_restated(const Row& r) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint64_t w : r) {
        h = (h ^ w) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 29;
    return h;
}

static void check_sizes(int N, uint64_t S) {
    const int W = (N + 63) / 64;
    std::map<Row, int32_t> ref;
    std::vector<uint64_t> flat;
    std::vector<int32_t> labels;
    while (ref.size() < S) {
        Row r = random_row(N);
        if (ref.count(r)) continue;
        const int32_t label = (int32_t)(rnd() % 7 == 0 ? 0x7FFFFFFF - rnd() % 3 : rnd() % 1000);
        ref[r] = label;
        flat.insert(flat.end(), r.begin(), r.end());
        labels.push_back(label);
    }
    StateSetTable t;
    CHECK(stateset_build(N, flat.data(), labels.data(), S, &t) == STATESET_OK);
    CHECK(t.W == W && t.n_states == S);
    uint32_t want_slots = 64;
    while (want_slots < 2 * S) want_slots *= 2;
    CHECK(t.slots == want_slots);
    CHECK(S == 0 ? t.max_probe == 0 : t.max_probe >= 1);
    // every member with its label, its longest walk bounded by max_probe
    uint32_t longest = 0;
    for (auto& kv : ref) {
        CHECK(lookup1(t, kv.first) == kv.second);
        uint32_t probes = 0;
        stateset_by_words(W, [&](auto w) {
            constexpr int WW = decltype(w)::value;
            uint64_t s[WW];
            for (int k = 0; k < WW; ++k) s[k] = kv.first[k];
            CHECK(stateset_lookup<WW>(s, t.meta.data(), t.keys.data(), t.slots, &probes) == kv.second);
            CHECK(((uint32_t)stateset_hash<WW>(s)) == (uint32_t)hash_restated(kv.first));
            return 0;
        });
        longest = probes > longest ? probes : longest;
    }
    CHECK(longest == t.max_probe);
    // non-members: random rows, members with one bit flipped, members differing only in the last word
    for (int q = 0; q < 2000; q++) {
        Row r = random_row(N);
        auto it = ref.find(r);
        CHECK(lookup1(t, r) == (it == ref.end() ? -1 : it->second));
    }
    int n = 0;
    for (auto& kv : ref) {
        if (++n > 200) break;
        Row r = kv.first;
        const int bit = (int)(rnd() % (uint64_t)N);
        r[bit / 64] ^= 1ull << (bit % 64);
        auto it = ref.find(r);
        CHECK(lookup1(t, r) == (it == ref.end() ? -1 : it->second));
        r = kv.first;
        r[W - 1] ^= 1ull << (rnd() % (uint64_t)(N - 64 * (W - 1)));
        it = ref.find(r);
        CHECK(lookup1(t, r) == (it == ref.end() ? -1 : it->second));
        // a query with a stray bit is no member
        if (N % 64) {
            r = kv.first;
            r[W - 1] |= 1ull << (N % 64);
            CHECK(lookup1(t, r) == -1);
        }
    }
    // the layout is a function of the input: a second build is identical
    StateSetTable t2;
    CHECK(stateset_build(N, flat.data(), labels.data(), S, &t2) == STATESET_OK);
    CHECK(t2.meta == t.meta && t2.keys == t.keys && t2.max_probe == t.max_probe);
    // NULL labels: all 0
    StateSetTable t0;
    CHECK(stateset_build(N, flat.data(), nullptr, S, &t0) == STATESET_OK);
    for (auto& kv : ref) CHECK(lookup1(t0, kv.first) == 0);
}

static void check_duplicates_and_refusals(int N) {
    const int W = (N + 63) / 64;
    Row a = random_row(N), b = random_row(N);
    while (b == a) b = random_row(N);
    std::vector<uint64_t> flat;
    for (const Row* r : {&a, &b, &a}) flat.insert(flat.end(), r->begin(), r->end());
    StateSetTable t;
    uint64_t bad = 99;
    int32_t same[] = {5, 6, 5};
    CHECK(stateset_build(N, flat.data(), same, 3, &t, &bad) == STATESET_OK);
    CHECK(t.n_states == 2 && lookup1(t, a) == 5 && lookup1(t, b) == 6);
    int32_t differ[] = {5, 6, 7};
    CHECK(stateset_build(N, flat.data(), differ, 3, &t, &bad) == STATESET_E_CONFLICT && bad == 2);
    int32_t negative[] = {5, -1, 5};
    CHECK(stateset_build(N, flat.data(), negative, 3, &t, &bad) == STATESET_E_LABEL && bad == 1);
    if (N % 64) {
        flat[(size_t)1 * W + W - 1] |= 1ull << (N % 64);
        CHECK(stateset_build(N, flat.data(), same, 3, &t, &bad) == STATESET_E_STRAY_BITS && bad == 1);
        flat[(size_t)1 * W + W - 1] = ~0ull;
        CHECK(stateset_build(N, flat.data(), same, 3, &t, &bad) == STATESET_E_STRAY_BITS && bad == 1);
    }
    CHECK(stateset_build(0, flat.data(), same, 3, &t) == STATESET_E_SHAPE);
    CHECK(stateset_build(64 * 8 + 1, flat.data(), same, 3, &t) == STATESET_E_SHAPE);
    CHECK(stateset_build(N, flat.data(), same, STATESET_MAX_STATES + 1, &t) == STATESET_E_SHAPE);
}

// 12 states whose home is the last slot of a 64-slot table: the walks wrap past the end, the last one 12 long.
static void check_wrapped_walks(int N) {
    const int W = (N + 63) / 64;
    std::vector<Row> rows;
    for (uint64_t v = 0; rows.size() < 12; v++) {
        Row r(W, 0);
        r[0] = v;
        if (W > 1) r[W - 1] = (v * 0x9E3779B97F4A7C15ull) & top_mask(N);
        if (((uint32_t)hash_restated(r) & 63u) == 63u) rows.push_back(r);
    }
    std::vector<uint64_t> flat;
    std::vector<int32_t> labels;
    for (size_t k = 0; k < rows.size(); k++) {
        flat.insert(flat.end(), rows[k].begin(), rows[k].end());
        labels.push_back((int32_t)(100 + k));
    }
    StateSetTable t;
    CHECK(stateset_build(N, flat.data(), labels.data(), 12, &t) == STATESET_OK);
    CHECK(t.slots == 64 && t.n_states == 12 && t.max_probe == 12);
    CHECK(t.meta[63] == 101 && t.meta[0] == 102 && t.meta[10] == 112 && t.meta[11] == 0);
    for (size_t k = 0; k < rows.size(); k++) CHECK(lookup1(t, rows[k]) == (int32_t)(100 + k));
    // a 13th state of the same home walks all 12 and ends at the empty slot behind them
    for (uint64_t v = 1ull << 20;; v++) {
        Row r(W, 0);
        r[0] = v;
        if (((uint32_t)hash_restated(r) & 63u) != 63u) continue;
        CHECK(lookup1(t, r) == -1);
        break;
    }
}

// A full table (never built by stateset_build, whose load stays <= 1/2): the walk still ends after `slots` probes.
static void check_full_table_terminates() {
    std::vector<uint32_t> meta(64, 1u);
    std::vector<uint64_t> keys(64);
    for (uint64_t k = 0; k < 64; k++) keys[k] = 1000 + k;
    uint64_t s[1] = {7};
    uint32_t probes = 0;
    CHECK(stateset_lookup<1>(s, meta.data(), keys.data(), 64, &probes) == -1 && probes == 64);
    s[0] = 1063;
    CHECK(stateset_lookup<1>(s, meta.data(), keys.data(), 64) == 0);
}

int main() {
    const int nodes[] = {1, 18, 64, 65, 128, 200, 256, 257, 449, 512};  // W = 1, 1, 1, 2, 2, 4, 4, 5, 8, 8
    const uint64_t sizes[] = {0, 1, 2, 31, 32, 33, 5000};
    for (int N : nodes)
        for (uint64_t S : sizes) {
            if (N == 1 && S > 2) continue;  // two states in all
            check_sizes(N, S);
        }
    for (int N : {18, 64, 100, 200, 512}) check_duplicates_and_refusals(N);
    for (int N : {40, 64, 128, 200, 512}) check_wrapped_walks(N);
    check_full_table_terminates();
    // the empty set: 64 empty slots, every lookup -1
    StateSetTable e;
    CHECK(stateset_build(200, nullptr, nullptr, 0, &e) == STATESET_OK);
    CHECK(e.slots == 64 && e.n_states == 0 && e.max_probe == 0);
    for (int q = 0; q < 100; q++) CHECK(lookup1(e, random_row(200)) == -1);
    CHECK(stateset_slots(32) == 64 && stateset_slots(33) == 128 && stateset_slots(1ull << 24) == 1u << 25);
    printf("stateset_check ok\n");
    return 0;
}
