// stateset_hull_check.cpp -- the state set's hull words, largest label and the hull pre-filter (csrc/pbn_stateset.hpp)
// on the CPU, under ASan + UBSan (`make statesethullcheck`).
//
// No HIP, no GPU, no library: the header alone. stateset_build's hull_all / hull_any are checked against an AND / OR
// loop over the distinct rows for every word count; stateset_hull_rejects (what k_env_set runs before it probes the
// table) must never reject a member, must reject a member with one agreed node flipped, and must pass every state
// when handed the words that switch the filter off.
#include "pbn_stateset.hpp"

#include <cstdio>
#include <cstdlib>

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

static uint64_t top_mask(int N) { return N % 64 ? (1ull << (N % 64)) - 1 : ~0ull; }

template <int W>
static void check(int N, uint64_t S, int free_bits) {
    // members: one base state with `free_bits` random nodes varying, so that the hull has agreed and free nodes
    std::vector<uint64_t> base(W), vary(W, 0);
    for (int k = 0; k < W; k++) base[k] = rnd() & (k == W - 1 ? top_mask(N) : ~0ull);
    for (int f = 0; f < free_bits; f++) {
        const int i = (int)(rnd() % (uint64_t)N);
        vary[i / 64] |= 1ull << (i % 64);
    }
    std::vector<uint64_t> flat;
    std::vector<int32_t> labels;
    int32_t top = -1;
    for (uint64_t r = 0; r < S; r++) {
        for (int k = 0; k < W; k++) flat.push_back(base[k] ^ (rnd() & vary[k]));
        labels.push_back((int32_t)(rnd() % 9));
        // a repeated row keeps its first label (a second label would be a conflict)
        for (uint64_t q = 0; q < r; q++) {
            bool same = true;
            for (int k = 0; k < W; k++) same = same && flat[q * W + k] == flat[r * W + k];
            if (same) labels[r] = labels[q];
        }
        top = labels[r] > top ? labels[r] : top;
    }
    StateSetTable t;
    CHECK(stateset_build(N, flat.data(), labels.data(), S, &t) == STATESET_OK);
    CHECK((int)t.hull_all.size() == W && (int)t.hull_any.size() == W);
    CHECK(t.max_label == top);
    uint64_t all[W], any[W], off_all[W], off_any[W];
    for (int k = 0; k < W; k++) {
        all[k] = k == W - 1 ? top_mask(N) : ~0ull;
        any[k] = 0;
        off_all[k] = ~0ull;
        off_any[k] = 0;
    }
    for (uint64_t r = 0; r < S; r++)
        for (int k = 0; k < W; k++) {
            all[k] &= flat[r * W + k];
            any[k] |= flat[r * W + k];
        }
    for (int k = 0; k < W; k++) CHECK(t.hull_all[k] == all[k] && t.hull_any[k] == any[k]);
    for (uint64_t r = 0; r < S; r++) {
        uint64_t s[W];
        for (int k = 0; k < W; k++) s[k] = flat[r * W + k];
        CHECK(!stateset_hull_rejects<W>(s, all, any));  // never a member
        CHECK(stateset_lookup<W>(s, t.meta.data(), t.keys.data(), t.slots) == labels[r]);
        // one node flipped: rejected iff every member agrees on it; what passes is still looked up exactly
        const int i = (int)(rnd() % (uint64_t)N);
        s[i / 64] ^= 1ull << (i % 64);
        const bool agreed = !(((all[i / 64] ^ any[i / 64]) >> (i % 64)) & 1ull);
        CHECK(stateset_hull_rejects<W>(s, all, any) == agreed);
        if (agreed) CHECK(stateset_lookup<W>(s, t.meta.data(), t.keys.data(), t.slots) == -1);
        CHECK(!stateset_hull_rejects<W>(s, off_all, off_any));  // the filter switched off passes everything
    }
}

int main() {
    const uint64_t sizes[] = {1, 2, 33, 700};
    const int frees[] = {0, 1, 5, 40};
    for (uint64_t S : sizes)
        for (int f : frees) {
            check<1>(1, S, 0);
            check<1>(18, S, f);
            check<1>(64, S, f);
            check<2>(65, S, f);
            check<3>(192, S, f);
            check<4>(200, S, f);
            check<5>(257, S, f);
            check<6>(384, S, f);
            check<7>(448, S, f);
            check<8>(512, S, f);
        }
    // the empty set: AND = the N-bit mask, OR = 0, no label
    StateSetTable e;
    CHECK(stateset_build(200, nullptr, nullptr, 0, &e) == STATESET_OK);
    CHECK(e.max_label == -1 && e.hull_all[3] == top_mask(200) && e.hull_all[0] == ~0ull && e.hull_any[2] == 0);
    printf("stateset_hull_check ok\n");
    return 0;
}
