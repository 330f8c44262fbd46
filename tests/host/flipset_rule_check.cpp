// flipset_rule_check.cpp -- the max over multi-flip action sets (csrc/pbn_flipset_rule.hpp) on the CPU.
//
// Built by `make flipsetrulecheck` with ASan + UBSan; no HIP header, no library, no GPU.
//  1. The rule: on cubes of 1 .. 6 nodes with a restricted set of allowed nodes, worths with many ties (small integers)
//     and without (random doubles), k in {0, 0.5, 1} and A in 1 .. 5, the level recursion -- made the way the kernels
//     make it: lane j of a group of G folds nodes j, j + G, ..., then the xor butterfly with flip_merge -- against the
//     enumeration of every set of 1 .. A allowed nodes: the whole summary T_A (both entries, flip counts and end rows
//     included), that every lane of the group ends with the same pair, and the chosen action.
//  2. The kernels' walk under pbn_control_plan.hpp, replayed lane by lane on arrays of the real sizes (std::vectors of
//     exactly that size, read through .at(): ASan and the range check watch them): every index into nbr ([S][N]), m ([S])
//     and the summaries ([S][2]) is in range, every row is written exactly once, and a row past the end writes nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pbn_control_plan.hpp"
#include "pbn_flipset_rule.hpp"

using namespace pbn;

#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            std::fprintf(stderr, "flipset_rule_check: %s failed at line %d\n", #cond, __LINE__); \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bool same(const FlipEntry& a, const FlipEntry& b) {
    if (!flip_is(a) || !flip_is(b)) return flip_is(a) == flip_is(b);
    return a.tag == b.tag && std::memcmp(&a.base, &b.base, 8) == 0;
}

// the order, restated on plain numbers
struct Plain {
    double value;
    int d, y;
    double base;
};
static bool plain_better(const Plain& a, const Plain& b) {
    if (a.value != b.value) return a.value > b.value;
    if (a.d != b.d) return a.d < b.d;
    return a.y < b.y;
}

// One level the way the kernels make it: per row, G lanes, lane j starts from the row's own pair and folds the nodes
// j, j + G, ...; then the butterfly. Every lane must end with the same pair.
static void level(uint32_t n, const std::vector<int32_t>& nbr, double k, const std::vector<FlipPair>& in,
                  std::vector<FlipPair>& out) {
    const uint32_t S = 1u << n, G = control_group(n);
    for (uint32_t s = 0; s < S; ++s) {
        std::vector<FlipPair> lane(G);
        for (uint32_t j = 0; j < G; ++j) {
            FlipPair p = in[s];
            for (uint32_t i = j; i < n; i += G) {
                const int32_t t = nbr.at(s * n + i);
                if (t < 0) continue;
                const FlipPair f{flip_bump(in.at(t).e0), flip_bump(in.at(t).e1)};
                p = flip_merge(p, f, k);
            }
            lane[j] = p;
        }
        for (uint32_t d = G / 2; d >= 1; d >>= 1) {
            std::vector<FlipPair> next(G);
            for (uint32_t j = 0; j < G; ++j) next[j] = flip_merge(lane[j], lane[j ^ d], k);
            lane = next;
        }
        for (uint32_t j = 1; j < G; ++j) REQUIRE(same(lane[j].e0, lane[0].e0) && same(lane[j].e1, lane[0].e1));
        out[s] = lane[0];
    }
}

static void check_cube(uint32_t n, uint32_t allowed, int A, double k, bool ties) {
    const uint32_t S = 1u << n;
    std::vector<double> m(S);
    for (auto& v : m) v = ties ? (double)(rnd() % 4) : (double)(rnd() >> 11) * 0x1p-53 * 8.0 - 4.0;
    std::vector<int32_t> nbr(S * n);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t i = 0; i < n; ++i) nbr[s * n + i] = (allowed >> i) & 1u ? (int32_t)(s ^ (1u << i)) : -1;
    std::vector<FlipPair> a(S), b(S);
    for (uint32_t s = 0; s < S; ++s) a[s] = FlipPair{flip_entry((int32_t)s, 0, m[s]), flip_none()};
    for (int lev = 0; lev < A; ++lev) {
        level(n, nbr, k, a, b);
        a.swap(b);
    }
    for (uint32_t s = 0; s < S; ++s) {
        // enumeration: every subset F of the allowed nodes with |F| <= A, the empty set included for the summary
        std::vector<Plain> all;
        for (uint32_t F = 0; F < S; ++F) {
            const int d = __builtin_popcount(F);
            if ((F & ~allowed) || d > A) continue;
            const int y = (int)(s ^ F);
            const double c = k * (double)d;
            all.push_back(Plain{m[y] - c, d, y, m[y]});
        }
        std::sort(all.begin(), all.end(), plain_better);  // distinct F: distinct ends, so the best two are all[0], all[1]
        REQUIRE(flip_is(a[s].e0) && flip_end(a[s].e0) == all[0].y && flip_count(a[s].e0) == all[0].d);
        REQUIRE(std::memcmp(&a[s].e0.base, &all[0].base, 8) == 0);
        if (all.size() > 1) {
            REQUIRE(flip_is(a[s].e1) && flip_end(a[s].e1) == all[1].y && flip_count(a[s].e1) == all[1].d);
            const double v1 = flip_value(a[s].e1, k);
            REQUIRE(std::memcmp(&v1, &all[1].value, 8) == 0);
        } else {
            REQUIRE(!flip_is(a[s].e1));
        }
        // the action: the best non-empty set
        const FlipEntry act = flip_action(a[s], (int32_t)s);
        const Plain* want = nullptr;
        for (const Plain& p : all)
            if (p.d > 0) {
                want = &p;
                break;
            }
        REQUIRE(flip_is(act) == (want != nullptr));
        if (want) {
            const double v = flip_value(act, k);
            REQUIRE(flip_end(act) == want->y && flip_count(act) == want->d && std::memcmp(&v, &want->value, 8) == 0);
            REQUIRE(flip_end(act) != (int32_t)s && flip_count(act) >= 1 && flip_count(act) <= A);
        }
    }
}

// The kernels' walk: workgroup b, thread t -> lane j = t % G of the group of row r = t / G; per trip the rows base + q *
// RPB + r, q < rows_unrolled. The one-cell kernel clamps a row past the end to S - 1 and a lane past N to cell 0 and
// reads there; the looping kernel reads nothing for such a row. A cell that is no row (-1, or >= S) gathers nothing
// (looping) or the row's own pair (one-cell). Lane 0 of a live row writes the row's two entries.
static void walk(uint64_t S, uint32_t N, int n_cu, int bpc, int cap, bool level0) {
    const ControlPlan p = control_plan(S, N, n_cu, bpc, cap);
    std::vector<int32_t> nbr(S * N);
    for (uint64_t c = 0; c < S * N; ++c) nbr[c] = (int32_t)((c * 2654435761ull) % (S + 1)) - (c % 5 == 0);  // -1 and S: no row
    std::vector<uint8_t> m(S, 0), in_base(2 * S, 0), in_tag(2 * S, 0), out_base(2 * S, 0), out_tag(2 * S, 0), cells(S * N, 0);
    auto gather = [&](uint64_t t) {
        if (level0) {
            m.at(t) |= 1;
        } else {
            in_base.at(2 * t) |= 1, in_base.at(2 * t + 1) |= 1;
            in_tag.at(2 * t) |= 1, in_tag.at(2 * t + 1) |= 1;
        }
    };
    const uint64_t per_trip = (uint64_t)p.rows_per_block * p.rows_unrolled;
    const bool one_cell = p.cells_per_lane == 1;
    for (int b = 0; b < p.grid; ++b)
        for (uint64_t base = (uint64_t)b * per_trip; base < S; base += (uint64_t)p.grid * per_trip)
            for (uint32_t qr = 0; qr < per_trip; ++qr) {
                const uint64_t want = base + qr;
                const bool live = want < S;
                if (!live && !one_cell) continue;  // the lanes stay for the shuffles with empty pairs
                const uint64_t row = live ? want : S - 1;
                for (uint32_t j = 0; j < p.G; ++j) {
                    gather(row);  // the row's own pair
                    for (uint64_t i = one_cell ? (j < N ? j : 0) : j; i < N; i += p.G) {
                        cells.at(row * N + i) += live && (!one_cell || j < N);
                        const uint64_t t = (uint64_t)(uint32_t)nbr.at(row * N + i);
                        if (t < S)
                            gather(t);
                        else if (one_cell)
                            gather(row);
                        if (one_cell) break;
                    }
                }
                if (live) {
                    out_base.at(2 * row)++, out_base.at(2 * row + 1)++;
                    out_tag.at(2 * row)++, out_tag.at(2 * row + 1)++;
                }
            }
    for (uint64_t s = 0; s < S; ++s) {
        REQUIRE(out_base[2 * s] == 1 && out_base[2 * s + 1] == 1 && out_tag[2 * s] == 1 && out_tag[2 * s + 1] == 1);
        for (uint32_t i = 0; i < N; ++i) REQUIRE(cells[s * N + i] == 1);
    }
}

int main() {
    // the tag: the largest row and flip count fit, and stay apart from "none"
    {
        const FlipEntry e = flip_entry((1 << 24) - 1, FLIPSET_MAX_FLIPS, 1.5);
        REQUIRE(flip_is(e) && flip_end(e) == (1 << 24) - 1 && flip_count(e) == FLIPSET_MAX_FLIPS);
        REQUIRE(!flip_is(flip_none()) && !flip_is(flip_bump(flip_none())));
        const FlipEntry f = flip_bump(flip_entry(7, 3, 2.0));
        REQUIRE(flip_end(f) == 7 && flip_count(f) == 4 && flip_value(f, 0.5) == 0.0);
        REQUIRE(flip_better(e, flip_none(), 1.0) && !flip_better(flip_none(), e, 1.0) && !flip_better(flip_none(), flip_none(), 1.0));
        // by hand: the walk i, i returns to s at cost 2k and beats every action; the action is still a real flip
        FlipPair p{flip_entry(0, 0, 10.0), flip_none()};
        flip_insert(p, flip_entry(0, 2, 10.0), 1.0);  // the cancelled walk: the same end, worse
        flip_insert(p, flip_entry(1, 1, 3.0), 1.0);
        flip_insert(p, flip_entry(2, 1, 5.0), 1.0);
        flip_insert(p, flip_entry(1, 3, 3.0), 1.0);
        REQUIRE(flip_end(p.e0) == 0 && flip_count(p.e0) == 0 && flip_end(p.e1) == 2);
        const FlipEntry act = flip_action(p, 0);
        REQUIRE(flip_end(act) == 2 && flip_count(act) == 1 && flip_value(act, 1.0) == 4.0);
    }
    const double costs[] = {0.0, 0.5, 1.0};
    int cubes = 0;
    for (uint32_t n = 1; n <= 6; ++n)
        for (int rep = 0; rep < 6; ++rep) {
            const uint32_t full = (1u << n) - 1u;
            const uint32_t allowed = rep == 0 ? full : rep == 1 ? full & ~1u : (uint32_t)rnd() & full;
            for (int A = 1; A <= 5; ++A)
                for (double k : costs)
                    for (bool ties : {true, false}) {
                        check_cube(n, allowed, A, k, ties);
                        ++cubes;
                    }
        }
    const uint32_t nodes[] = {1, 2, 3, 6, 8, 10, 16, 21, 33, 64, 65, 100, 257};
    for (uint32_t N : nodes) {
        const uint32_t G = control_group(N);
        const uint32_t per = CONTROL_BLOCK / G * (N <= G ? CONTROL_UNROLL : 1);
        const uint64_t sizes[] = {1, 2, per - 1 ? per - 1 : 1, per, per + 1, 2 * per + 3, 5 * per + 1};
        for (uint64_t S : sizes)
            for (bool level0 : {true, false}) {
                walk(S, N, 256, 8, 0, level0);
                walk(S, N, 256, 8, 3, level0);
                walk(S, N, 1, 1, 0, level0);
            }
    }
    std::printf("flipset_rule_check ok (%d cubes)\n", cubes);
    return 0;
}
