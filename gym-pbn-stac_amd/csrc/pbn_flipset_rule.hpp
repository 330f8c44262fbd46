// pbn_flipset_rule.hpp -- the max over multi-flip action sets: the entry a set of flips leads to, the
// total order on entries, and the best two entries with distinct end rows of a list ("top-two-distinct").
//
// In the style of pbn_mass_rule.hpp: no HIP header, PBN_HD functions, one definition for the kernels of pbn_flipset.hip
// and for the host (tests/host/flipset_rule_check.cpp). Nothing here branches on anything but the entries.
//
// The problem. M[y] is the worth of arriving at row y, k >= 0 the cost of one flip. From row s a set F of 1 <= |F| <= A
// distinct allowed nodes leads to the row of s ^ F and is worth M[s ^ F] - k |F|. Enumerating the sets costs
// sum_{j <= A} C(N, j) probes per row; the recursion below costs N * A gathers of a pair.
//
// Entries. An entry is (y, d, base): an end row, a flip count and base = M[y]. Its value is base - k * (double)d, one
// multiply and one subtract, never contracted: the formula `m[y] - cost * len(F)` of the host statement bit for bit.
// Order: larger value first, then fewer flips, then the lower end row. Two entries with the same (y, d) are the same
// entry (base is a function of y), so the order is total on distinct entries and "the better of two" does not depend
// on which side it is asked from.
//
// Derivation. With nbr[x][i] the row of x ^ bit(i) for an allowed i, ball_j(x) = the rows within j allowed flips of
// x, and the ball of radius j is the union of the balls of radius j - 1 of x and of its neighbours. The summary
//     T_0[x] = [(x, 0, M[x]), none]
//     T_j[x] = top-two-distinct( T_{j-1}[x]  u  { (y, d + 1, base) : (y, d, base) in T_{j-1}[nbr[x][i]], i allowed } )
// keeps, per end row, the best entry, and of those the best two. Claim: T_j[x] is the top-two-distinct of
// { (y, dist(x, y), M[y]) : y in ball_j(x) }, dist the number of allowed flips between two rows.
//   * Every candidate is a walk: (y, d) with y reached from x by d flips, d >= dist(x, y). A walk that cancels a flip
//     has a larger d than the shortest one; with k >= 0 its value is not larger and the order prefers fewer flips, so
//     it loses to the shortest walk's entry wherever both are present.
//   * Let e = (y, dist(x, y)) be one of the true best two of ball_j(x). If dist(x, y) < j it lies in ball_{j-1}(x), a
//     subset with the same entries, so it is among that ball's best two: in T_{j-1}[x]. If dist(x, y) = j take the
//     neighbour x' on a shortest path: (y, j - 1) lies in ball_{j-1}(x'). Were two entries (y1, d1), (y2, d2) with
//     other ends better than it there, then (y1, d1 + 1) and (y2, d2 + 1) -- walks from x inside ball_j(x) -- would be
//     better than (y, j) at x, since adding one flip to both sides of a comparison keeps it: e would not be among the
//     best two. So e is in T_{j-1}[x'] and arrives, shifted, in the list of T_j[x]; a member of a union's
//     top-two-distinct is in the top-two-distinct of the list where it attains its value.
// "Adding one flip keeps a comparison" is a statement about real numbers. It holds bit for bit whenever the values
// base - k d are exact (k = 0; integers and halves, as rewards and costs usually are) or no two walks' values are
// within a rounding of each other. Where two real values differ by less than one rounding of the subtraction, the
// recursion may keep the other of the two: its value is then within 2^-52 * (max|M| + k A) of the enumeration's.
//
// Why two. After A levels T_A[s] ranks every end within A flips of s, the empty set (end s, d = 0) included. An
// action is a non-empty set, whose end is never s. So the best action is the first entry of T_A[s] whose end is not s:
// the second entry if the best one ends at s, the best one otherwise. One entry per row cannot make that exclusion:
// the walk i, i returns to s at cost 2k and may beat every legal action.
#pragma once
#include <stdint.h>

#ifndef PBN_HD  // as in pbn_reach_rule.hpp
#if defined(__HIPCC__)  // the compiler's own attributes: no HIP header needed for them
#define PBN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define PBN_HD inline
#endif
#endif

namespace pbn {

constexpr int FLIPSET_D_SHIFT = 24;                     // tag = y | d << 24: y < 2^24 (PBN_STG_MAX_STATES), d <= 15
constexpr int32_t FLIPSET_Y_MASK = (1 << FLIPSET_D_SHIFT) - 1;
constexpr int32_t FLIPSET_EMPTY = -1;                   // the tag of no entry
constexpr int FLIPSET_MAX_FLIPS = 15;                   // d << 24 stays below 2^28: the tag is never negative

struct FlipEntry {
    double base;  // M[y]
    int32_t tag;  // y | d << 24, FLIPSET_EMPTY: none
};

struct FlipPair {
    FlipEntry e0, e1;  // e0 better than e1, distinct ends; e1 may be empty, and then e0 may be
};

PBN_HD FlipEntry flip_none() { return FlipEntry{0.0, FLIPSET_EMPTY}; }
PBN_HD FlipEntry flip_entry(int32_t y, int32_t d, double base) { return FlipEntry{base, y | (d << FLIPSET_D_SHIFT)}; }
PBN_HD bool flip_is(const FlipEntry& e) { return e.tag >= 0; }
PBN_HD int32_t flip_end(const FlipEntry& e) { return e.tag & FLIPSET_Y_MASK; }  // of an entry that is one
PBN_HD int32_t flip_count(const FlipEntry& e) { return e.tag >> FLIPSET_D_SHIFT; }

// a where c, else b, field by field: a select of two values, never of two addresses (a struct picked through `?:` is
// copied from the chosen address, which costs the kernels a private array).
PBN_HD FlipEntry flip_pick(bool c, const FlipEntry& a, const FlipEntry& b) {
    return FlipEntry{c ? a.base : b.base, c ? a.tag : b.tag};
}

// base - k * d: one rounded product, one rounded difference.
PBN_HD double flip_value(const FlipEntry& e, double k) {
#if defined(__clang__)  // hipcc contracts by default; the host checks are built by g++ for baseline x86-64: no fma to form
#pragma clang fp contract(off)
#endif
    const double c = k * (double)flip_count(e);
    return e.base - c;
}

// One more flip on the way to the same end (an empty entry stays empty).
PBN_HD FlipEntry flip_bump(const FlipEntry& e) {
    return FlipEntry{e.base, flip_is(e) ? e.tag + (1 << FLIPSET_D_SHIFT) : FLIPSET_EMPTY};
}

// Is a strictly better than b: larger value, then fewer flips, then the lower end row. An empty entry is better than
// nothing and worse than every entry. With d in the tag's high bits and y in its low bits, "fewer flips, then lower
// end" is tag order.
PBN_HD bool flip_better(const FlipEntry& a, const FlipEntry& b, double k) {
    const double va = flip_value(a, k), vb = flip_value(b, k);
    const bool wins = va > vb || (va == vb && a.tag < b.tag);
    return flip_is(a) && (!flip_is(b) || wins);
}

// Insert e into a top-two-distinct pair.
PBN_HD void flip_insert(FlipPair& p, const FlipEntry& e, double k) {
    const bool same0 = flip_is(e) && flip_is(p.e0) && flip_end(e) == flip_end(p.e0);
    const bool b0 = flip_better(e, p.e0, k), b1 = flip_better(e, p.e1, k);
    // the end of e0: the better of the two is first, e1 (another end) stays
    // the end of e1: e replaces it where it is better, and goes first where it also beats e0 -- (e, e0) or (e0, e)
    // a new end:     first (e, e0), second (e0, e), or dropped: the same two lines
    const FlipEntry first = flip_pick(b0, e, p.e0);
    const FlipEntry second = flip_pick(same0, p.e1, flip_pick(b0, p.e0, flip_pick(b1, e, p.e1)));
    p.e0 = first;
    p.e1 = second;
}

// The top-two-distinct of the union of two pairs.
PBN_HD FlipPair flip_merge(FlipPair a, const FlipPair& b, double k) {
    flip_insert(a, b.e0, k);
    flip_insert(a, b.e1, k);
    return a;
}

// The best action at row s from T_A[s]: the first entry whose end is not s (empty: no allowed node).
PBN_HD FlipEntry flip_action(const FlipPair& p, int32_t s) {
    const bool first_is_s = flip_is(p.e0) && flip_end(p.e0) == s;
    return flip_pick(first_is_s, p.e1, p.e0);
}

}  // namespace pbn
