// chain_split_check.cpp -- the slice rule of step mode's launch chains (csrc/pbn_chain_split.hpp) on the CPU.
//
// Built by `make chainsplitcheck` with ASan + UBSan; no HIP header, no library, no GPU. Exhaustive over
// B in [1, 5000], S in {1, 2, 4} and step blocks {256, 1024}, plus the bench sizes 2^20 and 2^23.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pbn_chain_split.hpp"

using namespace pbn;

#define REQUIRE(cond)                                                                                   \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            std::fprintf(stderr, "chain_split_check: %s failed (B=%llu S=%d block=%d) at line %d\n", #cond, \
                         (unsigned long long)B, S, block, __LINE__);                                    \
            std::exit(1);                                                                               \
        }                                                                                               \
    } while (0)

static void check(uint64_t B, int S, int block) {
    ChainSlice sl[STEP_CHAINS_MAX];
    const int n = chain_split(B, S, block, sl);
    REQUIRE(n >= 1 && n <= S);
    uint64_t at = 0;
    bool block_aligned = true;
    for (int c = 0; c < n; ++c) {
        REQUIRE(sl[c].off == at);         // in order, no gap, no overlap
        REQUIRE(sl[c].len > 0);           // none empty
        REQUIRE((sl[c].off & 1u) == 0u);  // even start
        block_aligned = block_aligned && sl[c].off % (2ull * (uint64_t)block) == 0;
        at += sl[c].len;
    }
    REQUIRE(at == B);  // the slices tile [0, B)
    for (int c = n; c < STEP_CHAINS_MAX; ++c) REQUIRE(sl[c].off == 0 && sl[c].len == 0);
    // clamped only where the batch has fewer env pairs than chains
    REQUIRE(n == S || (B + 1) / 2 < (uint64_t)S);
    // large enough for S whole units of 2 x block envs: every start is a multiple of one
    if (B >= (uint64_t)S * 2ull * (uint64_t)block) REQUIRE(block_aligned);
}

int main() {
    const int chains[] = {1, 2, 4}, blocks[] = {256, 1024};
    for (int block : blocks)
        for (int S : chains) {
            for (uint64_t B = 1; B <= 5000; ++B) check(B, S, block);
            check(1ull << 20, S, block);
            check(1ull << 23, S, block);
        }
    {
        const uint64_t B = 1ull << 20;
        const int S = 2, block = 1024;
        ChainSlice sl[STEP_CHAINS_MAX];
        REQUIRE(chain_split(B, S, block, sl) == 2);
        REQUIRE(sl[0].off == 0 && sl[0].len == (1ull << 19));
        REQUIRE(sl[1].off == (1ull << 19) && sl[1].len == (1ull << 19));
    }
    {  // out-of-range chain counts are clamped, never trusted
        const uint64_t B = 4099;
        int S = 1;
        const int block = 256;
        ChainSlice sl[STEP_CHAINS_MAX];
        REQUIRE(chain_split(B, 0, block, sl) == 1);
        REQUIRE(chain_split(B, -3, block, sl) == 1);
        REQUIRE(chain_split(B, 9, block, sl) == STEP_CHAINS_MAX);
        (void)S;
    }
    std::puts("chain_split_check ok");
    return 0;
}
