// pbn_step_plan.hpp -- what step mode (pbn_step, pbn_step_prepare) does with a batch and with a call, decided
// from plain integers: the batch's shape (block, launch chains, graphs on or off), a call's plan (a run or
// single launches, split into the chains or not, graphs or plain launches) and how a run is cut into graph
// replays. Finding or building a graph, and what follows a failed capture, stay with the caller
// (pbn_abi_sim.cpp): they depend on HIP results.
//
// No HIP and no other project header but the slice rule: tests/host/step_plan_check.cpp compiles it alone.
#pragma once
#include <cstdint>

#include "pbn_chain_split.hpp"

namespace pbn {

constexpr uint32_t STEP_GRAPH_K = 64;  // longest captured run of step launches
constexpr int STEP_GRAPH_SIZES = 6;     // graphs of 64, 32, 16, 8, 4 and 2 launches
// the smallest graph is the shortest run (StepCall::run): every run that may use graphs has a replay to make
static_assert(STEP_GRAPH_K >> (STEP_GRAPH_SIZES - 1) == 2, "the smallest step graph holds two launches");
constexpr uint64_t STEP_GRAPH_MAX_WORDS = 1ull << 20;  // state words from which step mode launches plainly
// ... and from which a batch stepped as two or more launch chains does: each step is one launch per chain, and
// the host issues plain launches at 3.3-4.4 us each (1M Bittner-200 envs, two chains: 8.5 us per step plain,
// 5.45 as graphs; 2M: 11.6 vs 10.5; 4M: 19.8 vs 20.5)
constexpr uint64_t STEP_CHAIN_GRAPH_MAX_WORDS = 1ull << 24;
// Updates from which a call is split into the chains chosen by size: the fork, the join and a graph start per
// chain cost a call about 20 us (1M Bittner-200 envs, bench.py --warmup 5, us per step, one chain -> two:
// 20 steps 9.7 -> 10.6, 64 steps 8.8 -> 8.7, 200 steps 8.0 -> 7.5; 1,000 steps after 200: 6.5 -> 5.9)
constexpr uint32_t STEP_CHAIN_MIN_UPDATES = 128;

// Step mode of one batch, fixed at pbn_batch_create.
struct StepShape {
    int block = 1024;                // threads per workgroup of the Philox step kernel (256 or 1024)
    int chains = 1;                  // launch chains in use (pbn_batch_info.step_chains)
    ChainSlice sl[STEP_CHAINS_MAX];  // sl[0 .. chains): the batch in order
    uint32_t min_updates = 2;        // calls of fewer updates run as one chain (2 = every run)
    // step mode without HIP graphs: by default for large batches (a graph replay's start on the
    // device costs more than host submission, which a long kernel hides: 1M Bittner-200 envs, 20
    // launches: 9.3 us per launch plain vs 9.9 us as one replay); PBNSIM_STEP_GRAPH=0/1 forces it
    bool graphs_off = false;
};

// B envs of W state words on n_cu compute units; the knobs (Knobs, pbn_host.hpp): step_block 256 / 1024 or 0,
// step_chains 1 / 2 / 4 or 0, step_graph 0 / 1 or -1 (0 and -1: by size), envs_per_thread >= 1.
inline StepShape step_shape(uint64_t B, int W, int n_cu, int step_block, int step_chains, int step_graph,
                            int envs_per_thread) {
    StepShape s;
    // envs from which one step launch fills every CU with 1024-thread workgroups
    const uint64_t fill = (uint64_t)n_cu * 1024u * (uint64_t)envs_per_thread;
    // 1024-thread groups stage the image 4x less often; small batches need more, smaller groups
    s.block = step_block ? step_block : B >= fill ? 1024 : 256;
    // Launch chains by batch size (chain_split clamps to the batch): two from the size at which each half still
    // fills every CU with 1024-thread workgroups. One chain's dispatch ramp, tail and kernel boundary then
    // overlap the other chain's kernel. Measured on MI355X (profiles/step_chains_ab.json, us per step, one
    // chain -> two): Bittner-200 1M envs 5.9 -> 5.45, 2M 12.6 -> 10.5, 4M 23.3 -> 19.8, 8M 45.0 -> 39.3; half
    // that size (524,288 envs) 4.13 -> 4.37, and 65,536 Bittner-28 envs 3.03 -> 3.37: one chain there. Four
    // chains were slower than two at every size.
    const int chains = step_chains ? step_chains : s.block == 1024 && B >= 2 * fill ? 2 : 1;
    s.chains = chain_split(B, chains, s.block, s.sl);
    s.min_updates = step_chains ? 2u : STEP_CHAIN_MIN_UPDATES;  // a forced count holds for every run
    // two chains issue two launches per step: below STEP_CHAIN_GRAPH_MAX_WORDS the host does not keep up with
    // them plainly, so a chained batch replays per-chain graphs up to there
    s.graphs_off = step_graph >= 0 ? step_graph == 0
                                   : B * (uint64_t)W >= (s.chains > 1 ? STEP_CHAIN_GRAPH_MAX_WORDS : STEP_GRAPH_MAX_WORDS);
    return s;
}

// The dirty write-back of the 1024-thread step kernels (STORE_HALF against STORE_DIRTY, pbn_params.hpp) by size:
// only the changed 16-B half of an env while the whole batch is resident at once -- two 1024-thread workgroups
// per CU, one env pair per thread, so n_cu x 4096 envs: the launch is one round of workgroups, it ends with its
// slowest wave, and one store instruction per env instead of two shortens that (1M Bittner-200 envs on 256 CUs,
// plain launches: 9.54 -> 8.83 us per step; 512K envs 5.25 -> 5.19). A larger batch keeps workgroups queued behind the resident ones and
// runs at the rate of its memory traffic, where a half-written 32-B sector costs more than a whole one (2M envs
// 14.6 -> 15.7 us per step with the half store, 4M 27.9 -> 29.7, 8M 55.5 -> 59.2): the whole env there.
// profiles/step_half_store_ab.json
inline bool step_half_store(uint64_t B, int n_cu, int block) {
    return block == 1024 && B <= (uint64_t)n_cu * 4096u;
}

// One pbn_step call (pbn_step_prepare: the call it prepares).
struct StepCall {
    // two or more updates, no event pair per launch (timing mode 1), not inside the caller's capture of the
    // stream. Only a run replays graphs, and only a run is split into the batch's launch chains.
    bool run = false;
    bool chained = false;  // issued as the shape's chains, forked off and joined back into the batch's stream
    // may replay graphs. Those of a batch with chains cover the chains' slices: its unsplit calls launch plainly
    bool graphs = false;
    bool capture = false;  // ... and may capture the ones it lacks: the null stream cannot capture
};

inline StepCall step_call(const StepShape& s, uint32_t n_updates, int timing_mode, bool capturing, bool null_stream) {
    StepCall c;
    c.run = !capturing && timing_mode != 1 && n_updates >= 2;
    c.chained = c.run && s.chains > 1 && n_updates >= s.min_updates;
    c.graphs = c.run && !s.graphs_off && (s.chains == 1 || c.chained);
    c.capture = c.graphs && !null_stream;
    return c;
}

// A call of n updates may replay one graph of exactly n launches (StepGraphs::exact_graph); longer runs replay
// the power-of-two graphs (one graph of thousands of launches replayed slower: 3.43 vs 3.16 us per launch at
// 65,536 Bittner-28 envs)
inline bool step_exact_fits(uint32_t n_updates) { return n_updates >= 2 && n_updates <= STEP_GRAPH_K; }

// n updates as power-of-two graphs: replays[j] of the (STEP_GRAPH_K >> j)-graph in that order -- 64-graphs, then
// the binary digits of the rest (n = 20: the 16- and the 4-graph) --, then `plain` single launches (n odd: one).
struct StepPow2 {
    uint32_t replays[STEP_GRAPH_SIZES] = {};
    uint32_t plain = 0;
};

inline StepPow2 step_pow2(uint32_t n_updates) {
    StepPow2 d;
    d.replays[0] = n_updates / STEP_GRAPH_K;
    for (int j = 1; j < STEP_GRAPH_SIZES; ++j) d.replays[j] = n_updates / (STEP_GRAPH_K >> j) & 1u;
    d.plain = n_updates % (STEP_GRAPH_K >> (STEP_GRAPH_SIZES - 1));
    return d;
}

}  // namespace pbn
