// reach_rule_check.cpp -- the support graphs' edge rule (csrc/pbn_reach_rule.hpp) on the CPU, under ASan + UBSan
// (`make reachrulecheck`).
//
// No HIP, no GPU, no library, no fixture file: this program is compiled together with pbn_image.cpp, makes random
// networks in code, lets the packers build their images and checks the rule the kernels evaluate on those images
// (can_flip, and net_unstable over it) against a restatement that never sees an image: for truth tables the
// probabilities as doubles with `> 0.0` / `< 1.0`, for predictor mixes the selection intervals from the descriptor.
#define PBN_HOST_NO_HIP
#include "pbn_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

static void init_net(pbn_net* n, const pbn_net_desc& d) {
    n->kind = d.kind;
    n->N = d.n_nodes;
    n->W = (d.n_nodes + 63) / 64;
}

static uint32_t state_bit(const uint64_t* s, uint32_t j) { return (uint32_t)(s[j >> 6] >> (j & 63u)) & 1u; }

static std::vector<uint64_t> random_states(int N, int count) {
    const int W = (N + 63) / 64;
    const uint64_t top = N % 64 ? (1ull << (N % 64)) - 1 : ~0ull;
    std::vector<uint64_t> s((size_t)count * W);
    for (int e = 0; e < count; e++)
        for (int k = 0; k < W; k++) s[(size_t)e * W + k] = rnd() & (k == W - 1 ? top : ~0ull);
    return s;
}

// ---------------------------------------------------------------- truth-table networks
struct TableNet {
    std::vector<int32_t> k, ioff, inputs;
    std::vector<int64_t> toff;
    std::vector<double> p;
    std::vector<uint64_t> thr;
    pbn_net_desc desc{};
    int N = 0;
};

// One table entry: the values at which the rule could go wrong, and ordinary ones.
static double random_prob() {
    switch (rnd() % 8) {
        case 0: return 0.0;
        case 1: return 1.0;
        case 2: return std::nextafter(0.0, 1.0);  // the smallest double above 0: still an edge 0 -> 1
        case 3: return std::nextafter(1.0, 0.0);  // the largest double below 1: still an edge 1 -> 0
        case 4: return std::ldexp(1.0, -53);      // threshold exactly 1
        default: return (double)(rnd() >> 11) * std::ldexp(1.0, -53);
    }
}

// ks[i] inputs at node i, chosen at random without repeats, ascending (first = most significant table axis)
static TableNet make_table(const std::vector<int>& ks) {
    TableNet t;
    t.N = (int)ks.size();
    t.ioff.push_back(0);
    t.toff.push_back(0);
    for (int i = 0; i < t.N; i++) {
        std::vector<int32_t> in;
        while ((int)in.size() < ks[i]) {
            const int32_t j = (int32_t)(rnd() % (uint64_t)t.N);
            if (std::find(in.begin(), in.end(), j) == in.end()) in.push_back(j);
        }
        std::sort(in.begin(), in.end());
        t.inputs.insert(t.inputs.end(), in.begin(), in.end());
        t.k.push_back(ks[i]);
        t.ioff.push_back((int32_t)t.inputs.size());
        for (int e = 0; e < 1 << ks[i]; e++) {
            const double p = random_prob();
            t.p.push_back(p);
            t.thr.push_back((uint64_t)std::ceil(std::ldexp(p, 53)));  // ceil(p * 2^53): network.py probability_threshold
        }
        t.toff.push_back((int64_t)t.p.size());
    }
    if (t.inputs.empty()) t.inputs.push_back(0);
    t.desc.kind = PBN_KIND_PROB_TABLE;
    t.desc.n_nodes = t.N;
    t.desc.node_k = t.k.data();
    t.desc.input_offsets = t.ioff.data();
    t.desc.inputs = t.inputs.data();
    t.desc.thr_offsets = t.toff.data();
    t.desc.thr = t.thr.data();
    return t;
}

// The restatement: pbn.py:186-199 on the doubles, nodes `first` .. N-1.
static uint32_t table_moves(const TableNet& t, const uint64_t* s, int i, int first) {
    if (i < first) return 0;
    size_t idx = 0;
    for (int q = t.ioff[i]; q < t.ioff[i] + t.k[i]; q++) idx = 2 * idx + state_bit(s, (uint32_t)t.inputs[q]);
    const double prob_true = t.p[(size_t)t.toff[i] + idx];
    const uint32_t x = state_bit(s, (uint32_t)i);
    return (prob_true > 0.0 && x == 0) || (prob_true < 1.0 && x == 1) ? 1u : 0u;
}

static void check_table(const std::vector<int>& ks, int n_states) {
    const TableNet t = make_table(ks);
    pbn_net net;
    init_net(&net, t.desc);
    CHECK(build_table_image(&t.desc, &net) == 0);
    CHECK(net.L.bytes <= REACH_LDS_MAX);
    const int W = net.W;
    const std::vector<uint64_t> states = random_states(t.N, n_states);
    std::vector<uint64_t> masks(states.size());
    const int graphs[2] = {PBN_TABLE_GRAPH_STG, PBN_TABLE_GRAPH_STEP};
    for (int graph : graphs) {
        const int first = graph == PBN_TABLE_GRAPH_STEP ? 1 : 0;
        CHECK((int)table_graph_first_node(graph) == first);
        net_unstable(&net, graph, states.data(), (uint64_t)n_states, masks.data());
        for (int e = 0; e < n_states; e++) {
            const uint64_t* s = states.data() + (size_t)e * W;
            auto bit = [s](uint32_t j) { return state_bit(s, j); };
            for (int i = 0; i < t.N; i++) {
                const uint32_t want = table_moves(t, s, i, first);
                CHECK(can_flip<KIND_PROB_TABLE>(bit, (uint32_t)i, (uint32_t)first, net.image.data(), net.L) == want);
                CHECK(state_bit(masks.data() + (size_t)e * W, (uint32_t)i) == want);
            }
            const uint64_t top = t.N % 64 ? ~0ull << (t.N % 64) : 0;
            CHECK((masks[(size_t)e * W + W - 1] & top) == 0);  // nothing past the last node
        }
    }
}

// The four table values at the two edges of the rule, one node each way: a constant node (k = 0) per value.
static void check_table_edges() {
    TableNet t;
    const double ps[6] = {0.0, std::nextafter(0.0, 1.0), 0.5, std::nextafter(1.0, 0.0), 1.0, 0.0};
    t.N = 6;
    t.ioff.assign(7, 0);
    t.inputs.push_back(0);
    for (int i = 0; i < 6; i++) {
        t.k.push_back(0);
        t.toff.push_back(i);
        t.p.push_back(ps[i]);
        t.thr.push_back((uint64_t)std::ceil(std::ldexp(ps[i], 53)));
    }
    t.toff.push_back(6);
    CHECK(t.thr[0] == 0 && t.thr[1] == 1 && t.thr[3] == REACH_TWO53 - 1 && t.thr[4] == REACH_TWO53);
    t.desc.kind = PBN_KIND_PROB_TABLE;
    t.desc.n_nodes = 6;
    t.desc.node_k = t.k.data();
    t.desc.input_offsets = t.ioff.data();
    t.desc.inputs = t.inputs.data();
    t.desc.thr_offsets = t.toff.data();
    t.desc.thr = t.thr.data();
    pbn_net net;
    init_net(&net, t.desc);
    CHECK(build_table_image(&t.desc, &net) == 0);
    const uint64_t zeros = 0, ones = 0x3F;
    uint64_t m = 0;
    net_unstable(&net, PBN_TABLE_GRAPH_STG, &zeros, 1, &m);
    CHECK(m == 0x1E);  // from 0: every p > 0 moves (nodes 1, 2, 3, 4), the smallest double included
    net_unstable(&net, PBN_TABLE_GRAPH_STG, &ones, 1, &m);
    CHECK(m == 0x2F);  // from 1: every p < 1 moves (nodes 0, 1, 2, 3, 5)
    net_unstable(&net, PBN_TABLE_GRAPH_STEP, &ones, 1, &m);
    CHECK(m == 0x2E);  // node 0 never moves in the step graph
}

// ---------------------------------------------------------------- predictor-mix networks
struct PredNet {
    std::vector<int32_t> offsets, inputs;
    std::vector<uint16_t> tt;
    std::vector<uint64_t> thr;
    pbn_net_desc desc{};
    int N = 0;
};

static PredNet make_pred(const std::vector<int>& counts) {
    PredNet p;
    p.N = (int)counts.size();
    p.offsets.push_back(0);
    for (int i = 0; i < p.N; i++) {
        const int c = counts[i];
        std::vector<uint64_t> t(c, 0);
        // thresholds with repeats (empty intervals), 0 and values at and past 2^53 among them
        for (int q = 0; q + 1 < c; q++) {
            const uint64_t r = rnd() % 6;
            t[q] = r == 0 ? 0 : r == 1 ? REACH_TWO53 : r == 2 ? REACH_TWO53 + 5 : rnd() >> (11 + rnd() % 3 * 20);
        }
        std::sort(t.begin(), t.begin() + (c - 1));
        t[c - 1] = c > 1 ? t[c - 2] : 0;
        for (int q = 0; q < c; q++) {
            p.thr.push_back(t[q]);
            for (int k = 0; k < 3; k++) p.inputs.push_back((int32_t)(rnd() % (uint64_t)p.N));
            p.tt.push_back((uint16_t)rnd());
        }
        p.offsets.push_back((int32_t)p.tt.size());
    }
    p.desc.kind = PBN_KIND_PREDICTOR_MIX;
    p.desc.n_nodes = p.N;
    p.desc.n_preds = (int32_t)p.tt.size();
    p.desc.pred_offsets = p.offsets.data();
    p.desc.pred_inputs = p.inputs.data();
    p.desc.pred_tt = p.tt.data();
    p.desc.pred_thr = p.thr.data();
    return p;
}

// Predictor j of node i is selected for k53 in [T_{j-1}, T_j) on the grid 0 .. 2^53 - 1 (T_{-1} = 0, the last T
// = 2^53): node i can flip iff a predictor with a non-empty interval outputs 1 - x_i.
static uint32_t pred_moves(const PredNet& p, const uint64_t* s, int i) {
    const int o0 = p.offsets[i], o1 = p.offsets[i + 1];
    const uint32_t x = state_bit(s, (uint32_t)i);
    uint64_t lo = 0;
    for (int j = o0; j < o1; j++) {
        const uint64_t hi = j < o1 - 1 ? std::min(p.thr[j], REACH_TWO53) : REACH_TWO53;
        if (hi > lo) {
            const uint32_t pat = (state_bit(s, (uint32_t)p.inputs[3 * j]) << 3) | (state_bit(s, (uint32_t)p.inputs[3 * j + 1]) << 2) |
                                 (state_bit(s, (uint32_t)p.inputs[3 * j + 2]) << 1) | x;
            if ((((uint32_t)p.tt[j] >> pat) & 1u) != x) return 1;
            lo = hi;
        }
    }
    return 0;
}

static void check_pred(const std::vector<int>& counts, int n_states) {
    const PredNet p = make_pred(counts);
    pbn_net net;
    init_net(&net, p.desc);
    CHECK(build_predictor_image(&p.desc, &net) == 0);
    const int W = net.W;
    const std::vector<uint64_t> states = random_states(p.N, n_states);
    std::vector<uint64_t> masks(states.size());
    net_unstable(&net, 77, states.data(), (uint64_t)n_states, masks.data());  // the graph code is ignored
    for (int e = 0; e < n_states; e++) {
        const uint64_t* s = states.data() + (size_t)e * W;
        auto bit = [s](uint32_t j) { return state_bit(s, j); };
        for (int i = 0; i < p.N; i++) {
            const uint32_t want = pred_moves(p, s, i);
            CHECK(can_flip<KIND_PREDICTOR_MIX>(bit, (uint32_t)i, 0u, net.image.data(), net.L) == want);
            CHECK(state_bit(masks.data() + (size_t)e * W, (uint32_t)i) == want);
        }
    }
}

int main() {
    check_table_edges();
    check_table({0, 1, 2, 3, 4, 5, 6, 0, 0}, 512);  // every state of a 9-node network (and repeats)
    std::vector<int> ks;
    for (int i = 0; i < 64; i++) ks.push_back((int)(rnd() % 5));
    check_table(ks, 300);  // the last node at bit 63
    ks.push_back(3);
    check_table(ks, 300);  // 65 nodes: the last one alone in word 1
    ks.clear();
    for (int i = 0; i < 200; i++) ks.push_back(i == 17 ? 10 : i == 130 ? 0 : (int)(rnd() % 6));
    check_table(ks, 200);  // four words, one wide table, lanes of different k side by side
    check_pred({1, 2, 3, 1, 4, 2, 7, 1}, 256);
    std::vector<int> counts;
    for (int i = 0; i < 130; i++) counts.push_back(1 + (int)(rnd() % 5));
    check_pred(counts, 200);
    printf("reach_rule_check ok\n");
    return 0;
}
