// mass_rule_check.cpp -- the law of the update (csrc/pbn_mass_rule.hpp) on the CPU, under ASan + UBSan
// (`make massrulecheck`).
//
// No HIP, no GPU, no library, no fixture file. Two parts:
//   1. an image of each kind written out by hand in this file (layout words and table bytes, no packer), with the
//      masses worked out by hand;
//   2. random networks made in code, their images built by the packers of pbn_image.cpp (compiled in), the mass the
//      kernel evaluates (edge_mass, and net_edge_mass over it) against a restatement from the descriptor that never
//      sees an image, plus the two identities: the masses of a node's two values add up to 2^53, and mass > 0
//      exactly where the support rule of pbn_reach_rule.hpp says the node can flip.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
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

constexpr uint64_t ONE = MASS_ONE;

// ---------------------------------------------------------------- part 1: images by hand
static uint64_t rec_word(uint32_t in0, uint32_t in1, uint32_t in2, uint16_t tt) {
    return (uint64_t)in0 | (uint64_t)in1 << 16 | (uint64_t)in2 << 32 | (uint64_t)tt << 48;
}

// Three nodes, tp = 2 thresholds and pmax = 3 record slots per node:
//   node 0: predictors NOT-self [0, ONE/4), self [ONE/4, ONE/4) (empty), constant 1 [ONE/4, ONE);
//   node 1: one predictor, copy of node 0 (thresholds: the padding UINT64_MAX);
//   node 2: XOR of nodes 0 and 1 on [0, 5), self on [5, ONE + 9 -> clamped to ONE), a NOT-self slot that is never reached.
static void check_predictor_by_hand() {
    NetLayout L{};
    L.kind = KIND_PREDICTOR_MIX;
    L.n_nodes = 3;
    L.tp = 2;
    L.pmax = 3;
    L.off_thr = 0;
    L.off_rec = 3 * 2 * 8;
    L.bytes = L.off_rec + 3 * 3 * 8;
    std::vector<uint64_t> im(L.bytes / 8);
    uint64_t* thr = im.data();
    uint64_t* rec = im.data() + L.off_rec / 8;
    // pattern p = x_in0 << 3 | x_in1 << 2 | x_in2 << 1 | x_self; bit p of tt is the output
    const uint16_t SELF = 0xAAAA, NOT_SELF = 0x5555, CONST1 = 0xFFFF, COPY_IN0 = 0xFF00, XOR01 = 0x0FF0;
    thr[0] = ONE / 4, thr[1] = ONE / 4;
    rec[0] = rec_word(0, 0, 0, NOT_SELF), rec[1] = rec_word(0, 0, 0, SELF), rec[2] = rec_word(0, 0, 0, CONST1);
    thr[2] = ~0ull, thr[3] = ~0ull;
    rec[3] = rec_word(0, 1, 1, COPY_IN0), rec[4] = rec[3], rec[5] = rec[3];
    thr[4] = 5, thr[5] = ONE + 9;
    rec[6] = rec_word(0, 1, 2, XOR01), rec[7] = rec_word(2, 2, 2, SELF), rec[8] = rec_word(2, 2, 2, NOT_SELF);
    const uint8_t* tbl = reinterpret_cast<const uint8_t*>(im.data());
    for (uint64_t x = 0; x < 8; x++) {
        auto bit = [&x](uint32_t j) { return state_bit(&x, j); };
        const uint32_t x0 = x & 1, x1 = (x >> 1) & 1, x2 = (x >> 2) & 1;
        // node 0: from 0 both live predictors give 1 (mass ONE); from 1 only NOT-self leaves it (ONE / 4)
        CHECK(edge_mass<KIND_PREDICTOR_MIX>(bit, 0, 0, tbl, L) == (x0 ? ONE / 4 : ONE));
        // node 1 copies node 0: all or nothing
        CHECK(edge_mass<KIND_PREDICTOR_MIX>(bit, 1, 0, tbl, L) == (x0 != x1 ? ONE : 0));
        // node 2: only the 5 draws of the XOR predictor can move it, when x0 ^ x1 differs from it
        CHECK(edge_mass<KIND_PREDICTOR_MIX>(bit, 2, 0, tbl, L) == ((x0 ^ x1) != x2 ? 5u : 0u));
        for (uint32_t i = 0; i < 3; i++) {
            CHECK(edge_mass<KIND_PREDICTOR_MIX>(bit, i, i + 1, tbl, L) == 0);  // below `first`: frozen
            CHECK(can_flip<KIND_PREDICTOR_MIX>(bit, i, 0, tbl, L) == (edge_mass<KIND_PREDICTOR_MIX>(bit, i, 0, tbl, L) > 0));
        }
    }
}

// Three nodes: node 0 constant (k = 0) with T = ONE / 2; node 1 with input 2: T = {0, ONE}; node 2 with inputs 0, 1
// (first = most significant): T = {1, ONE - 1, ONE + 7 (clamped), 12345}.
static void check_table_by_hand() {
    NetLayout L{};
    L.kind = KIND_PROB_TABLE;
    L.n_nodes = 3;
    L.off_node = 0;
    L.off_rec = 3 * 8;           // u16 inputs: {2}, {0, 1}
    L.off_thr = L.off_rec + 8;   // u64 thresholds, 8-byte aligned
    L.bytes = L.off_thr + 7 * 8;
    std::vector<uint64_t> im(L.bytes / 8 + 1);
    uint8_t* b = reinterpret_cast<uint8_t*>(im.data());
    auto info = [](uint32_t toff, uint32_t ioff, uint32_t k) { return (uint64_t)toff | (uint64_t)ioff << 32 | (uint64_t)k << 48; };
    im[0] = info(0, 0, 0), im[1] = info(1, 0, 1), im[2] = info(3, 1, 2);
    const uint16_t in[3] = {2, 0, 1};
    memcpy(b + L.off_rec, in, sizeof in);
    const uint64_t T[7] = {ONE / 2, 0, ONE, 1, ONE - 1, ONE + 7, 12345};
    memcpy(b + L.off_thr, T, sizeof T);
    for (uint64_t x = 0; x < 8; x++) {
        auto bit = [&x](uint32_t j) { return state_bit(&x, j); };
        const uint32_t x0 = x & 1, x1 = (x >> 1) & 1, x2 = (x >> 2) & 1;
        CHECK(edge_mass<KIND_PROB_TABLE>(bit, 0, 0, b, L) == ONE / 2);
        CHECK(edge_mass<KIND_PROB_TABLE>(bit, 0, 1, b, L) == 0);  // the step graph: node 0 never moves
        const uint64_t t1 = x2 ? ONE : 0;
        CHECK(edge_mass<KIND_PROB_TABLE>(bit, 1, 1, b, L) == (x1 ? ONE - t1 : t1));
        const uint64_t raw = T[3 + 2 * x0 + x1], t2 = raw > ONE ? ONE : raw;
        CHECK(edge_mass<KIND_PROB_TABLE>(bit, 2, 0, b, L) == (x2 ? ONE - t2 : t2));
        for (uint32_t i = 0; i < 3; i++)
            for (uint32_t first = 0; first < 2; first++)
                CHECK(can_flip<KIND_PROB_TABLE>(bit, i, first, b, L) == (edge_mass<KIND_PROB_TABLE>(bit, i, first, b, L) > 0));
    }
}

// ---------------------------------------------------------------- part 2: packer-built images of random networks
static void init_net(pbn_net* n, const pbn_net_desc& d) {
    n->kind = d.kind;
    n->N = d.n_nodes;
    n->W = (d.n_nodes + 63) / 64;
}

struct TableNet {
    std::vector<int32_t> k, ioff, inputs;
    std::vector<int64_t> toff;
    std::vector<uint64_t> thr;
    pbn_net_desc desc{};
    int N = 0;
};

static uint64_t random_threshold() {
    switch (rnd() % 8) {
        case 0: return 0;
        case 1: return ONE;
        case 2: return 1;
        case 3: return ONE - 1;
        default: return (uint64_t)std::ceil(std::ldexp((double)(rnd() >> 11) * std::ldexp(1.0, -53), 53));
    }
}

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
        for (int e = 0; e < 1 << ks[i]; e++) t.thr.push_back(random_threshold());
        t.toff.push_back((int64_t)t.thr.size());
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

static void check_table(const std::vector<int>& ks, int n_states) {
    const TableNet t = make_table(ks);
    pbn_net net;
    init_net(&net, t.desc);
    CHECK(build_table_image(&t.desc, &net) == 0);
    const int W = net.W, N = t.N;
    const std::vector<uint64_t> states = random_states(N, n_states);
    std::vector<uint64_t> mass((size_t)n_states * N), masks(states.size());
    const int graphs[2] = {PBN_TABLE_GRAPH_STG, PBN_TABLE_GRAPH_STEP};
    for (int graph : graphs) {
        const int first = graph == PBN_TABLE_GRAPH_STEP ? 1 : 0;
        net_edge_mass(&net, graph, states.data(), (uint64_t)n_states, mass.data());
        net_unstable(&net, graph, states.data(), (uint64_t)n_states, masks.data());
        for (int e = 0; e < n_states; e++) {
            const uint64_t* s = states.data() + (size_t)e * W;
            for (int i = 0; i < N; i++) {
                size_t idx = 0;
                for (int q = t.ioff[i]; q < t.ioff[i] + t.k[i]; q++) idx = 2 * idx + state_bit(s, (uint32_t)t.inputs[q]);
                const uint64_t T = t.thr[(size_t)t.toff[i] + idx];
                const uint64_t want = i < first ? 0 : state_bit(s, (uint32_t)i) ? ONE - T : T;
                CHECK(mass[(size_t)e * N + i] == want);
                CHECK((want > 0) == (state_bit(masks.data() + (size_t)e * W, (uint32_t)i) != 0));
            }
        }
    }
}

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
            t[q] = r == 0 ? 0 : r == 1 ? ONE : r == 2 ? ONE + 5 : rnd() >> (11 + rnd() % 3 * 20);
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
    p.desc.n_preds = (int32_t)p.tt.size();
    p.desc.n_nodes = p.N;
    p.desc.pred_offsets = p.offsets.data();
    p.desc.pred_inputs = p.inputs.data();
    p.desc.pred_tt = p.tt.data();
    p.desc.pred_thr = p.thr.data();
    return p;
}

// PredictorNetwork.update_probability's arithmetic (network.py): the mass with which node i becomes `value` at s.
static uint64_t pred_mass_to(const PredNet& p, const uint64_t* s, int i, uint32_t value) {
    const int o0 = p.offsets[i], o1 = p.offsets[i + 1];
    const uint32_t x = state_bit(s, (uint32_t)i);
    uint64_t prev = 0, mass = 0;
    for (int j = o0; j < o1; j++) {
        const uint64_t t = j < o1 - 1 ? std::min(p.thr[j], ONE) : ONE;
        const uint64_t w = t > prev ? t - prev : 0;
        prev = std::max(prev, t);
        const uint32_t pat = (state_bit(s, (uint32_t)p.inputs[3 * j]) << 3) | (state_bit(s, (uint32_t)p.inputs[3 * j + 1]) << 2) |
                             (state_bit(s, (uint32_t)p.inputs[3 * j + 2]) << 1) | x;
        if ((((uint32_t)p.tt[j] >> pat) & 1u) == value) mass += w;
    }
    return mass;
}

static void check_pred(const std::vector<int>& counts, int n_states) {
    const PredNet p = make_pred(counts);
    pbn_net net;
    init_net(&net, p.desc);
    CHECK(build_predictor_image(&p.desc, &net) == 0);
    const int W = net.W, N = p.N;
    const std::vector<uint64_t> states = random_states(N, n_states);
    std::vector<uint64_t> mass((size_t)n_states * N), masks(states.size());
    net_edge_mass(&net, 77, states.data(), (uint64_t)n_states, mass.data());  // the graph code is ignored
    net_unstable(&net, 77, states.data(), (uint64_t)n_states, masks.data());
    for (int e = 0; e < n_states; e++) {
        const uint64_t* s = states.data() + (size_t)e * W;
        auto bit = [s](uint32_t j) { return state_bit(s, j); };
        for (int i = 0; i < N; i++) {
            const uint32_t x = state_bit(s, (uint32_t)i);
            const uint64_t want = pred_mass_to(p, s, i, 1u - x);
            CHECK(want + pred_mass_to(p, s, i, x) == ONE);  // the live widths add up to the whole range
            CHECK(mass[(size_t)e * N + i] == want);
            CHECK(edge_mass<KIND_PREDICTOR_MIX>(bit, (uint32_t)i, 0u, net.image.data(), net.L) == want);
            CHECK((want > 0) == (state_bit(masks.data() + (size_t)e * W, (uint32_t)i) != 0));
        }
    }
}

int main() {
    check_predictor_by_hand();
    check_table_by_hand();
    check_table({0, 1, 2, 3, 4, 5, 6, 0, 0}, 512);
    std::vector<int> ks;
    for (int i = 0; i < 64; i++) ks.push_back((int)(rnd() % 5));
    check_table(ks, 300);  // the last node at bit 63
    ks.push_back(3);
    check_table(ks, 300);  // 65 nodes: the last one alone in word 1
    ks.clear();
    for (int i = 0; i < 200; i++) ks.push_back(i == 17 ? 10 : i == 130 ? 0 : (int)(rnd() % 6));
    check_table(ks, 200);  // four words, one wide table
    check_pred({1, 2, 3, 1, 4, 2, 7, 1}, 256);
    std::vector<int> counts;
    for (int i = 0; i < 130; i++) counts.push_back(1 + (int)(rnd() % 5));
    check_pred(counts, 200);
    printf("mass_rule_check ok\n");
    return 0;
}
