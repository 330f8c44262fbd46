// image_check.cpp -- the packers of csrc/pbn_image.cpp on the CPU, under ASan + UBSan (`make imagecheck`).
//
// No HIP, no GPU, no library: this program is compiled together with pbn_image.cpp, builds its descriptors
// in code and checks the packed images against rules stated from the descriptors (not from the packers' code).
#define PBN_HOST_NO_HIP
#include "pbn_host.hpp"

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

static uint64_t k53(uint64_t a) { return (a << 21) | (a >> 11); }  // a < 2^32

// The smallest choice word a in [0, 2^32] with k53(a) >= T (2^32: none), by bisection: k53 is monotone.
static uint64_t first_word_passing(uint64_t T) {
    uint64_t lo = 0, hi = 1ull << 32;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (k53(mid) >= T) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <class T>
static T load(const uint8_t* p) {
    T v;
    memcpy(&v, p, sizeof v);
    return v;
}

// ---------------------------------------------------------------- predictor-mix networks
struct PredNet {
    std::vector<int32_t> offsets, inputs;
    std::vector<uint16_t> tt;
    std::vector<uint64_t> thr;  // per predictor; a node's first c - 1 are its thresholds
    pbn_net_desc desc{};
    int N = 0;
    uint64_t record(int j) const {
        return (uint64_t)(uint32_t)inputs[3 * j] | ((uint64_t)(uint32_t)inputs[3 * j + 1] << 16) |
               ((uint64_t)(uint32_t)inputs[3 * j + 2] << 32) | ((uint64_t)tt[j] << 48);
    }
};

// counts[i] predictors at node i; rows[i] (if given) its thresholds, else random non-decreasing ones below 2^53
static PredNet make_pred(const std::vector<int>& counts, const std::vector<std::vector<uint64_t>>& rows = {}) {
    PredNet p;
    p.N = (int)counts.size();
    p.offsets.push_back(0);
    for (int i = 0; i < p.N; i++) {
        const int c = counts[i];
        std::vector<uint64_t> t(c, 0);
        for (int q = 0; q + 1 < c; q++) t[q] = i < (int)rows.size() && !rows[i].empty() ? rows[i][q] : rnd() >> 11;
        std::sort(t.begin(), t.begin() + (c - 1));
        t[c - 1] = c > 1 ? t[c - 2] : 0;  // the last entry is never a threshold; keep the row non-decreasing
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

static void init_net(pbn_net* n, const pbn_net_desc& d) {
    n->kind = d.kind;
    n->N = d.n_nodes;
    n->W = (d.n_nodes + 63) / 64;
}

// Env config over `net` with H random cubes; care_nodes > 0: cube 0 cares about exactly that many nodes.
struct EnvDesc {
    std::vector<uint64_t> care, value, tcare, tvalue, rcare, rvalue;
    pbn_envcfg_desc desc{};
};

static EnvDesc make_env(const pbn_net& net, int H, int H_reset, int care_nodes = 0) {
    EnvDesc e;
    const int W = net.W;
    const uint64_t top = net.N % 64 ? (1ull << (net.N % 64)) - 1 : ~0ull;
    auto word = [&](int k, bool sparse) { return (sparse ? rnd() & rnd() & rnd() : rnd()) & (k == W - 1 ? top : ~0ull); };
    for (int h = 0; h < H; h++)
        for (int k = 0; k < W; k++) {
            e.care.push_back(word(k, true));
            e.value.push_back(word(k, false));  // bits outside care are set too: the packer masks them
        }
    if (care_nodes) {
        for (int k = 0; k < W; k++) e.care[k] = 0;
        for (int i = 0; i < care_nodes; i++) e.care[i / 64] |= 1ull << (i % 64);
    }
    for (int k = 0; k < W; k++) {
        e.tcare.push_back(word(k, true));
        e.tvalue.push_back(word(k, false));
    }
    for (int k = 0; k < W * H_reset; k++) {
        e.rcare.push_back(rnd());
        e.rvalue.push_back(rnd());
    }
    e.desc.n_cubes = H;
    e.desc.cube_care = H ? e.care.data() : nullptr;
    e.desc.cube_value = H ? e.value.data() : nullptr;
    e.desc.n_reset_cubes = H_reset;
    e.desc.reset_care = H_reset ? e.rcare.data() : nullptr;
    e.desc.reset_value = H_reset ? e.rvalue.data() : nullptr;
    e.desc.target_care = e.tcare.data();
    e.desc.target_value = e.tvalue.data();
    e.desc.horizon = 77;
    e.desc.reward_success = 900;
    e.desc.action_cost = 3;
    e.desc.first_update_tested = 5;
    return e;
}

// Packed byte counters of cubes 0..7 for state x: byte h = cared bits where x differs from cube h.
static void counters(const EnvDesc& e, int H, int W, const std::vector<uint64_t>& x, uint32_t out[2]) {
    out[0] = out[1] = 0;
    for (int h = 0; h < H && h < 8; h++) {
        uint32_t m = 0;
        for (int k = 0; k < W; k++) m += __builtin_popcountll(e.care[(size_t)h * W + k] & (x[k] ^ e.value[(size_t)h * W + k]));
        out[h >> 2] += m << (8 * (h & 3));
    }
}

static void check_envcfg(const pbn_net& net, int H, int H_reset, int care_nodes, int want_fast) {
    const EnvDesc e = make_env(net, H, H_reset, care_nodes);
    const int W = net.W;
    pbn_envcfg c;
    CHECK(build_envcfg_image(net, &e.desc, &c) == 0);
    CHECK(c.W == W && c.H == H && c.H_reset == H_reset && c.counters_ok == want_fast);
    CHECK(c.off_cubes == net.L.bytes && c.off_cubes % 16 == 0 && c.off_target % 16 == 0 && c.off_ndelta % 16 == 0);
    CHECK(c.off_target >= c.off_cubes + 16u * W * H && c.off_ndelta >= c.off_target + 16u * W);
    CHECK(c.L.bytes == c.image.size() && c.L.bytes >= c.off_ndelta + 8u * net.N && c.L.plane_off == c.L.bytes);
    CHECK(memcmp(c.image.data(), net.image.data(), net.L.bytes) == 0);
    const uint8_t* im = c.image.data();
    for (int h = 0; h < H; h++)
        for (int k = 0; k < W; k++) {
            const uint64_t care = e.care[(size_t)h * W + k];
            CHECK(load<uint64_t>(im + c.off_cubes + 8 * ((size_t)h * 2 * W + k)) == care);
            CHECK(load<uint64_t>(im + c.off_cubes + 8 * ((size_t)h * 2 * W + W + k)) == (e.value[(size_t)h * W + k] & care));
        }
    for (int k = 0; k < W; k++) {
        CHECK(load<uint64_t>(im + c.off_target + 8 * (size_t)k) == e.tcare[k]);
        CHECK(load<uint64_t>(im + c.off_target + 8 * (size_t)(W + k)) == (e.tvalue[k] & e.tcare[k]));
    }
    if (c.counters_ok)  // node i going 0 -> 1 moves the packed counters by its delta, from any state
        for (int i = 0; i < net.N; i++) {
            std::vector<uint64_t> x(W);
            for (auto& w : x) w = rnd();
            x[i / 64] &= ~(1ull << (i % 64));
            uint32_t m0[2], m1[2];
            counters(e, H, W, x, m0);
            x[i / 64] |= 1ull << (i % 64);
            counters(e, H, W, x, m1);
            CHECK(load<uint32_t>(im + c.off_ndelta + 8 * (size_t)i) == m1[0] - m0[0]);
            CHECK(load<uint32_t>(im + c.off_ndelta + 8 * (size_t)i + 4) == m1[1] - m0[1]);
        }
    CHECK(c.reset.size() == 2 * (size_t)H_reset * W);
    for (size_t k = 0; k < (size_t)H_reset * W; k++)
        CHECK(c.reset[k] == e.rcare[k] && c.reset[(size_t)H_reset * W + k] == e.rvalue[k]);
    CHECK(c.horizon == 77 && c.reward_success == 900 && c.action_cost == 3 && c.first_tested == 1);
}

// The cooperative-draw image over an env config of `net`: its u32 threshold rows are the compact image's,
// its 16-B records re-encode the records the rule selects, its cubes are the config's moved up by erec_shift.
static void check_gen_image(const PredNet& p, const pbn_net& net, int H) {
    const EnvDesc e = make_env(net, H, 1);
    pbn_envcfg c;
    CHECK(build_envcfg_image(net, &e.desc, &c) == 0);
    const Thr32 X = thr32_layout(c.L);
    const uint32_t N = (uint32_t)net.N;
    const uint32_t erec_shift = c.L.off_rec + 16u * N * X.rs - c.off_cubes;  // as env_plan (pbn_env_plan.hpp) sets it
    const std::vector<uint8_t> g = env_gen_image(&c, erec_shift);
    CHECK(g.size() == (size_t)c.L.bytes + erec_shift);
    CHECK(memcmp(g.data(), net.image.data() + net.L.bytes, 4 * (size_t)N * X.tp4) == 0);
    CHECK(memcmp(g.data() + c.off_cubes + erec_shift, c.image.data() + c.off_cubes, c.L.bytes - c.off_cubes) == 0);
    const uint32_t row = ENV_BLOCK * 4u, nd = c.off_ndelta + erec_shift;
    for (uint32_t i = 0; i < N; i++) {
        const int o = p.offsets[i], cnt = p.offsets[i + 1] - o;
        uint32_t below = 0;  // thresholds some choice word reaches
        for (int q = 0; q + 1 < cnt; q++) below += first_word_passing(p.thr[o + q]) >> 32 ? 0u : 1u;
        for (uint32_t q = 0; q < X.rs; q++) {
            const uint32_t src = q == X.tp4 ? below : q;
            const uint64_t rec = src < (uint32_t)cnt ? p.record(o + (int)src) : 0;
            const uint32_t x0 = rec & 0xFFFF, x1 = (rec >> 16) & 0xFFFF, x2 = (rec >> 32) & 0xFFFF;
            const uint32_t want[4] = {(x0 >> 5) * row | ((x1 >> 5) * row) << 16, (x2 >> 5) * row | ((i >> 5) * row) << 16,
                                      (x0 & 31) | (x1 & 31) << 8 | (x2 & 31) << 16 | (i & 31) << 24,
                                      (uint32_t)(rec >> 48) | (nd + 8 * i) << 16};
            CHECK(memcmp(g.data() + c.L.off_rec + 16 * ((size_t)i * X.rs + q), want, 16) == 0);
        }
    }
}

static void check_pred(const PredNet& p, uint32_t want_tp, uint32_t want_tp4, uint32_t want_rs, bool env = true) {
    pbn_net net;
    init_net(&net, p.desc);
    CHECK(build_predictor_image(&p.desc, &net) == 0);
    const Thr32 X = thr32_layout(net.L);
    CHECK(net.L.tp == want_tp && X.tp4 == want_tp4 && X.rs == want_rs);
    CHECK(net.L.bytes % 16 == 0 && X.rec_off % 16 == 0 && net.image.size() == (size_t)net.L.bytes + X.bytes);
    CHECK(net.L.plane_off == std::max(net.L.bytes, X.bytes) && net.L.plane_off <= MAX_IMAGE);
    // Predstep's rule from the descriptor: predictor j = the count of k53(a) >= T_q over the node's c - 1
    // thresholds, capped at c - 1 -- at a = 0, a = 2^32 - 1 and the words either side of every threshold
    for (int i = 0; i < p.N; i++) {
        const int o = p.offsets[i], c = p.offsets[i + 1] - o;
        std::vector<uint64_t> words = {0, 0xFFFFFFFFull};
        for (int q = 0; q + 1 < c; q++) {
            const uint64_t t = first_word_passing(p.thr[o + q]);
            for (uint64_t w : {t - 1, t, t + 1})
                if (w < (1ull << 32)) words.push_back(w);  // t - 1 wraps at t = 0: dropped here
        }
        for (uint64_t a : words) {
            int j = 0;
            for (int q = 0; q + 1 < c; q++) j += k53(a) >= p.thr[o + q] ? 1 : 0;
            j = std::min(j, c - 1);
            CHECK(net_select_u32(&net, i, (uint32_t)a) == p.record(o + j));
        }
    }
    if (!env) return;  // the network alone fills the budget: no room for an env config
    check_gen_image(p, net, 3);
    for (int H : {0, 4, 8, 9}) check_envcfg(net, H, 2, 0, H <= 8 ? 1 : 0);
    check_envcfg(net, 2, 0, 0, 1);  // no reset cubes: null reset arrays
    if (net.N >= 256) check_envcfg(net, 2, 1, 256, 0);  // a cube caring about 256 nodes: no byte counters
}

// ---------------------------------------------------------------- truth-table networks
static int table_rc(const std::vector<int>& ks, pbn_net* net, std::string* msg = nullptr) {
    const int N = (int)ks.size();
    std::vector<int32_t> node_k(ks.begin(), ks.end()), in_off, inputs;
    std::vector<int64_t> thr_off;
    std::vector<uint64_t> thr;
    for (int i = 0; i < N; i++) {
        in_off.push_back((int32_t)inputs.size());
        thr_off.push_back((int64_t)thr.size());
        for (int q = 0; q < ks[i]; q++) inputs.push_back((int32_t)(rnd() % (uint64_t)N));
        for (int q = 0; q < 1 << ks[i]; q++) thr.push_back(rnd() >> 11);
    }
    pbn_net_desc d{};
    d.kind = PBN_KIND_PROB_TABLE;
    d.n_nodes = N;
    d.node_k = node_k.data();
    d.input_offsets = in_off.data();
    d.inputs = inputs.empty() ? nullptr : inputs.data();
    d.thr_offsets = thr_off.data();
    d.thr = thr.data();
    init_net(net, d);
    const int rc = build_table_image(&d, net);
    if (msg) *msg = g_err;
    if (rc) return rc;
    const NetLayout& L = net->L;
    CHECK(L.kind == KIND_PROB_TABLE && L.n_nodes == N && L.bytes % 16 == 0 && L.plane_off == L.bytes);
    CHECK(net->image.size() == L.bytes && L.bytes <= MAX_IMAGE);
    CHECK(net->kmax == *std::max_element(ks.begin(), ks.end()));
    const uint8_t* im = net->image.data();
    for (int i = 0; i < N; i++) {
        const uint64_t info = load<uint64_t>(im + L.off_node + 8 * (size_t)i);
        CHECK((uint32_t)info == (uint32_t)thr_off[i] && ((info >> 32) & 0xFFFF) == (uint64_t)in_off[i] && (info >> 48) == (uint64_t)ks[i]);
        for (int q = 0; q < ks[i]; q++) CHECK(load<uint16_t>(im + L.off_rec + 2 * (size_t)(in_off[i] + q)) == inputs[in_off[i] + q]);
    }
    CHECK(memcmp(im + L.off_thr, thr.data(), 8 * thr.size()) == 0);
    return 0;
}

int main() {
    // one predictor per node: no thresholds at all
    check_pred(make_pred(std::vector<int>(40, 1)), 0, 0, 1);
    // the threshold edge cases in one row of six (seven predictors), among ordinary nodes
    const uint64_t two21 = 1ull << 21, two53 = 1ull << 53;
    check_pred(make_pred({3, 7, 1, 2, 4}, {{}, {0, two21 - 1, two21, two53 - two21 + 1, two53 - 1, two53}}), 6, 8, 9);
    // W = 8 (N = 512) with two predictors per node
    check_pred(make_pred(std::vector<int>(512, 2)), 2, 4, 5);
    // pmax = 16 (rows are padded to pmax: 256 B per node); N = 192 lands exactly on the LDS budget ...
    {
        std::vector<int> counts(100, 5);
        counts[17] = 16;
        check_pred(make_pred(counts), 16, 16, 17);
        counts.resize(192, 3);
        const PredNet p = make_pred(counts);
        check_pred(p, 16, 16, 17, false);
        pbn_net net;
        init_net(&net, p.desc);
        CHECK(build_predictor_image(&p.desc, &net) == 0 && net.L.plane_off == MAX_IMAGE);
    }
    {  // ... so pmax = 16 at N = 512 is refused
        std::vector<int> counts(512, 1);
        counts[0] = 16;
        const PredNet p = make_pred(counts);
        pbn_net net;
        init_net(&net, p.desc);
        CHECK(build_predictor_image(&p.desc, &net) == PBN_E_UNSUPPORTED && g_err.find("LDS budget") != std::string::npos);
    }
    // truth tables: k = 0 next to the widest node that fits; k = 16 passes the input-count check but its 2^16
    // thresholds are past the budget
    pbn_net t;
    std::string msg;
    CHECK(table_rc({0, 12, 0, 3}, &t) == 0);
    {
        pbn_net u;
        CHECK(table_rc({0, 16}, &u, &msg) == PBN_E_UNSUPPORTED && msg.find("probability tables") != std::string::npos);
    }
    {  // exactly MAX_IMAGE: 192 B of node info and inputs + 6,120 thresholds; one more input doubles a table
        pbn_net u, v;
        CHECK(table_rc({12, 10, 9, 8, 7, 6, 5, 3}, &u) == 0 && u.L.bytes == MAX_IMAGE);
        CHECK(table_rc({12, 10, 9, 8, 7, 6, 5, 4}, &v, &msg) == PBN_E_UNSUPPORTED && msg.find("LDS budget") != std::string::npos);
    }
    // env configs at W = 1 over a truth-table network too (the packer is kind-agnostic)
    for (int H : {0, 4, 8, 9}) check_envcfg(t, H, 1, 0, H <= 8 ? 1 : 0);
    // a NULL array is reported through the one error string
    pbn_net_desc bad{};
    bad.kind = PBN_KIND_PREDICTOR_MIX;
    bad.n_nodes = 4;
    pbn_net n;
    CHECK(build_predictor_image(&bad, &n) == PBN_E_INVALID && g_err == "pred_offsets is NULL");
    puts("image_check ok");
    return 0;
}
