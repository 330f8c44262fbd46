// pbn_image.cpp -- the packers: descriptors in, LDS images out. Offset arithmetic and memcpy only; this file
// includes no HIP header and makes no device call, so it also builds on its own under host sanitizers
// (tests/host/image_check.cpp, `make imagecheck`). It owns the error string every host file reports through.
#define PBN_HOST_NO_HIP
#include "pbn_host.hpp"

#include <cstdarg>
#include <cstdio>

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// A u64 threshold as the compact images store it: on the choice word, saturated ("never" passes only a = 2^32 - 1).
static uint32_t thr32_entry(uint64_t T) {
    const uint64_t t = u32_threshold(T);
    return t >> 32 ? 0xFFFFFFFFu : (uint32_t)t;
}

static uint64_t load64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

// Writes node i's compact threshold row (tp4 entries) from its u64 row (tp entries) and returns the
// number of thresholds below 2^32 on the choice word (a prefix: non-decreasing): the record a = 2^32 - 1 selects.
static uint32_t pack_thr32_row(const uint8_t* thr64, uint32_t tp, uint32_t tp4, uint8_t* row) {
    uint32_t m = 0;
    for (uint32_t q = 0; q < tp4; q++) {
        const uint64_t T = q < tp ? load64(thr64 + 8 * (size_t)q) : ~0ull;
        m += u32_threshold(T) >> 32 ? 0u : 1u;
        const uint32_t s = thr32_entry(T);
        memcpy(row + 4 * (size_t)q, &s, 4);
    }
    return m;
}

int build_predictor_image(const pbn_net_desc* d, pbn_net* n) {
    const int N = d->n_nodes, P = d->n_preds;
    CHECK_NN(d->pred_offsets, "pred_offsets");
    CHECK_NN(d->pred_inputs, "pred_inputs");
    CHECK_NN(d->pred_tt, "pred_tt");
    CHECK_NN(d->pred_thr, "pred_thr");
    if (P < 1 || P > 65535) return fail(PBN_E_UNSUPPORTED, "n_preds=%d outside [1, 65535]", P);
    if (d->pred_offsets[0] != 0 || d->pred_offsets[N] != P) return fail(PBN_E_INVALID, "pred_offsets must span [0, P]");
    for (int i = 0; i < N; i++) {
        int c = d->pred_offsets[i + 1] - d->pred_offsets[i];
        if (c < 1) return fail(PBN_E_INVALID, "node %d has no predictors (Predstep would fail, base.py:95-104)", i);
        for (int j = d->pred_offsets[i] + 1; j < d->pred_offsets[i + 1]; j++)
            if (d->pred_thr[j] < d->pred_thr[j - 1]) return fail(PBN_E_INVALID, "pred_thr not non-decreasing at node %d", i);
    }
    for (int j = 0; j < 3 * P; j++)
        if (d->pred_inputs[j] < 0 || d->pred_inputs[j] >= N)
            return fail(PBN_E_RANGE, "predictor input %d out of range [0, %d)", d->pred_inputs[j], N);
    uint32_t pmax = 1;
    for (int i = 0; i < N; i++) pmax = std::max(pmax, (uint32_t)(d->pred_offsets[i + 1] - d->pred_offsets[i]));
    NetLayout L{};
    L.tp = (pmax - 1 + 1) & ~1u;
    L.pmax = pmax;
    L.off_node = 0;
    L.off_thr = 0;
    L.off_rec = align16(8u * L.tp * (uint32_t)N);
    L.bytes = align16(L.off_rec + 8u * pmax * (uint32_t)N);
    L.kind = KIND_PREDICTOR_MIX;
    L.n_nodes = N;
    // the Philox kernels' compact LDS image (thr32_layout, pbn_params.hpp): their planes follow it
    const Thr32 X = thr32_layout(L);
    L.plane_off = std::max(L.bytes, X.bytes);
    if (L.plane_off > MAX_IMAGE)
        return fail(PBN_E_UNSUPPORTED, "network tables (%u B) exceed the LDS budget", L.plane_off);
    // the u64 image, then the compact one at L.bytes: u32 thresholds on the choice word, saturated; slot
    // tp4 of a node's record row holds the record a = 2^32 - 1 selects (its count of thresholds below
    // 2^32), which is where the saturated count lands
    n->image.assign((size_t)L.bytes + X.bytes, 0);
    uint8_t* im = n->image.data();
    uint8_t* cm = im + L.bytes;
    for (int i = 0; i < N; i++) {
        const int o0 = d->pred_offsets[i], c = d->pred_offsets[i + 1] - d->pred_offsets[i];
        uint8_t* thr64 = im + L.off_thr + 8 * ((size_t)i * L.tp);
        for (uint32_t q = 0; q < L.tp; q++) {
            // predictor j is skipped iff k53 >= thr[j]; thresholds past the last-but-one never are
            const uint64_t t = (int)q < c - 1 ? d->pred_thr[o0 + q] : ~0ull;
            memcpy(thr64 + 8 * (size_t)q, &t, 8);
        }
        uint8_t* rec64 = im + L.off_rec + 8 * ((size_t)i * pmax);
        for (int q = 0; q < c; q++) {
            const int j = o0 + q;
            uint64_t rec = (uint64_t)(uint32_t)d->pred_inputs[3 * j] |
                           ((uint64_t)(uint32_t)d->pred_inputs[3 * j + 1] << 16) |
                           ((uint64_t)(uint32_t)d->pred_inputs[3 * j + 2] << 32) | ((uint64_t)d->pred_tt[j] << 48);
            memcpy(rec64 + 8 * (size_t)q, &rec, 8);
        }
        const uint32_t m = pack_thr32_row(thr64, L.tp, X.tp4, cm + 4 * ((size_t)i * X.tp4));
        for (uint32_t q = 0; q < X.rs; q++) {
            const uint32_t src = q == X.tp4 ? m : q;
            if (src < pmax) memcpy(cm + X.rec_off + 8 * ((size_t)i * X.rs + q), rec64 + 8 * (size_t)src, 8);
        }
    }
    n->L = L;
    return 0;
}

int build_table_image(const pbn_net_desc* d, pbn_net* n) {
    const int N = d->n_nodes;
    CHECK_NN(d->node_k, "node_k");
    CHECK_NN(d->input_offsets, "input_offsets");
    CHECK_NN(d->thr_offsets, "thr_offsets");
    CHECK_NN(d->thr, "thr");
    if (N < 2) return fail(PBN_E_INVALID, "a PBN needs N >= 2 (node 0 is never updated, pbn.py:131)");
    int64_t sum_k = 0, sum_t = 0;
    for (int i = 0; i < N; i++)
        if (d->node_k[i] > 0 && !d->inputs) return fail(PBN_E_INVALID, "inputs is NULL");
    for (int i = 0; i < N; i++) {
        int k = d->node_k[i];
        if (k < 0 || k > 16) return fail(PBN_E_UNSUPPORTED, "node %d has %d inputs (max 16)", i, k);
        if (d->input_offsets[i] != sum_k) return fail(PBN_E_INVALID, "input_offsets inconsistent at node %d", i);
        if (d->thr_offsets[i] != sum_t) return fail(PBN_E_INVALID, "thr_offsets inconsistent at node %d", i);
        for (int q = 0; q < k; q++) {
            int in = d->inputs[sum_k + q];
            if (in < 0 || in >= N) return fail(PBN_E_RANGE, "input %d of node %d out of range", in, i);
        }
        sum_k += k;
        sum_t += (int64_t)1 << k;
        n->kmax = std::max(n->kmax, (int)k);
    }
    NetLayout L{};
    L.off_node = 0;
    L.off_rec = align16(8u * (uint32_t)N);
    uint64_t after_in = L.off_rec + 2u * (uint64_t)sum_k;
    if (after_in > MAX_IMAGE) return fail(PBN_E_UNSUPPORTED, "input lists exceed the LDS budget");
    L.off_thr = align16((uint32_t)after_in);
    uint64_t total = (uint64_t)L.off_thr + 8u * (uint64_t)sum_t;
    if (total > MAX_IMAGE) return fail(PBN_E_UNSUPPORTED, "probability tables (%llu B) exceed the LDS budget",
                                       (unsigned long long)total);
    L.bytes = align16((uint32_t)total);
    L.plane_off = L.bytes;
    L.kind = KIND_PROB_TABLE;
    L.n_nodes = N;
    n->image.assign(L.bytes, 0);
    uint8_t* im = n->image.data();
    for (int i = 0; i < N; i++) {
        uint64_t v = (uint64_t)(uint32_t)d->thr_offsets[i] | ((uint64_t)(uint32_t)d->input_offsets[i] << 32) |
                     ((uint64_t)(uint32_t)d->node_k[i] << 48);
        memcpy(im + L.off_node + 8 * i, &v, 8);
    }
    for (int64_t q = 0; q < sum_k; q++) {
        uint16_t v = (uint16_t)d->inputs[q];
        memcpy(im + L.off_rec + 2 * q, &v, 2);
    }
    memcpy(im + L.off_thr, d->thr, 8 * (size_t)sum_t);
    n->L = L;
    return 0;
}

// predictor_choice32 / predictor_record32 (pbn_device.hpp) on the host copy of the compact image
uint64_t net_select_u32(const pbn_net* n, int32_t node, uint32_t a) {
    const Thr32 X = thr32_layout(n->L);
    const uint8_t* cm = n->image.data() + n->L.bytes;
    uint32_t j = 0;
    for (uint32_t q = 0; q < X.tp4; q++) {
        uint32_t t;
        memcpy(&t, cm + 4 * ((size_t)node * X.tp4 + q), 4);
        j += a >= t ? 1u : 0u;
    }
    return load64(cm + X.rec_off + 8 * ((size_t)node * X.rs + j));
}

// The support graphs' edge rule (pbn_reach_rule.hpp, the definition k_unstable evaluates) on the host copy of
// the u64 image: masks [S][W], bit i set iff node i can flip at states [S][W]. graph: a truth-table network's
// PBN_TABLE_GRAPH_*; predictor mix has one graph.
static_assert((int)PBN_TABLE_GRAPH_STG == (int)TABLE_GRAPH_STG && (int)PBN_TABLE_GRAPH_STEP == (int)TABLE_GRAPH_STEP,
              "the ABI's graph codes are the rule header's");

void net_unstable(const pbn_net* n, int graph, const uint64_t* states, uint64_t n_states, uint64_t* masks) {
    const uint32_t N = (uint32_t)n->L.n_nodes, W = (uint32_t)n->W;
    const bool table = n->L.kind == KIND_PROB_TABLE;
    const uint32_t first = table ? table_graph_first_node(graph) : 0u;
    const uint8_t* im = n->image.data();
    for (uint64_t e = 0; e < n_states; e++) {
        const uint64_t* s = states + e * W;
        uint64_t* m = masks + e * W;
        auto bit = [s](uint32_t j) { return (uint32_t)(s[j >> 6] >> (j & 63u)) & 1u; };
        for (uint32_t k = 0; k < W; k++) m[k] = 0;
        for (uint32_t i = 0; i < N; i++) {
            const uint32_t f = table ? can_flip<KIND_PROB_TABLE>(bit, i, first, im, n->L)
                                     : can_flip<KIND_PREDICTOR_MIX>(bit, i, first, im, n->L);
            m[i >> 6] |= (uint64_t)f << (i & 63u);
        }
    }
}

// The law of the update (pbn_mass_rule.hpp, the definition k_stg_rows evaluates) on the host copy of the u64 image:
// mass [S][N], the edge mass of node i at states [S][W]. graph as for net_unstable.
void net_edge_mass(const pbn_net* n, int graph, const uint64_t* states, uint64_t n_states, uint64_t* mass) {
    const uint32_t N = (uint32_t)n->L.n_nodes, W = (uint32_t)n->W;
    const bool table = n->L.kind == KIND_PROB_TABLE;
    const uint32_t first = table ? table_graph_first_node(graph) : 0u;
    const uint8_t* im = n->image.data();
    for (uint64_t e = 0; e < n_states; e++) {
        const uint64_t* s = states + e * W;
        auto bit = [s](uint32_t j) { return (uint32_t)(s[j >> 6] >> (j & 63u)) & 1u; };
        for (uint32_t i = 0; i < N; i++)
            mass[e * N + i] = table ? edge_mass<KIND_PROB_TABLE>(bit, i, first, im, n->L)
                                    : edge_mass<KIND_PREDICTOR_MIX>(bit, i, first, im, n->L);
    }
}

// The env config's image: the network's u64 image, the attractor cubes, the target and the per-node
// counter deltas; `c` also takes the reset cubes and the scalars of `d`.
int build_envcfg_image(const pbn_net& net, const pbn_envcfg_desc* d, pbn_envcfg* c) {
    const int W = net.W;
    c->net = &net;
    c->W = W;
    c->H = d->n_cubes;
    c->H_reset = d->n_reset_cubes;
    c->L = net.L;
    c->off_cubes = net.L.bytes;
    c->off_target = align16(c->off_cubes + 16u * (uint32_t)W * (uint32_t)c->H);
    c->off_ndelta = align16(c->off_target + 16u * (uint32_t)W);
    uint32_t bytes = align16(c->off_ndelta + 8u * (uint32_t)net.N);
    if (bytes > MAX_IMAGE)
        return fail(PBN_E_UNSUPPORTED, "network + %d attractor cubes exceed the LDS budget", d->n_cubes);
    c->image.assign(bytes, 0);
    memcpy(c->image.data(), net.image.data(), net.L.bytes);  // not the compact image appended after it
    uint64_t* cubes = reinterpret_cast<uint64_t*>(c->image.data() + c->off_cubes);
    for (int h = 0; h < c->H; h++)
        for (int k = 0; k < W; k++) {
            uint64_t care = d->cube_care[(size_t)h * W + k];
            cubes[(size_t)h * 2 * W + k] = care;
            cubes[(size_t)h * 2 * W + W + k] = d->cube_value[(size_t)h * W + k] & care;
        }
    uint64_t* tgt = reinterpret_cast<uint64_t*>(c->image.data() + c->off_target);
    for (int k = 0; k < W; k++) {
        tgt[k] = d->target_care[k];
        tgt[W + k] = d->target_value[k] & d->target_care[k];
    }
    // Fast attractor test: one byte counter per cube (<= 8 cubes) holding the number of cared
    // bits where the state differs from the cube. Node i going 0 -> 1 adds +1 to the cubes
    // that want it 0 and -1 to those that want it 1; per node that is one packed delta
    // d = plus - minus per 32-bit half (bytes 0-3 = cubes 0-3, 4-7 = cubes 4-7). The
    // counters never leave [0, 255], so M += d (or M -= d for 1 -> 0) is exact word arithmetic.
    int max_care = 0;
    for (int h = 0; h < c->H; h++) {
        int pc = 0;
        for (int k = 0; k < W; k++) pc += __builtin_popcountll(d->cube_care[(size_t)h * W + k]);
        max_care = std::max(max_care, pc);
    }
    c->counters_ok = c->H <= 8 && max_care <= 255;
    uint32_t* nd = reinterpret_cast<uint32_t*>(c->image.data() + c->off_ndelta);
    for (int i = 0; i < net.N; i++) {
        uint32_t plus[2] = {0, 0}, minus[2] = {0, 0};
        for (int h = 0; h < c->H && h < 8; h++) {
            const uint64_t cw = d->cube_care[(size_t)h * W + i / 64], vw = d->cube_value[(size_t)h * W + i / 64];
            if (!((cw >> (i % 64)) & 1u)) continue;
            const uint32_t byte = 1u << (8 * (h & 3));
            if ((vw >> (i % 64)) & 1u)
                minus[h >> 2] |= byte;
            else
                plus[h >> 2] |= byte;
        }
        nd[2 * i] = plus[0] - minus[0];
        nd[2 * i + 1] = plus[1] - minus[1];
    }
    c->L.bytes = bytes;
    c->L.plane_off = bytes;
    const size_t rw = (size_t)c->H_reset * W;
    c->reset.resize(2 * rw);
    if (rw) {
        memcpy(c->reset.data(), d->reset_care, 8 * rw);
        memcpy(c->reset.data() + rw, d->reset_value, 8 * rw);
    }
    c->horizon = d->horizon;
    c->reward_success = d->reward_success;
    c->action_cost = d->action_cost;
    c->first_tested = d->first_update_tested ? 1 : 0;
    return 0;
}

// The LDS image of k_env's cooperative-draw modes (2 / 4), built on the host once per env config: the
// thresholds re-expressed on the draw word (u32, rows of tp4, saturated), the cubes / target / counter
// deltas moved up by erec_shift, and the 16-B env records (env_record_words, pbn_params.hpp) in rows of rs,
// slot tp4 holding the record a = 2^32 - 1 selects. The kernel used to build these itself from the u64
// image in its prologue (dependent global reads in every workgroup: ~8 us of a 63 us lone-env launch);
// now it stages them with plain 16-B copies. Same bytes as the kernel's construction (every R6 test).
std::vector<uint8_t> env_gen_image(const pbn_envcfg* cfg, uint32_t erec_shift) {
    const NetLayout& L = cfg->L;
    const Thr32 X = thr32_layout(L);
    const uint32_t N = (uint32_t)L.n_nodes;
    std::vector<uint8_t> g((size_t)L.bytes + erec_shift, 0);
    const uint8_t* im = cfg->image.data();
    memcpy(g.data() + cfg->off_cubes + erec_shift, im + cfg->off_cubes, L.bytes - cfg->off_cubes);
    const uint32_t nd_off = cfg->off_ndelta + erec_shift;
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t m = pack_thr32_row(im + L.off_thr + 8 * ((size_t)i * L.tp), L.tp, X.tp4,
                                          g.data() + 4 * ((size_t)i * X.tp4));
        for (uint32_t q = 0; q < X.rs; q++) {
            const uint32_t src = q == X.tp4 ? m : q;
            const uint64_t rec = src < L.pmax ? load64(im + L.off_rec + 8 * ((size_t)i * L.pmax + src)) : 0;
            const EnvRecord w = env_record_words(rec, i, nd_off);
            memcpy(g.data() + L.off_rec + 16 * ((size_t)i * X.rs + q), &w, 16);
        }
    }
    return g;
}
