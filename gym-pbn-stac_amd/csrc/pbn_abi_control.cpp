// pbn_abi_control.cpp -- exact optimal control over a transition graph: the entry points over the kernels of
// pbn_control.hip and the graph handle of pbn_abi_stg.cpp. DESIGN.md §17.
#include "pbn_control_plan.hpp"
#include "pbn_host.hpp"

namespace {

// The kernel of slot `which` for this graph's shape and its resident workgroups per CU, asked once per handle.
int control_kernel(pbn_stg* g, int which, pbn_stg::Ctl** out) {
    pbn_stg::Ctl& c = g->ctl[which];
    if (!c.kernel) {
        const uint32_t G = control_group((uint32_t)g->net->N);
        const bool one_cell = (uint32_t)g->net->N <= G;
        c.kernel = which == pbn_stg::CTL_FLIP     ? stg_flip_rows_kernel(g->W)
                   : which == pbn_stg::CTL_EXPECT ? stg_expect_kernel(G, one_cell)
                                                  : stg_backup_kernel(G, one_cell);
        if (!c.kernel) return fail(PBN_E_UNSUPPORTED, "no control kernel for %d nodes in %d words", g->net->N, g->W);
    }
    if (!c.bpc)
        if (int e = max_blocks_control(c.kernel, &c.bpc))
            return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)e));
    *out = &c;
    return 0;
}

// One launch of a reducing kernel over all rows of the graph, in the shape of pbn_control_plan.hpp.
int launch_rows(pbn_stg* g, int which, const char* name, void* args) {
    pbn_stg::Ctl* c = nullptr;
    if (int rc = control_kernel(g, which, &c)) return rc;
    const ControlPlan p = control_plan(g->n_states, (uint32_t)g->net->N, g->n_cu, c->bpc, g->grid_cap);
    if (int e = launch_control(c->kernel, p.grid, nullptr, args))
        return fail(PBN_E_HIP, "%s launch: %s", name, hipGetErrorString((hipError_t)e));
    return 0;
}

int host_only(const pbn_stg* g) {
    if (g->device < 0) return fail(PBN_E_STATE, "the transition graph is a host-only handle (created with device -1)");
    return 0;
}

}  // namespace

extern "C" {

int pbn_stg_flip_rows_device(pbn_stg* g, uint64_t first_row, uint64_t n_rows, const uint64_t* action_mask, void* d_nbr) {
    CHECK_NN(g, "stg");
    if (first_row > g->n_states || n_rows > g->n_states - first_row)
        return fail(PBN_E_RANGE, "rows [%llu, %llu + %llu) reach past the %llu states of the graph",
                    (unsigned long long)first_row, (unsigned long long)first_row, (unsigned long long)n_rows,
                    (unsigned long long)g->n_states);
    const int N = g->net->N;
    StgFlipArgs a{};
    for (int k = 0; k < g->W; ++k) {
        const uint64_t full = k == g->W - 1 && (N & 63) ? (1ull << (N & 63)) - 1ull : ~0ull;
        a.allowed[k] = action_mask ? action_mask[k] : full;
        if (a.allowed[k] & ~full) return fail(PBN_E_INVALID, "action_mask has bits set beyond node %d", N - 1);
    }
    CHECK_NN(d_nbr, "d_nbr");
    if (int rc = host_only(g)) return rc;
    if (!n_rows) return 0;
    SET_DEV(g);
    pbn_stg::Ctl* c = nullptr;
    if (int rc = control_kernel(g, pbn_stg::CTL_FLIP, &c)) return rc;
    a.states = (const uint64_t*)g->rows.p;
    a.set = g->view();
    a.first_row = first_row;
    a.n_cells = n_rows * (uint64_t)N;
    a.n_nodes = (uint32_t)N;
    a.nbr = (int32_t*)d_nbr;
    int grid = resident_grid(a.n_cells, g->n_cu, c->bpc, BLOCK);
    if (g->grid_cap > 0) grid = std::min(grid, g->grid_cap);
    if (int e = launch_control(c->kernel, grid, nullptr, &a))
        return fail(PBN_E_HIP, "k_stg_flip_rows launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

int pbn_stg_expect_device(pbn_stg* g, const void* d_mass, const void* d_succ, const double* d_v, double* d_out,
                          const double* d_pen, double cost, double* d_out_pen) {
    CHECK_NN(g, "stg");
    CHECK_NN(d_mass, "d_mass");
    CHECK_NN(d_succ, "d_succ");
    CHECK_NN(d_v, "d_v");
    CHECK_NN(d_out, "d_out");
    if (d_pen) CHECK_NN(d_out_pen, "d_out_pen");
    if (int rc = host_only(g)) return rc;
    SET_DEV(g);
    StgExpectArgs a{};
    a.mass = (const unsigned long long*)d_mass;
    a.succ = (const int32_t*)d_succ;
    a.v = d_v;
    a.out = d_out;
    a.pen = d_pen;
    a.cost = cost;
    a.out_pen = d_out_pen;
    a.n_states = g->n_states;
    a.n_nodes = (uint32_t)g->net->N;
    a.n_movable = (double)(g->net->N - (int)g->first_node());
    return launch_rows(g, pbn_stg::CTL_EXPECT, "k_stg_expect", &a);
}

int pbn_stg_backup_device(pbn_stg* g, const void* d_nbr, const double* d_u, const double* d_ua, double* d_v,
                          int32_t* d_policy) {
    CHECK_NN(g, "stg");
    CHECK_NN(d_nbr, "d_nbr");
    CHECK_NN(d_u, "d_u");
    CHECK_NN(d_ua, "d_ua");
    CHECK_NN(d_v, "d_v");
    CHECK_NN(d_policy, "d_policy");
    if (int rc = host_only(g)) return rc;
    SET_DEV(g);
    StgBackupArgs a{};
    a.nbr = (const int32_t*)d_nbr;
    a.u = d_u;
    a.ua = d_ua;
    a.v = d_v;
    a.policy = d_policy;
    a.n_states = g->n_states;
    a.n_nodes = (uint32_t)g->net->N;
    return launch_rows(g, pbn_stg::CTL_BACKUP, "k_stg_backup", &a);
}

int pbn_stg_lookup_device(pbn_stg* g, const void* d_words, uint64_t n, int32_t* d_rows) {
    CHECK_NN(g, "stg");
    CHECK_NN(d_words, "d_words");
    CHECK_NN(d_rows, "d_rows");
    if (n > PBN_STG_LOOKUP_MAX)
        return fail(PBN_E_RANGE, "n=%llu above PBN_STG_LOOKUP_MAX = %llu: ask in parts", (unsigned long long)n,
                    (unsigned long long)PBN_STG_LOOKUP_MAX);
    if (int rc = host_only(g)) return rc;
    if (!n) return 0;
    SET_DEV(g);
    // k_set_lookup (pbn_tenv.hip) over the graph's own table: the label of a row is its index
    SetLookupArgs a{(const uint64_t*)d_words, g->view(), n, d_rows};
    if (int e = launch_set_lookup(g->W, a, nullptr))
        return fail(PBN_E_HIP, "k_set_lookup launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

}  // extern "C"
