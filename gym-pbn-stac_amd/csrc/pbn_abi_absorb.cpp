// pbn_abi_absorb.cpp -- absorption over a transition graph: the entry point over k_stg_absorb (pbn_absorb.hip) and the
// graph handle of pbn_abi_stg.cpp. DESIGN.md §18.
#include "pbn_absorb_plan.hpp"
#include "pbn_host.hpp"

namespace {

// The kernel for this graph's shape and a column tile, and its resident workgroups per CU, asked once per handle.
int absorb_kernel(pbn_stg* g, const AbsorbPlan& shape, pbn_stg::Ctl** out) {
    const int slot = shape.col_tile == 1 ? 0 : shape.col_tile == 2 ? 1 : shape.col_tile == 4 ? 2 : 3;
    pbn_stg::Ctl& c = g->absorb[slot];
    if (!c.kernel) {
        c.kernel = stg_absorb_kernel(shape.G, shape.cells_per_lane == 1, shape.col_tile);
        if (!c.kernel)
            return fail(PBN_E_UNSUPPORTED, "no absorb kernel for %d nodes and a tile of %u columns", g->net->N, shape.col_tile);
    }
    if (!c.bpc)
        if (int e = max_blocks_control(c.kernel, &c.bpc))
            return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)e));
    *out = &c;
    return 0;
}

}  // namespace

extern "C" {

int pbn_stg_absorb_device(pbn_stg* g, const void* d_mass, const void* d_succ, const int32_t* d_label, const double* d_x,
                          double* d_out, uint32_t n_cols, uint64_t ld, const double* src) {
    CHECK_NN(g, "stg");
    CHECK_NN(d_mass, "d_mass");
    CHECK_NN(d_succ, "d_succ");
    CHECK_NN(d_label, "d_label");
    CHECK_NN(d_x, "d_x");
    CHECK_NN(d_out, "d_out");
    if (n_cols < 1 || n_cols > PBN_STG_ABSORB_MAX_COLS)
        return fail(PBN_E_INVALID, "n_cols=%u outside [1, %d]", n_cols, PBN_STG_ABSORB_MAX_COLS);
    if (ld < n_cols)
        return fail(PBN_E_INVALID, "ld=%llu below n_cols=%u", (unsigned long long)ld, n_cols);
    if (d_out == d_x) return fail(PBN_E_INVALID, "d_out aliases d_x: a Jacobi sweep reads rows it has not yet written");
    if (g->device < 0) return fail(PBN_E_STATE, "the transition graph is a host-only handle (created with device -1)");
    SET_DEV(g);
    const uint32_t N = (uint32_t)g->net->N;
    pbn_stg::Ctl* c = nullptr;
    // the shape first (it names the kernel), then the grid from that kernel's occupancy
    if (int rc = absorb_kernel(g, absorb_plan(g->n_states, N, n_cols, g->n_cu, 1, g->grid_cap), &c)) return rc;
    const AbsorbPlan p = absorb_plan(g->n_states, N, n_cols, g->n_cu, c->bpc, g->grid_cap);
    StgAbsorbArgs a{};
    a.mass = (const unsigned long long*)d_mass;
    a.succ = (const int32_t*)d_succ;
    a.label = d_label;
    a.x = d_x;
    a.out = d_out;
    a.ld = ld;
    a.n_states = g->n_states;
    a.n_nodes = N;
    a.n_cols = n_cols;
    a.n_movable = (double)(g->net->N - (int)g->first_node());
    for (uint32_t k = 0; k < n_cols; ++k) a.src.b[k] = src ? src[k] : 0.0;
    if (int e = launch_control(c->kernel, p.grid, nullptr, &a))
        return fail(PBN_E_HIP, "k_stg_absorb launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

}  // extern "C"
