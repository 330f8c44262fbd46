// pbn_abi_flipset.cpp -- the max over multi-flip action sets: the entry points over the kernels of pbn_flipset.hip and
// the graph handle of pbn_abi_stg.cpp. DESIGN.md §19.
#include <cmath>

#include "pbn_control_plan.hpp"
#include "pbn_host.hpp"

namespace {

enum { FLIPSET_LEVEL = 0, FLIPSET_SELECT = 1 };

// The kernel of slot `which` for this graph's shape and its resident workgroups per CU, asked once per handle.
int flipset_kernel(pbn_stg* g, int which, pbn_stg::Ctl** out) {
    pbn_stg::Ctl& c = g->flipset[which];
    if (!c.kernel) {
        const uint32_t G = control_group((uint32_t)g->net->N);
        c.kernel = which == FLIPSET_LEVEL ? stg_flipset_kernel(G, (uint32_t)g->net->N <= G) : stg_flipset_select_kernel();
        if (!c.kernel) return fail(PBN_E_UNSUPPORTED, "no flip-set kernel for %d nodes", g->net->N);
    }
    if (!c.bpc)
        if (int e = max_blocks_control(c.kernel, &c.bpc))
            return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)e));
    *out = &c;
    return 0;
}

int check_cost(double cost, const char* name) {
    if (!(cost >= 0.0) || std::isinf(cost)) return fail(PBN_E_INVALID, "%s=%g is not a finite cost >= 0", name, cost);
    return 0;
}

}  // namespace

extern "C" {

int pbn_stg_flipset_level_device(pbn_stg* g, const void* d_nbr, const double* d_m, double cost, const double* d_in_base,
                                 const int32_t* d_in_tag, double* d_out_base, int32_t* d_out_tag) {
    CHECK_NN(g, "stg");
    CHECK_NN(d_nbr, "d_nbr");
    CHECK_NN(d_out_base, "d_out_base");
    CHECK_NN(d_out_tag, "d_out_tag");
    if (!d_in_base != !d_in_tag) return fail(PBN_E_INVALID, "d_in_base and d_in_tag: both, or both NULL (level 0 -> 1 from d_m)");
    if (!d_in_base) CHECK_NN(d_m, "d_m");
    if (int rc = check_cost(cost, "cost")) return rc;
    if (d_in_base == d_out_base || d_in_tag == d_out_tag)
        return fail(PBN_E_INVALID, "the output summary aliases the input: a level reads rows it has not yet written");
    if (g->device < 0) return fail(PBN_E_STATE, "the transition graph is a host-only handle (created with device -1)");
    SET_DEV(g);
    pbn_stg::Ctl* c = nullptr;
    if (int rc = flipset_kernel(g, FLIPSET_LEVEL, &c)) return rc;
    const ControlPlan p = control_plan(g->n_states, (uint32_t)g->net->N, g->n_cu, c->bpc, g->grid_cap);
    StgFlipsetArgs a{};
    a.nbr = (const int32_t*)d_nbr;
    a.m = d_m;
    a.in_base = d_in_base;
    a.in_tag = d_in_tag;
    a.out_base = d_out_base;
    a.out_tag = d_out_tag;
    a.cost = cost;
    a.n_states = g->n_states;
    a.n_nodes = (uint32_t)g->net->N;
    if (int e = launch_control(c->kernel, p.grid, nullptr, &a))
        return fail(PBN_E_HIP, "k_stg_flipset launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

int pbn_stg_flipset_select_device(pbn_stg* g, const double* d_base, const int32_t* d_tag, const double* d_m, double cost,
                                  const double* noop_cost, double* d_v, int32_t* d_policy_end, int32_t* d_policy_flips) {
    CHECK_NN(g, "stg");
    CHECK_NN(d_base, "d_base");
    CHECK_NN(d_tag, "d_tag");
    CHECK_NN(d_m, "d_m");
    CHECK_NN(d_v, "d_v");
    CHECK_NN(d_policy_end, "d_policy_end");
    CHECK_NN(d_policy_flips, "d_policy_flips");
    if (int rc = check_cost(cost, "cost")) return rc;
    if (noop_cost)
        if (int rc = check_cost(*noop_cost, "noop_cost")) return rc;
    if (g->device < 0) return fail(PBN_E_STATE, "the transition graph is a host-only handle (created with device -1)");
    SET_DEV(g);
    pbn_stg::Ctl* c = nullptr;
    if (int rc = flipset_kernel(g, FLIPSET_SELECT, &c)) return rc;
    StgFlipsetSelectArgs a{};
    a.base = d_base;
    a.tag = d_tag;
    a.m = d_m;
    a.cost = cost;
    a.noop_cost = noop_cost ? *noop_cost : 0.0;
    a.has_noop = noop_cost ? 1u : 0u;
    a.n_states = g->n_states;
    a.v = d_v;
    a.policy_end = d_policy_end;
    a.policy_flips = d_policy_flips;
    int grid = resident_grid(g->n_states, g->n_cu, c->bpc, BLOCK);
    if (g->grid_cap > 0) grid = std::min(grid, g->grid_cap);
    if (int e = launch_control(c->kernel, grid, nullptr, &a))
        return fail(PBN_E_HIP, "k_stg_flipset_select launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

}  // extern "C"
