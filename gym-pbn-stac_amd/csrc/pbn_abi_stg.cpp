// pbn_abi_stg.cpp -- the exact transition graph of a state set (pbn_stg_*): the entry points over the mass rule of
// pbn_mass_rule.hpp, the state set of pbn_stateset.hpp and the kernel of pbn_stg.hip. DESIGN.md §16.
#include <cstdlib>

#include "pbn_host.hpp"

static_assert(PBN_STG_MAX_STATES == STATESET_MAX_STATES && PBN_STG_MAX_CELLS == STG_MAX_CELLS,
              "pbn_abi.h, pbn_stateset.hpp and pbn_params.hpp name the same caps");

extern "C" {

int pbn_stg_create(const pbn_net* net_c, int device, int32_t graph, const uint64_t* states, uint64_t n_states,
                   pbn_stg** out) {
    CHECK_NN(net_c, "net");
    CHECK_NN(out, "out");
    *out = nullptr;
    CHECK_NN(states, "states");
    pbn_net* net = const_cast<pbn_net*>(net_c);
    if (net->L.kind == KIND_PROB_TABLE && graph != PBN_TABLE_GRAPH_STG && graph != PBN_TABLE_GRAPH_STEP)
        return fail(PBN_E_INVALID, "graph=%d is neither PBN_TABLE_GRAPH_STG nor PBN_TABLE_GRAPH_STEP", (int)graph);
    if (n_states < 1 || n_states > PBN_STG_MAX_STATES)
        return fail(PBN_E_INVALID, "n_states=%llu outside [1, PBN_STG_MAX_STATES = %llu]", (unsigned long long)n_states,
                    (unsigned long long)PBN_STG_MAX_STATES);
    if (device < -1) return fail(PBN_E_RANGE, "device %d: a device index, or -1 for a host-only handle", device);
    // the kernel stages the whole image, as the edge-rule kernels of pbn_reach.hip do: one that does not fit is refused here
    if (net->L.bytes > REACH_LDS_MAX)
        return fail(PBN_E_UNSUPPORTED, "network image (%u B) exceeds the %u B of LDS the transition kernel stages it in",
                    net->L.bytes, REACH_LDS_MAX);
    pbn_stg* g = new pbn_stg;
    auto bail = [&](int code) {
        pbn_stg_destroy(g);
        return code;
    };
    g->net = net;
    g->W = net->W;
    g->graph = net->L.kind == KIND_PROB_TABLE ? graph : TABLE_GRAPH_NONE;
    g->n_states = n_states;
    std::vector<int32_t> labels((size_t)n_states);
    for (uint64_t r = 0; r < n_states; ++r) labels[(size_t)r] = (int32_t)r;
    uint64_t row = 0;
    switch (stateset_build(net->N, states, labels.data(), n_states, &g->t, &row)) {
        case STATESET_OK: break;
        case STATESET_E_STRAY_BITS:
            return bail(fail(PBN_E_INVALID, "state %llu has bits set beyond node %d", (unsigned long long)row, net->N - 1));
        case STATESET_E_CONFLICT:
            return bail(fail(PBN_E_INVALID, "state %llu repeats an earlier state: the rows of a graph are distinct",
                             (unsigned long long)row));
        default: return bail(fail(PBN_E_INVALID, "state set shape refused"));
    }
    if (device >= 0) {
        if (int rc = open_device(device)) return bail(rc);
        g->device = device;
        g->kernel = stg_rows_kernel(g->W, net->L.kind);
        if (!g->kernel) return bail(fail(PBN_E_UNSUPPORTED, "no transition kernel for %d state words", g->W));
        const size_t rb = 8 * (size_t)g->W * n_states, mb = 4 * (size_t)g->t.slots, kb = 8 * (size_t)g->W * g->t.slots;
        int rc = 0;
        if ((rc = g->rows.ensure(rb)) || (rc = g->meta.ensure(mb)) || (rc = g->keys.ensure(kb)) ||
            (rc = g->leaks.ensure(8)))
            return bail(rc);
        if (hipMemcpy(g->rows.p, states, rb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(g->meta.p, g->t.meta.data(), mb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(g->keys.p, g->t.keys.data(), kb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(g->leaks.p, 0, 8) != hipSuccess)
            return bail(fail(PBN_E_HIP, "transition graph upload failed"));
        g->d_image = net->image_on(device);
        if (!g->d_image) return bail(fail(PBN_E_NOMEM, "network image upload failed"));
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(fail(PBN_E_HIP, "hipGetDeviceProperties"));
        g->n_cu = prop.multiProcessorCount;
        if (int e = max_blocks_stg_rows(g->kernel, net->L.bytes, &g->bpc))
            return bail(fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)e)));
        if (const char* e = getenv("PBNSIM_STG_GRID")) g->grid_cap = std::max(atoi(e), 0);
    }
    *out = g;
    return 0;
}

void pbn_stg_destroy(pbn_stg* g) {
    if (!g) return;
    if (g->device >= 0) {
        (void)hipSetDevice(g->device);
        (void)hipStreamSynchronize(nullptr);  // a launch may still be writing the leak counter
    }
    delete g;  // the DevBufs give back the device copy
}

int pbn_stg_get_info(pbn_stg* g, pbn_stg_info* info) {
    CHECK_NN(g, "stg");
    CHECK_NN(info, "info");
    uint64_t leaks = 0;
    if (g->device >= 0) {
        SET_DEV(g);
        HIP_TRY(hipMemcpy(&leaks, g->leaks.p, 8, hipMemcpyDeviceToHost));  // waits for the launches before it
    }
    info->n_nodes = g->net->N;
    info->n_words = g->W;
    info->first_node = (int32_t)g->first_node();
    info->n_movable = g->net->N - (int32_t)g->first_node();
    info->device = g->device;
    info->table_graph = g->graph;
    info->n_states = g->n_states;
    info->leaks = leaks;
    return 0;
}

int pbn_stg_clear_leaks(pbn_stg* g) {
    CHECK_NN(g, "stg");
    if (g->device < 0) return 0;
    SET_DEV(g);
    HIP_TRY(hipMemsetAsync(g->leaks.p, 0, 8, nullptr));
    return 0;
}

int pbn_stg_rows_device(pbn_stg* g, uint64_t first_row, uint64_t n_rows, void* d_mass, void* d_succ) {
    CHECK_NN(g, "stg");
    // what the handle alone decides comes first, so that it is decided the same way with and without a device
    if (first_row > g->n_states || n_rows > g->n_states - first_row)
        return fail(PBN_E_RANGE, "rows [%llu, %llu + %llu) reach past the %llu states of the graph",
                    (unsigned long long)first_row, (unsigned long long)first_row, (unsigned long long)n_rows,
                    (unsigned long long)g->n_states);
    const uint64_t n_cells = n_rows * (uint64_t)g->net->N;
    if (n_cells > PBN_STG_MAX_CELLS)
        return fail(PBN_E_INVALID, "n_rows * n_nodes = %llu above PBN_STG_MAX_CELLS = %llu: ask for fewer rows per call",
                    (unsigned long long)n_cells, (unsigned long long)PBN_STG_MAX_CELLS);
    CHECK_NN(d_mass, "d_mass");
    CHECK_NN(d_succ, "d_succ");
    if (g->device < 0) return fail(PBN_E_STATE, "the transition graph is a host-only handle (created with device -1)");
    if (!n_rows) return 0;
    SET_DEV(g);
    StgArgs a{};
    a.img = g->d_image;
    a.L = g->net->L;
    a.first_node = g->first_node();
    a.states = (const uint64_t*)g->rows.p;
    a.set = SetView{(const uint32_t*)g->meta.p, (const uint64_t*)g->keys.p, g->t.slots};
    a.first_row = (uint32_t)first_row;
    a.n_cells = n_cells;
    a.mass = (unsigned long long*)d_mass;
    a.succ = (int32_t*)d_succ;
    a.leaks = (unsigned long long*)g->leaks.p;
    // what is resident: a workgroup stages the image once and walks the cells with a grid stride
    int grid = resident_grid(n_cells, g->n_cu, g->bpc, BLOCK);
    if (g->grid_cap > 0) grid = std::min(grid, g->grid_cap);
    if (int e = launch_stg_rows(g->kernel, a, grid, nullptr))
        return fail(PBN_E_HIP, "k_stg_rows launch: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

}  // extern "C"
