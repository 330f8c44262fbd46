// pbn_abi_env_set.cpp -- the until-attractor multi-flip env over an exact labelled state set (pbn_env_set_*): the entry
// points over the kernels of pbn_env_set.hip. DESIGN.md §14.
#include "pbn_host.hpp"

// The sticky flag of k_env_set / k_env_set_reset: zeroed at allocation and after every pbn_env_set_check.
static int env_set_error_flag(pbn_batch* b, int32_t** flag) {
    if (!b->envset.err.p) {
        if (int rc = b->envset.err.ensure(4)) return rc;
        HIP_TRY(hipMemsetAsync(b->envset.err.p, 0, 4, b->stream));
    }
    *flag = (int32_t*)b->envset.err.p;
    return 0;
}

extern "C" {

int pbn_stateset_get_hull(const pbn_stateset* s, uint64_t* all_words, uint64_t* any_words, int32_t* max_label) {
    CHECK_NN(s, "stateset");
    if (all_words) memcpy(all_words, s->t.hull_all.data(), 8 * (size_t)s->t.W);
    if (any_words) memcpy(any_words, s->t.hull_any.data(), 8 * (size_t)s->t.W);
    if (max_label) *max_label = s->t.max_label;
    return 0;
}

int pbn_env_set_step_device(pbn_batch* b, const pbn_stateset* set, const int32_t* d_actions, int A, int dedup,
                            int offset, uint32_t update_cap, int32_t horizon, int32_t reward_success,
                            int32_t action_cost, int first_update_tested, int32_t target_label,
                            const int32_t* d_target_labels, uint64_t* d_obs, int32_t* d_reward, uint8_t* d_flags,
                            uint32_t* d_n_updates, int32_t* d_labels) {
    CHECK_NN(b, "batch");
    CHECK_NN(set, "set");
    CHECK_NN(d_actions, "d_actions");
    CHECK_NN(d_obs, "d_obs");
    CHECK_NN(d_reward, "d_reward");
    CHECK_NN(d_flags, "d_flags");
    CHECK_NN(d_n_updates, "d_n_updates");
    if (int rc = check_action_shape(A, offset)) return rc;
    if (set->device < 0) return fail(PBN_E_INVALID, "the state set is host-only (created with device -1)");
    if (set->device != b->device)
        return fail(PBN_E_INVALID, "the state set lives on device %d, the batch on device %d", set->device, b->device);
    if (set->t.n_nodes != b->N)
        return fail(PBN_E_INVALID, "the state set holds states of %d nodes, the batch has %d", set->t.n_nodes, b->N);
    if (!d_target_labels && (target_label < 0 || target_label > set->t.max_label))
        return fail(PBN_E_INVALID, "target_label=%d outside the set's labels [0, %d]", (int)target_label,
                    (int)set->t.max_label);
    if (b->net->kind == PBN_KIND_PROB_TABLE && b->N < 2)
        return fail(PBN_E_UNSUPPORTED, "PBN.step updates a node in [1, N-1]: the network needs two nodes");
    SET_DEV(b);
    int32_t* flag;
    if (int rc = env_set_error_flag(b, &flag)) return rc;
    if (!b->envset.bpc)
        if (int e = max_blocks_env_set(b->W, b->net->kind, b->net->L.bytes, &b->envset.bpc))
            return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)e));
    EnvSetArgs a{};
    a.state = b->d_state;
    a.n_steps = b->d_nsteps;
    a.actions = d_actions;
    a.img = b->d_image;
    a.L = b->net->L;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.call_idx = b->r6.calls;
    a.update_cap = update_cap;
    a.A = A;
    a.offset = offset;
    a.dedup = dedup ? 1 : 0;
    a.horizon = horizon;
    a.reward_success = reward_success;
    a.action_cost = action_cost;
    a.first_tested = first_update_tested ? 1 : 0;
    a.set = set->view();
    for (int k = 0; k < b->W; ++k) {
        // without the pre-filter: all = any = 0 would reject; all = ~0, any = 0 cares about no node
        a.hull_all[k] = b->knob.envset_no_hull ? ~0ull : set->t.hull_all[k];
        a.hull_any[k] = b->knob.envset_no_hull ? 0ull : set->t.hull_any[k];
    }
    a.always_lookup = b->knob.envset_no_skip ? 1 : 0;
    a.target_label = target_label;
    a.target_labels = d_target_labels;
    a.obs = d_obs;
    a.reward = d_reward;
    a.flags = d_flags;
    a.n_updates = d_n_updates;
    a.labels = d_labels;
    a.error = flag;
    int grid = b->grid_for(b->B, b->envset.bpc);
    if (b->knob.envset_grid > 0) grid = std::min(grid, b->knob.envset_grid);
    if (int rc = timed_launch(b, "k_env_set", [&] { return launch_env_set(b->W, a, grid, b->stream); })) return rc;
    b->r6.calls++;  // as pbn_env_step_multi_device: one env step launched
    return 0;
}

int pbn_env_set_reset_device(pbn_batch* b, const uint64_t* d_rows, const uint32_t* d_row_off, int32_t n_labels,
                             int32_t source_label, const int32_t* d_source_labels, const uint8_t* d_mask) {
    CHECK_NN(b, "batch");
    CHECK_NN(d_rows, "d_rows");
    CHECK_NN(d_row_off, "d_row_off");
    if (n_labels < 1) return fail(PBN_E_INVALID, "n_labels=%d: at least one attractor", (int)n_labels);
    SET_DEV(b);
    int32_t* flag;
    if (int rc = env_set_error_flag(b, &flag)) return rc;
    EnvSetResetArgs a{};
    a.state = b->d_state;
    a.n_steps = b->d_nsteps;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.reset_count = b->reset_count;
    a.rows = d_rows;
    a.row_off = d_row_off;
    a.n_labels = n_labels;
    a.source_label = source_label;
    a.source_labels = d_source_labels;
    a.mask = d_mask;
    a.clear_node0 = b->net->kind == PBN_KIND_PROB_TABLE ? 1 : 0;
    a.error = flag;
    if (int rc = timed_launch(b, "k_env_set_reset", [&] { return launch_env_set_reset(b->W, a, b->stream); })) return rc;
    b->reset_count++;
    return 0;
}

int pbn_env_set_check(pbn_batch* b) {
    CHECK_NN(b, "batch");
    SET_DEV(b);
    int32_t* flag;
    if (int rc = env_set_error_flag(b, &flag)) return rc;
    if (!b->pin.ready()) return fail(PBN_E_NOMEM, "pinned staging buffer");
    HIP_TRY(hipMemcpyAsync(b->pin.p, flag, 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemsetAsync(flag, 0, 4, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    int32_t err;
    memcpy(&err, b->pin.p, 4);
    if (err)
        return fail(PBN_E_RANGE, "Invalid action or source attractor: an env step or reset was skipped (envs holding "
                                 "one were left untouched)");
    return 0;
}

}  // extern "C"
