// pbn_abi_env_set.cpp -- the until-attractor multi-flip env over an exact labelled state set (pbn_env_set_*): the entry
// points over the kernels of pbn_env_set.hip. DESIGN.md §14.
#include "pbn_host.hpp"

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
    if (int rc = check_set_for_batch(b, set, "the state set", PBN_E_INVALID)) return rc;
    if (!d_target_labels && (target_label < 0 || target_label > set->t.max_label))
        return fail(PBN_E_INVALID, "target_label=%d outside the set's labels [0, %d]", (int)target_label,
                    (int)set->t.max_label);
    if (b->net->kind == PBN_KIND_PROB_TABLE)
        if (int rc = check_two_nodes(b)) return rc;
    SET_DEV(b);
    int32_t* flag = nullptr;
    if (int rc = b->envset.err.get(b->stream, &flag)) return rc;
    void* kernel = env_set_kernel(b->W, b->net->kind);
    if (int rc = cached_bpc(b->envset.bpc, kernel, b->W, b->net->L.bytes)) return rc;
    EnvSetArgs a{};
    fill_lane_env(b, a);
    a.n_steps = b->d_nsteps;
    a.actions = d_actions;
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
    if (int rc = launch_lane_env_step(b, "k_env_set", kernel, a.L.bytes, b->envset.bpc, a)) return rc;
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
    int32_t* flag = nullptr;
    if (int rc = b->envset.err.get(b->stream, &flag)) return rc;
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
    int32_t err;
    if (int rc = b->envset.err.read_and_clear(b, &err)) return rc;
    if (err)
        return fail(PBN_E_RANGE, "Invalid action or source attractor: an env step or reset was skipped (envs holding "
                                 "one were left untouched)");
    return 0;
}

}  // extern "C"
