// pbn_abi_tenv.cpp -- exact state sets (pbn_stateset_*), the PBN-v0 env and the macro-action envs on the device
// (pbn_tenv_*): the entry points over pbn_stateset.hpp (the set's one definition) and the kernels of pbn_tenv.hip
// and pbn_tenv_macro.hip (the reset: k_env_set_reset, pbn_env_set.hip).
#include "pbn_host.hpp"

static_assert((int)PBN_MACRO_INTERVAL == (int)TENV_MACRO_INTERVAL && (int)PBN_MACRO_TRIGGER == (int)TENV_MACRO_TRIGGER &&
                  PBN_TENV_MACRO_MAX_T == TENV_MACRO_MAX_T,
              "pbn_abi.h and pbn_params.hpp name the same modes and cap");

static int check_table_batch(const pbn_batch* b, const char* fn) {
    if (b->net->kind != PBN_KIND_PROB_TABLE)
        return fail(PBN_E_UNSUPPORTED, "%s steps the PBN-v0 env of a truth-table network; this batch holds a "
                                       "predictor-mix network (its env is pbn_env_step_multi)", fn);
    return 0;
}

extern "C" {

int pbn_stateset_create(int32_t n_nodes, int device, const uint64_t* states, const int32_t* labels, uint64_t n_states,
                        pbn_stateset** out) {
    CHECK_NN(out, "out");
    *out = nullptr;
    if (n_states && !states) return fail(PBN_E_INVALID, "states is NULL");
    if (n_nodes < 1 || n_nodes > 64 * MAX_WORDS)
        return fail(PBN_E_INVALID, "n_nodes=%d outside [1, %d]", (int)n_nodes, 64 * MAX_WORDS);
    if (n_states > PBN_STATESET_MAX_STATES)
        return fail(PBN_E_INVALID, "n_states=%llu above PBN_STATESET_MAX_STATES (%llu)", (unsigned long long)n_states,
                    (unsigned long long)PBN_STATESET_MAX_STATES);
    if (device < -1) return fail(PBN_E_RANGE, "device %d: a device index, or -1 for a host-only set", device);
    pbn_stateset* s = new pbn_stateset;
    uint64_t row = 0;
    switch (stateset_build(n_nodes, states, labels, n_states, &s->t, &row)) {
        case STATESET_OK: break;
        case STATESET_E_STRAY_BITS:
            delete s;
            return fail(PBN_E_INVALID, "state %llu has bits set beyond node %d", (unsigned long long)row, n_nodes - 1);
        case STATESET_E_LABEL:
            delete s;
            return fail(PBN_E_INVALID, "state %llu has a negative label", (unsigned long long)row);
        case STATESET_E_CONFLICT:
            delete s;
            return fail(PBN_E_INVALID, "state %llu repeats an earlier state under a different label",
                        (unsigned long long)row);
        default:
            delete s;
            return fail(PBN_E_INVALID, "state set shape refused");
    }
    if (device >= 0) {
        auto bail = [&](int code) {
            pbn_stateset_destroy(s);
            return code;
        };
        if (int rc = open_device(device)) {
            delete s;
            return rc;
        }
        s->device = device;
        const size_t mb = 4 * (size_t)s->t.slots, kb = 8 * (size_t)s->t.W * s->t.slots;
        if (int rc = s->meta.ensure(mb)) return bail(rc);
        if (int rc = s->keys.ensure(kb)) return bail(rc);
        if (hipMemcpy(s->meta.p, s->t.meta.data(), mb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(s->keys.p, s->t.keys.data(), kb, hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(PBN_E_HIP, "state set upload failed"));
    }
    *out = s;
    return 0;
}

void pbn_stateset_destroy(pbn_stateset* s) {
    if (!s) return;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    delete s;  // the DevBufs give back the device copy
}

int pbn_stateset_get_info(const pbn_stateset* s, pbn_stateset_info* info) {
    CHECK_NN(s, "stateset");
    CHECK_NN(info, "info");
    info->n_nodes = s->t.n_nodes;
    info->n_words = s->t.W;
    info->device = s->device;
    info->n_states = s->t.n_states;
    info->table_slots = s->t.slots;
    info->max_probe = s->t.max_probe;
    return 0;
}

int pbn_stateset_lookup(const pbn_stateset* s, const uint64_t* states, uint64_t n, int32_t* labels) {
    CHECK_NN(s, "stateset");
    if (!n) return 0;
    CHECK_NN(states, "states");
    CHECK_NN(labels, "labels");
    stateset_lookup_host(s->t, states, n, labels);
    return 0;
}

int pbn_stateset_lookup_device(pbn_batch* b, const pbn_stateset* s, const void* d_words, int32_t* d_labels) {
    CHECK_NN(b, "batch");
    CHECK_NN(s, "stateset");
    CHECK_NN(d_labels, "d_labels");
    if (int rc = check_set_for_batch(b, s, "the state set", PBN_E_STATE)) return rc;
    SET_DEV(b);
    SetLookupArgs a{d_words ? (const uint64_t*)d_words : b->d_state, s->view(), b->B, d_labels};
    return timed_launch(b, "k_set_lookup", [&] { return launch_set_lookup(b->W, a, b->stream); });
}

int pbn_tenv_step_device(pbn_batch* b, const pbn_stateset* target, const int32_t* d_actions, int32_t reward_target,
                         int32_t step_cost, int32_t action_cost, int check, uint64_t* d_obs, int32_t* d_reward,
                         uint8_t* d_flags, int32_t* d_labels) {
    CHECK_NN(b, "batch");
    CHECK_NN(target, "target");
    CHECK_NN(d_actions, "d_actions");
    CHECK_NN(d_reward, "d_reward");
    CHECK_NN(d_flags, "d_flags");
    if (int rc = check_table_batch(b, "pbn_tenv_step_device")) return rc;
    if (int rc = check_set_for_batch(b, target, "the target set", PBN_E_STATE)) return rc;
    if (int rc = check_two_nodes(b)) return rc;
    SET_DEV(b);
    int32_t* flag = nullptr;
    if (int rc = b->tenv.err.get(b->stream, &flag)) return rc;
    void* kernel = tenv_step_kernel(b->W);
    if (int rc = cached_bpc(b->tenv.bpc, kernel, b->W, b->net->L.plane_off)) return rc;
    TenvArgs a{};
    fill_lane_env(b, a);
    a.update = b->update_count;
    a.actions = d_actions;
    a.target = target->view();
    a.reward_target = reward_target;
    a.step_cost = step_cost;
    a.action_cost = action_cost;
    a.obs = d_obs;
    a.reward = d_reward;
    a.flags = d_flags;
    a.labels = d_labels;
    a.error = flag;
    if (int rc = launch_lane_env_step(b, "k_tenv_step", kernel, a.L.plane_off, b->tenv.bpc, a)) return rc;
    b->update_count++;  // the launch happened: the count advances whether or not an action was refused
    if (!check) return 0;
    int32_t err;
    if (int rc = b->tenv.err.read_and_clear(b, &err)) return rc;
    if (err) return fail(PBN_E_RANGE, "Invalid action: a value outside [0, %d] (envs holding one were left untouched)", b->N - 1);
    return 0;
}

int pbn_tenv_macro_device(pbn_batch* b, const pbn_stateset* target, int mode, uint32_t t_max, const int32_t* d_actions,
                          const int32_t* d_limit, const double* d_gpow, const uint64_t* d_stop_thr,
                          int32_t reward_target, int32_t step_cost, int32_t action_cost, int check, uint64_t* d_obs,
                          int32_t* d_reward_i32, double* d_reward_f64, uint8_t* d_flags, int32_t* d_interval,
                          int32_t* d_first_hit, int32_t* d_labels) {
    CHECK_NN(b, "batch");
    CHECK_NN(target, "target");
    CHECK_NN(d_actions, "d_actions");
    CHECK_NN(d_limit, "d_limit");
    CHECK_NN(d_flags, "d_flags");
    if (mode != PBN_MACRO_INTERVAL && mode != PBN_MACRO_TRIGGER)
        return fail(PBN_E_INVALID, "mode=%d: PBN_MACRO_INTERVAL (%d) or PBN_MACRO_TRIGGER (%d)", mode,
                    (int)PBN_MACRO_INTERVAL, (int)PBN_MACRO_TRIGGER);
    if (mode == PBN_MACRO_INTERVAL) {
        CHECK_NN(d_reward_i32, "d_reward_i32");
    } else {
        CHECK_NN(d_reward_f64, "d_reward_f64");
        CHECK_NN(d_gpow, "d_gpow");
        CHECK_NN(d_stop_thr, "d_stop_thr");
    }
    if (t_max < 1 || t_max > PBN_TENV_MACRO_MAX_T)
        return fail(PBN_E_INVALID, "t_max=%u outside [1, PBN_TENV_MACRO_MAX_T = %u]", (unsigned)t_max,
                    (unsigned)PBN_TENV_MACRO_MAX_T);
    if (int rc = check_table_batch(b, "pbn_tenv_macro_device")) return rc;
    if (int rc = check_set_for_batch(b, target, "the target set", PBN_E_STATE)) return rc;
    if (int rc = check_two_nodes(b)) return rc;
    SET_DEV(b);
    int32_t* flag = nullptr;
    if (int rc = b->tenv.err.get(b->stream, &flag)) return rc;
    void* kernel = tenv_macro_kernel(b->W, mode);
    int& bpc = b->tenv.macro_bpc[mode];
    if (int rc = cached_bpc(bpc, kernel, b->W, b->net->L.plane_off)) return rc;
    TenvMacroArgs a{};
    fill_lane_env(b, a);
    a.update = b->update_count;
    a.actions = d_actions;
    a.limit = d_limit;
    a.target = target->view();
    a.reward_target = reward_target;
    a.step_cost = step_cost;
    a.action_cost = action_cost;
    a.mode = mode;
    a.t_max = t_max;
    a.gpow = d_gpow;
    a.stop_thr = d_stop_thr;
    a.obs = d_obs;
    a.reward_i32 = d_reward_i32;
    a.reward_f64 = d_reward_f64;
    a.flags = d_flags;
    a.interval = d_interval;
    a.first_hit = d_first_hit;
    a.labels = d_labels;
    a.error = flag;
    if (int rc = launch_lane_env_step(b, "k_tenv_macro", kernel, a.L.plane_off, bpc, a)) return rc;
    // t_max, not the longest run of rounds (which the host does not know): the next call's draws stay disjoint from
    // this one's whatever the envs did, and whether or not an env was refused
    b->update_count += t_max;
    if (!check) return 0;
    int32_t err;
    if (int rc = b->tenv.err.read_and_clear(b, &err)) return rc;
    if (err)
        return fail(PBN_E_RANGE, "Invalid action: an action outside [0, %d] or a limit outside [1, %u] (envs holding "
                                 "one were left untouched)", b->N, mode == PBN_MACRO_INTERVAL ? (unsigned)t_max : 10u);
    return 0;
}

int pbn_tenv_reset_device(pbn_batch* b, const uint64_t* d_states, uint64_t n_states, const uint8_t* d_mask) {
    CHECK_NN(b, "batch");
    CHECK_NN(d_states, "d_states");
    if (int rc = check_table_batch(b, "pbn_tenv_reset_device")) return rc;
    if (n_states == 0 || n_states >> 32) return fail(PBN_E_INVALID, "n_states outside [1, 2^32)");
    SET_DEV(b);
    // k_env_set_reset over one attractor (row_off null), n_steps left alone; n_states >= 1, so no env is skipped and
    // the flag is never raised
    EnvSetResetArgs a{};
    a.state = b->d_state;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.reset_count = b->reset_count;
    a.n_rows = (uint32_t)n_states;
    a.rows = d_states;
    a.mask = d_mask;
    a.clear_node0 = 1;
    if (int rc = timed_launch(b, "k_env_set_reset", [&] { return launch_env_set_reset(b->W, a, b->stream); })) return rc;
    b->reset_count++;
    return 0;
}

}  // extern "C"
