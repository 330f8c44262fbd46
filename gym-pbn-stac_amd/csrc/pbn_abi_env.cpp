// pbn_abi_env.cpp -- R6: env reset, the env-step launch (env_plan, pbn_env_plan.hpp, decides; env_launch launches), the four
// pbn_env_step* / rollout entry points and the hand-off / grid-pool statistics.
#include "pbn_host.hpp"

static int env_reset(pbn_batch* b, const pbn_envcfg* cfg_c, const void* d_mask) {
    pbn_envcfg* cfg = const_cast<pbn_envcfg*>(cfg_c);
    const uint64_t* cubes = (const uint64_t*)cfg->dev_reset.on(b->device, cfg->reset.data(), 8 * cfg->reset.size());
    if (!cubes) return fail(PBN_E_NOMEM, "envcfg upload failed");
    return run_init(b, cfg, d_mask, cubes, cubes + cfg->reset.size() / 2);
}

#define CHECK_RESET(b, cfg)                                                                        \
    CHECK_NN(b, "batch");                                                                          \
    CHECK_NN(cfg, "cfg");                                                                          \
    if (cfg->net != b->net) return fail(PBN_E_INVALID, "envcfg belongs to another network");       \
    if (cfg->H_reset < 1) return fail(PBN_E_STATE, "envcfg has no reset cubes (all_attractors[0])"); \
    SET_DEV(b)

// One R6 launch as its entry point asked for it; env_plan_in and env_launch read the same one.
struct EnvCall {
    int A, dedup, offset;
    uint32_t cap;  // updates per env step
    int replay;
    uint32_t n_calls;  // env steps per env
};

// replay mode has no update cap: an env step ends with its recorded draws
constexpr uint32_t REPLAY_NO_CAP = 0xFFFFFFFFu;

// The plan's inputs (pbn_env_plan.hpp): the one place that reads the batch and the env config for the decision.
static EnvPlanIn env_plan_in(const pbn_batch* b, const pbn_envcfg* cfg, const EnvCall& c) {
    EnvPlanIn in;
    in.B = b->B;
    in.W = b->W;
    in.N = b->net->N;
    in.kind = b->net->kind;
    in.n_cu = b->n_cu;
    in.counters_ok = cfg->counters_ok;
    in.H = cfg->H;
    in.pmax = cfg->L.pmax;
    in.image_bytes = cfg->L.bytes;
    in.off_rec = cfg->L.off_rec;
    in.off_cubes = cfg->off_cubes;
    in.rs = thr32_layout(cfg->L).rs;
    in.replay = c.replay != 0;
    in.cap = c.cap;
    in.n_calls = c.n_calls;
    in.knob = b->knob.env;
    in.grid_steal = b->knob.env_grid_steal;
    return in;
}

// env_plan with the device's answer to its occupancy queries
static EnvPlan env_call_plan(const pbn_batch* b, const pbn_envcfg* cfg, const EnvCall& c) {
    return env_plan(env_plan_in(b, cfg, c), [b](int mode, int grp, uint32_t image_bytes, uint32_t chunk, int* bpc) {
        return max_blocks_env(b->W, b->net->kind, mode, grp, image_bytes, bpc, chunk);
    });
}

// Device pointers of one R6 launch: actions in, outputs, and (replay mode) the recorded draws.
struct EnvIO {
    const int32_t* act;
    uint64_t* obs;
    int32_t* rew;
    uint8_t* flags;
    uint32_t* nup;
    const void *draw_off = nullptr, *draws_i = nullptr, *draws_k = nullptr;
};

// The acting half: uploads what the plan needs, zeroes the launch's counters, fills EnvArgs and launches.
static int env_launch(pbn_batch* b, pbn_envcfg* cfg, const EnvCall& c, const EnvPlan& p, const EnvIO& io) {
    if (p.error) return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)p.error));
    const int replay = c.replay;
    EnvArgs a{};
    a.img = cfg->dev_image.on(b->device, cfg->image.data(), cfg->image.size());
    if (!a.img) return fail(PBN_E_NOMEM, "envcfg upload failed");
    if (p.host_image) {
        {
            std::lock_guard<std::mutex> g(cfg->mu);
            if (cfg->gen_image.empty()) cfg->gen_image = env_gen_image(cfg, p.erec_shift);
        }
        a.gen_img = cfg->dev_gen.on(b->device, cfg->gen_image.data(), cfg->gen_image.size());
        if (!a.gen_img) return fail(PBN_E_NOMEM, "envcfg upload failed");
    }
    a.state = b->d_state;
    a.n_steps = b->d_nsteps;
    a.actions = io.act;
    a.obs = io.obs;
    a.reward = io.rew;
    a.flags = io.flags;
    a.n_updates = io.nup;
    a.error = b->d_error;
    a.L = cfg->L;
    a.off_cubes = cfg->off_cubes + p.erec_shift;
    a.off_target = cfg->off_target + p.erec_shift;
    a.off_ndelta = cfg->off_ndelta + p.erec_shift;
    a.erec_shift = p.erec_shift;
    a.tail_max = p.tail_max;
    a.lane_limit = p.lane_limit;
    a.mode = p.mode;
    a.grp = p.grp;
    a.chunk = p.chunk;
    a.off_gen = p.mode == ENV_MODE_GROUP ? cfg->L.bytes : cfg->L.bytes + p.erec_shift + 8u * (uint32_t)b->W * ENV_BLOCK;
    if (int rc = b->r6.counter.ensure(8)) return rc;
    a.counter = (unsigned long long*)b->r6.counter.p;
    a.n_cubes = cfg->H;
    a.B = b->B;
    a.env_base = b->env_base;
    a.seed = b->seed;
    a.call_idx = b->r6.calls;
    a.update_cap = c.cap;
    a.A = c.A;
    a.offset = c.offset;
    a.dedup = c.dedup ? 1 : 0;
    a.horizon = cfg->horizon;
    a.reward_success = cfg->reward_success;
    a.action_cost = cfg->action_cost;
    a.first_tested = cfg->first_tested;
    a.n_calls = c.n_calls;
    a.draw_off = (const int64_t*)io.draw_off;
    a.draws_i = (const uint32_t*)io.draws_i;
    a.draws_k = (const uint64_t*)io.draws_k;
    HIP_TRY(hipMemsetAsync(b->d_error, 0, 4, b->stream));
    HIP_TRY(hipMemsetAsync(b->r6.counter.p, 0, 8, b->stream));
    if (p.handoff) {
        if (int rc = b->r6.steal.ensure(16)) return rc;
        HIP_TRY(hipMemsetAsync(b->r6.steal.p, 0, 16, b->stream));
        a.steal_local = 1;
        // [0] envs handed off, [1] tail helpers recruited, [2] tail blocks read from helper rings, [3] of those,
        // the ones whose helper had not written them when the session reached them
        a.steal_count = (uint32_t*)b->r6.steal.p;
        a.tail_helpers = b->knob.env_helpers;
    }
    if (p.gpool) {
        // grid pool: control words (GPOOL_CTL_BYTES, zeroed per launch), then the slots' state words, then the slots
        const size_t st_bytes = 4 * (size_t)GPOOL_CAP, sl_bytes = 8 * (size_t)GPOOL_GRANULES * GPOOL_CAP;
        if (int rc = b->r6.gpool.ensure(GPOOL_CTL_BYTES + st_bytes + sl_bytes)) return rc;
        HIP_TRY(hipMemsetAsync(b->r6.gpool.p, 0, GPOOL_CTL_BYTES, b->stream));
        uint8_t* base = static_cast<uint8_t*>(b->r6.gpool.p);
        // epochs 1 .. 2^30 - 1: slot words of earlier launches never match; the whole pool is zeroed at its
        // first use and when the epoch wraps
        if (b->r6.gpool_epoch == 0u || b->r6.gpool_epoch >= 0x3FFFFFFEu)
            HIP_TRY(hipMemsetAsync(base, 0, GPOOL_CTL_BYTES + st_bytes + sl_bytes, b->stream));
        b->r6.gpool_epoch = b->r6.gpool_epoch % 0x3FFFFFFEu + 1u;
        a.gpool_ctl = reinterpret_cast<uint32_t*>(base);
        a.gpool_state = reinterpret_cast<uint32_t*>(base + GPOOL_CTL_BYTES);
        a.gpool = reinterpret_cast<uint64_t*>(base + GPOOL_CTL_BYTES + st_bytes);
        a.gpool_cap = b->knob.env_grid_slots > 0 ? (uint32_t)b->knob.env_grid_slots : GPOOL_CAP;
        a.gpool_epoch = b->r6.gpool_epoch;
        a.gpool_cu_idle = b->knob.env_pool_cu_idle != 0 ? 1u : 0u;
        if (io.obs != b->s_obs.p) b->r6.fault_check = true;  // device path: pbn_sync reads the sticky fault word
    }
    if (int rc = timed_launch(b, "k_env", [&] { return launch_env_multi(b->W, a, replay, p.grid, b->stream); })) return rc;
    if (!replay) b->r6.calls += c.n_calls;
    b->r6.last = p;
    return 0;
}

static int env_host_common(pbn_batch* b, pbn_envcfg* cfg, const int32_t* actions, int A, int offset) {
    if (cfg->net != b->net) return fail(PBN_E_INVALID, "envcfg belongs to another network");
    if (int rc = validate_actions(b, actions, A, offset)) return rc;
    size_t ab = 4 * (size_t)A * b->B;
    if (int rc = b->s_act.ensure(ab)) return rc;
    if (int rc = b->s_obs.ensure(8 * (size_t)b->W * b->B)) return rc;
    if (int rc = b->s_rew.ensure(4 * b->B)) return rc;
    if (int rc = b->s_flags.ensure(b->B)) return rc;
    if (int rc = b->s_nup.ensure(4 * b->B)) return rc;
    return h2d(b, b->s_act.p, actions, ab);
}

// The host path's staging buffers as a launch's pointers.
static EnvIO env_host_io(const pbn_batch* b) {
    return EnvIO{(const int32_t*)b->s_act.p, (uint64_t*)b->s_obs.p, (int32_t*)b->s_rew.p, (uint8_t*)b->s_flags.p,
                 (uint32_t*)b->s_nup.p};
}

// The launch's error word (d_error[0]): bit 1 = a grid-pool wait timed out, otherwise an action out of range.
static int env_error(int32_t err) {
    if (err & 2) return fail(PBN_E_HIP, "k_env grid pool: a wait timed out");
    if (err) return fail(PBN_E_RANGE, "an action was out of range");
    return 0;
}

static int env_host_out(pbn_batch* b, uint64_t* obs, int32_t* reward, uint8_t* flags, uint32_t* n_updates) {
    const size_t so = 8 * (size_t)b->W * b->B, sr = 4 * b->B, sf = b->B, sn = 4 * b->B;
    const size_t oo = 0, orr = oo + so, of = orr + sr, on = of + sf, oe = (on + sn + 3) & ~(size_t)3;
    int32_t err = 0;
    if (oe + 4 <= PinBuf::CAP && b->pin.ready()) {  // one pinned block, one sync
        uint8_t* q = b->pin.p;
        HIP_TRY(hipMemcpyAsync(q + oo, b->s_obs.p, so, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(q + orr, b->s_rew.p, sr, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(q + of, b->s_flags.p, sf, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(q + on, b->s_nup.p, sn, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(q + oe, b->d_error, 4, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (obs) memcpy(obs, q + oo, so);
        if (reward) memcpy(reward, q + orr, sr);
        if (flags) memcpy(flags, q + of, sf);
        if (n_updates) memcpy(n_updates, q + on, sn);
        memcpy(&err, q + oe, 4);
        return env_error(err);
    }
    if (obs) HIP_TRY(hipMemcpyAsync(obs, b->s_obs.p, so, hipMemcpyDeviceToHost, b->stream));
    if (reward) HIP_TRY(hipMemcpyAsync(reward, b->s_rew.p, sr, hipMemcpyDeviceToHost, b->stream));
    if (flags) HIP_TRY(hipMemcpyAsync(flags, b->s_flags.p, sf, hipMemcpyDeviceToHost, b->stream));
    if (n_updates) HIP_TRY(hipMemcpyAsync(n_updates, b->s_nup.p, sn, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(&err, b->d_error, 4, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return env_error(err);
}

// n_calls env steps per env in one launch, inputs and outputs in device memory (no host round trip)
static int env_steps_device(pbn_batch* b, const pbn_envcfg* cfg_c, uint32_t n_calls, const int32_t* d_actions, int A,
                            int dedup, int offset, uint32_t update_cap, uint64_t* d_obs, int32_t* d_reward,
                            uint8_t* d_flags, uint32_t* d_n_updates) {
    CHECK_NN(b, "batch");
    CHECK_NN(cfg_c, "cfg");
    CHECK_NN(d_actions, "d_actions");
    CHECK_NN(d_obs, "d_obs");
    CHECK_NN(d_reward, "d_reward");
    CHECK_NN(d_flags, "d_flags");
    CHECK_NN(d_n_updates, "d_n_updates");
    pbn_envcfg* cfg = const_cast<pbn_envcfg*>(cfg_c);
    if (cfg->net != b->net) return fail(PBN_E_INVALID, "envcfg belongs to another network");
    if (int rc = check_action_shape(A, offset)) return rc;
    if (n_calls < 1 || n_calls > (1u << 20)) return fail(PBN_E_INVALID, "n_steps=%u outside [1, 2^20]", n_calls);
    SET_DEV(b);
    const EnvCall c{A, dedup, offset, update_cap, 0, n_calls};
    return env_launch(b, cfg, c, env_call_plan(b, cfg, c), EnvIO{d_actions, d_obs, d_reward, d_flags, d_n_updates});
}

// The first `words` counters of the last launch's tail hand-off (zeros if it had none).
static int read_steal(pbn_batch* b, uint32_t* out, const char* name, int first, int words) {
    CHECK_NN(b, "batch");
    CHECK_NN(out, name);
    SET_DEV(b);
    for (int k = 0; k < words; k++) out[k] = 0;
    if (!b->r6.last.handoff) return 0;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(out, (const uint32_t*)b->r6.steal.p + first, 4 * (size_t)words, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" {

int pbn_env_reset(pbn_batch* b, const pbn_envcfg* cfg, const uint8_t* mask) {
    CHECK_RESET(b, cfg);
    const void* d_mask = nullptr;
    if (mask) {
        if (int rc = b->s_mask.ensure(b->B)) return rc;
        HIP_TRY(hipMemcpyAsync(b->s_mask.p, mask, b->B, hipMemcpyHostToDevice, b->stream));
        d_mask = b->s_mask.p;
    }
    if (int rc = env_reset(b, cfg, d_mask)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_env_reset_device(pbn_batch* b, const pbn_envcfg* cfg, const uint8_t* d_mask) {
    CHECK_RESET(b, cfg);
    return env_reset(b, cfg, d_mask);
}

int pbn_set_n_steps(pbn_batch* b, const int64_t* n_steps) {
    CHECK_NN(b, "batch");
    CHECK_NN(n_steps, "n_steps");
    SET_DEV(b);
    HIP_TRY(hipMemcpyAsync(b->d_nsteps, n_steps, 8 * b->B, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_get_n_steps(pbn_batch* b, int64_t* n_steps) {
    CHECK_NN(b, "batch");
    CHECK_NN(n_steps, "n_steps");
    SET_DEV(b);
    HIP_TRY(hipMemcpyAsync(n_steps, b->d_nsteps, 8 * b->B, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int pbn_env_step_multi(pbn_batch* b, const pbn_envcfg* cfg_c, const int32_t* actions, int A, int dedup, int offset,
                       uint32_t update_cap, uint64_t* obs, int32_t* reward, uint8_t* flags, uint32_t* n_updates) {
    CHECK_NN(b, "batch");
    CHECK_NN(cfg_c, "cfg");
    CHECK_NN(actions, "actions");
    pbn_envcfg* cfg = const_cast<pbn_envcfg*>(cfg_c);
    SET_DEV(b);
    if (int rc = env_host_common(b, cfg, actions, A, offset)) return rc;
    const EnvCall c{A, dedup, offset, update_cap, 0, 1};
    if (int rc = env_launch(b, cfg, c, env_call_plan(b, cfg, c), env_host_io(b))) return rc;
    return env_host_out(b, obs, reward, flags, n_updates);
}

int pbn_env_step_multi_device(pbn_batch* b, const pbn_envcfg* cfg, const int32_t* d_actions, int A, int dedup,
                              int offset, uint32_t update_cap, uint64_t* d_obs, int32_t* d_reward, uint8_t* d_flags,
                              uint32_t* d_n_updates) {
    return env_steps_device(b, cfg, 1, d_actions, A, dedup, offset, update_cap, d_obs, d_reward, d_flags, d_n_updates);
}

int pbn_env_rollout_multi_device(pbn_batch* b, const pbn_envcfg* cfg, uint32_t n_steps, const int32_t* d_actions,
                                 int A, int dedup, int offset, uint32_t update_cap, uint64_t* d_obs, int32_t* d_reward,
                                 uint8_t* d_flags, uint32_t* d_n_updates) {
    return env_steps_device(b, cfg, n_steps, d_actions, A, dedup, offset, update_cap, d_obs, d_reward, d_flags,
                            d_n_updates);
}

int pbn_env_step_multi_replay(pbn_batch* b, const pbn_envcfg* cfg_c, const int32_t* actions, int A, int dedup,
                              int offset, const int64_t* draw_offsets, const uint32_t* draws_i,
                              const uint64_t* draws_k, uint64_t* obs, int32_t* reward, uint8_t* flags,
                              uint32_t* n_updates) {
    CHECK_NN(b, "batch");
    CHECK_NN(cfg_c, "cfg");
    CHECK_NN(actions, "actions");
    CHECK_NN(draw_offsets, "draw_offsets");
    pbn_envcfg* cfg = const_cast<pbn_envcfg*>(cfg_c);
    const int64_t nd = draw_offsets[b->B];
    if (draw_offsets[0] != 0 || nd < 0) return fail(PBN_E_INVALID, "draw_offsets must start at 0");
    for (uint64_t e = 0; e < b->B; e++)
        if (draw_offsets[e + 1] < draw_offsets[e]) return fail(PBN_E_INVALID, "draw_offsets not non-decreasing");
    const uint32_t lo = b->net->kind == PBN_KIND_PROB_TABLE ? 1u : 0u;
    for (int64_t q = 0; q < nd; q++)
        if (draws_i[q] >= (uint32_t)b->N || draws_i[q] < lo || (draws_k[q] >> 53))
            return fail(PBN_E_RANGE, "replay draw %lld out of range", (long long)q);
    SET_DEV(b);
    if (int rc = env_host_common(b, cfg, actions, A, offset)) return rc;
    if (int rc = b->s_off.ensure(8 * (b->B + 1))) return rc;
    if (int rc = b->s_replay_i.ensure(4 * (size_t)std::max<int64_t>(nd, 1))) return rc;
    if (int rc = b->s_replay_k.ensure(8 * (size_t)std::max<int64_t>(nd, 1))) return rc;
    HIP_TRY(hipMemcpyAsync(b->s_off.p, draw_offsets, 8 * (b->B + 1), hipMemcpyHostToDevice, b->stream));
    if (nd) {
        HIP_TRY(hipMemcpyAsync(b->s_replay_i.p, draws_i, 4 * (size_t)nd, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->s_replay_k.p, draws_k, 8 * (size_t)nd, hipMemcpyHostToDevice, b->stream));
    }
    EnvIO io = env_host_io(b);
    io.draw_off = b->s_off.p;
    io.draws_i = b->s_replay_i.p;
    io.draws_k = b->s_replay_k.p;
    const EnvCall c{A, dedup, offset, REPLAY_NO_CAP, 1, 1};
    if (int rc = env_launch(b, cfg, c, env_call_plan(b, cfg, c), io)) return rc;
    return env_host_out(b, obs, reward, flags, n_updates);
}

int pbn_env_handoffs(pbn_batch* b, uint32_t* count) {
    return read_steal(b, count, "count", 0, 1);
}

int pbn_env_tail_helpers(pbn_batch* b, uint32_t* count) {
    return read_steal(b, count, "count", 1, 1);
}

int pbn_env_tail_stats(pbn_batch* b, uint32_t* stats) {
    return read_steal(b, stats, "stats", 0, 4);
}

int pbn_env_grid_stats(pbn_batch* b, uint32_t* stats) {
    CHECK_NN(b, "batch");
    CHECK_NN(stats, "stats");
    SET_DEV(b);
    for (int k = 0; k < 4; k++) stats[k] = 0;
    if (!b->r6.last.gpool) return 0;
    HIP_TRY(hipStreamSynchronize(b->stream));
    uint32_t ctl[6];
    HIP_TRY(hipMemcpy(ctl, b->r6.gpool.p, sizeof ctl, hipMemcpyDeviceToHost));
    stats[0] = ctl[3];  // envs pushed
    stats[1] = ctl[1];  // tickets taken
    stats[2] = ctl[4];  // waits given up
    stats[3] = ctl[2];  // live count at the end (0 after a complete launch)
    return 0;
}

}  // extern "C"
