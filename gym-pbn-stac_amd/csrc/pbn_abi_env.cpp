// pbn_abi_env.cpp -- R6: env reset, the env-step launch (env_plan decides, env_launch launches), the four
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

// Lanes per env for the R6 kernel: 1 (lane mode, k_env) while the batch fills the chip
// several times over; group mode where it does not and the until-attractor tail would
// leave lanes idle (measured: DESIGN.md section 6).
// Per-step call, Bittner-200, 1 MI355X (256 CUs): G = 8 beats lane mode up to 32k envs (0.21 vs
// 0.33 ms at B = 1, 0.88 vs 1.99 ms at 8k, 1.85 vs 2.04 ms at 32k) and loses from 64k on (2.31 vs
// 2.07 ms; 131k: 3.28 vs 2.60 ms) -- the crossover sits near 48k envs.
// Group mode (G = 8 lanes per env) for small batches -- except where the tail kernel (k_env ENV_MODE_TAIL:
// <= 4 cubes and its 16-B env records fit) applies: its tail mode with one env per wave
// (env_lane_limit) is faster at every batch size measured (profiles/r03_r6_lanes_sweep.json)
static int env_group_size(const pbn_batch* b, bool tail_kernel) {
    if (tail_kernel) return 1;
    return b->B * 8 <= (uint64_t)b->n_cu * 1536 ? 8 : 1;
}

// The decision half of an R6 launch: kernel mode, geometry and hand-offs. Reads the batch and the env config
// and queries occupancy; writes no buffer and does not touch the stream. p.error: a failed occupancy query.
static EnvPlan env_plan(const pbn_batch* b, const pbn_envcfg* cfg, int replay, uint32_t cap, uint32_t n_calls) {
    EnvPlan p;
    const Knobs& k = b->knob;
    // cooperative draw generation: predictor mix, Philox, record index fits the u16 entry
    int mode = (cfg->fast && !replay && b->net->kind == KIND_PREDICTOR_MIX && cfg->L.pmax <= 16 &&
                b->net->N <= 512 && !k.env_no_gen)
                   ? (int)ENV_MODE_COOP
                   : cfg->fast;
    // cooperative-draw mode keeps 16-B env records in LDS where the 8-B predictor records were
    // (env_record_words, pbn_params.hpp): the tables after them move up by erec_shift. Whether they fit is
    // decided first, so that the group-size rule below knows whether the tail kernel (ENV_MODE_TAIL) applies
    uint32_t erec_shift = 0;
    bool erec_fits = false;
    if (mode == ENV_MODE_COOP) {
        // rows of rs records (thr32_layout: tp4 + 1 slots at least, for the saturated choice)
        const uint32_t nrec = (uint32_t)b->net->N * thr32_layout(cfg->L).rs;
        erec_shift = cfg->L.off_rec + 16u * nrec - cfg->off_cubes;
        erec_fits = nrec <= 65535u &&
                    env_lds_bytes(b->W, cfg->L.bytes + erec_shift, ENV_MODE_COOP, 1, ENV_CHUNK_SMALL) <= ENV_LDS_MAX;
    }
    // group mode (k_env_grp: G lanes per env, G updates per round trip; its rows need no env records)
    int grp = 1;
    if (mode == ENV_MODE_COOP && b->net->N <= 256) {
        grp = k.env_group ? k.env_group : env_group_size(b, erec_fits && cfg->H <= 4);
        if (grp != 2 && grp != 4 && grp != 8) grp = 1;
        if (grp > 1) mode = ENV_MODE_GROUP;
    }
    if (mode == ENV_MODE_COOP) {
        if (!erec_fits)
            mode = cfg->fast;  // too large for the u16 record index / one workgroup's LDS
        else if (cfg->H <= 4)
            mode = ENV_MODE_TAIL;  // the same kernel with one packed counter word (<= 4 cubes)
        // ENV_MODE_TAIL adds the workgroup hand-off control words: re-check the fit with the final mode
        if (mode == ENV_MODE_TAIL &&
            env_lds_bytes(b->W, cfg->L.bytes + erec_shift, ENV_MODE_TAIL, 1, ENV_CHUNK_SMALL) > ENV_LDS_MAX)
            mode = cfg->fast;
    }
    const bool coop = mode == ENV_MODE_COOP || mode == ENV_MODE_TAIL;
    if (!coop) erec_shift = 0;
    const uint32_t img = cfg->L.bytes + erec_shift;
    // PBNSIM_ENV_KERNEL_IMAGE=1: the kernel builds its LDS image itself (tests keep that path covered)
    p.host_image = coop && img % 16u == 0u && !k.env_kernel_image;
    int bpc = 1;
    uint32_t chunk = ENV_CHUNK_SMALL;
    if (coop) {
        // the draw-round chunk (pbn_params.hpp ENV_CHUNK_SMALL / _LARGE): the large one unless the small
        // one's draw buffers let more workgroups onto a CU and the launch is a throughput-bound fused run
        // (>= 16 env steps per env over a queue of >= 4 envs per lane of the large one's grid), or the large
        // one does not fit one workgroup's 64 KiB; PBNSIM_ENV_CHUNK=32 / 48 overrides
        int bpc_s = 1, bpc_l = 1;
        p.error = max_blocks_env(b->W, b->net->kind, mode, grp, img, &bpc_s, ENV_CHUNK_SMALL);
        const bool large_fits = env_lds_bytes(b->W, img, mode, 1, ENV_CHUNK_LARGE) <= ENV_LDS_MAX;
        if (large_fits && !p.error)
            p.error = max_blocks_env(b->W, b->net->kind, mode, grp, img, &bpc_l, ENV_CHUNK_LARGE);
        const uint64_t lanes_l = (uint64_t)b->n_cu * (uint64_t)bpc_l * ENV_BLOCK;
        const bool throughput = n_calls >= 16u && b->B >= 4u * lanes_l && bpc_s > bpc_l;
        chunk = large_fits && !throughput ? ENV_CHUNK_LARGE : ENV_CHUNK_SMALL;
        if (k.env_chunk == (int)ENV_CHUNK_SMALL || (k.env_chunk == (int)ENV_CHUNK_LARGE && large_fits))
            chunk = (uint32_t)k.env_chunk;
        bpc = chunk == ENV_CHUNK_LARGE ? bpc_l : bpc_s;
    } else {
        p.error = max_blocks_env(b->W, b->net->kind, mode, grp, img, &bpc);
    }
    if (k.env_bpc) bpc = std::min(bpc, k.env_bpc);
    p.tail_max = k.env_tail >= 0 ? (uint32_t)k.env_tail : ENV_TAIL_DEFAULT;
    // tail-mode kernel: small batches (ENV_ONE_LANE_ENVS_PER_SLOT envs per wave slot) take one env per
    // wave at a time -- every wave resolves its env 64 updates per block and takes the next from the
    // queue when it is done (PBNSIM_ENV_LANES overrides; 64 = lane mode, the tail at the end)
    p.lane_limit = 64u;
    if (mode == ENV_MODE_TAIL) {
        const uint64_t slots = (uint64_t)b->n_cu * (uint64_t)bpc * (ENV_BLOCK / 64);
        if (k.env_lane_limit > 0)
            p.lane_limit = (uint32_t)k.env_lane_limit;
        else if (p.tail_max >= 1 && b->B <= ENV_ONE_LANE_ENVS_PER_SLOT * slots)
            p.lane_limit = 1u;
    }
    // lanes per env (group mode) or, with a lane limit, 64 / limit lane slots per env
    p.grid = b->grid_for(p.lane_limit < 64u ? (b->B * 64u + p.lane_limit - 1u) / p.lane_limit : b->B * (uint64_t)grp, bpc,
                         env_block(mode));
    // PBNSIM_ENV_GRID: exactly that many workgroups (at most the resident count; persistent waves: any grid
    // drains the counter, and surplus workgroups find the queue empty)
    if (k.env_grid_cap) p.grid = std::min(k.env_grid_cap, b->n_cu * bpc);
    // tail hand-off (k_env ENV_MODE_TAIL): a wave holding several envs in tail mode passes envs it has not
    // started on to idle waves of its workgroup (LDS). One lane per wave taking envs (small batches)
    // never holds two: off there
    p.handoff = mode == ENV_MODE_TAIL && k.env_steal && p.tail_max >= 1u && p.lane_limit >= 2u;
    p.gpool = p.handoff && (k.env_grid_steal > 0 || (k.env_grid_steal < 0 && (cap >= GPOOL_MIN_CAP || n_calls > 1u)));
    p.mode = mode;
    p.grp = grp;
    p.erec_shift = erec_shift;
    p.chunk = chunk;
    p.bpc = bpc;
    p.kernel = replay ? std::min(mode, (int)ENV_MODE_COUNTERS) : mode;
    return p;
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
static int env_launch(pbn_batch* b, pbn_envcfg* cfg, const EnvPlan& p, const EnvIO& io, int A, int dedup, int offset,
                      uint32_t cap, int replay, uint32_t n_calls) {
    if (p.error) return fail(PBN_E_HIP, "occupancy query: %s", hipGetErrorString((hipError_t)p.error));
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
    a.fast = p.mode;
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
    a.update_cap = cap;
    a.A = A;
    a.offset = offset;
    a.dedup = dedup ? 1 : 0;
    a.horizon = cfg->horizon;
    a.reward_success = cfg->reward_success;
    a.action_cost = cfg->action_cost;
    a.first_tested = cfg->first_tested;
    a.n_calls = n_calls;
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
    if (!replay) b->r6.calls += n_calls;
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
    const EnvIO io{d_actions, d_obs, d_reward, d_flags, d_n_updates};
    return env_launch(b, cfg, env_plan(b, cfg, 0, update_cap, n_calls), io, A, dedup, offset, update_cap, 0, n_calls);
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
    if (int rc = env_launch(b, cfg, env_plan(b, cfg, 0, update_cap, 1), env_host_io(b), A, dedup, offset, update_cap, 0, 1))
        return rc;
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
    if (int rc = env_launch(b, cfg, env_plan(b, cfg, 1, 0xFFFFFFFFu, 1), io, A, dedup, offset, 0xFFFFFFFFu, 1, 1)) return rc;
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
