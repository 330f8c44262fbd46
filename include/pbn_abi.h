/*
 * pbn_abi.h -- C ABI of libpbnsim.so, the MI355X (gfx950) vectorised PBN simulator.
 *
 * The reference (jakub-zarzycki2022/gym-PBN-stac) is pure Python; its hot path
 * sits behind plain method calls. Each entry point below names the reference
 * interface it replaces (file:line, relative to the reference root). A Python
 * ctypes binding lives in gym-pbn-stac_amd/gym_pbn_amd/_lib.py; INTEGRATION.md
 * shows the binding a gym-PBN maintainer would add.
 *
 * Conventions
 *  - Every function returns PBN_OK (0) or a negative PBN_E_* code and never
 *    aborts; pbn_last_error() returns a thread-local message for the last failure.
 *  - State is bit-packed: env e, node i lives in bit (i % 64) of word
 *    e*W + i/64, W = ceil(N/64). Host arrays are [B][W] uint64.
 *  - The library owns all device memory and copies network tables; callers own
 *    host arrays, which are read or written only during the call.
 *  - One batch = one device + one HIP stream. Calls on one batch must be
 *    serialised by the caller; different batches may be driven from different
 *    threads. Functions taking host outputs synchronise the batch stream; the
 *    rest are asynchronous until pbn_sync().
 *  - RNG modes: PHILOX (production; counter-based, keyed by
 *    (seed, global env id, update counter) so results do not depend on batch
 *    size or GPU count), REPLAY (caller supplies the reference's own draws), and
 *    MT (each env runs CPython's MT19937 -- and for probability-table networks
 *    numpy's legacy MT19937 too -- seeded like random.seed(s)/np.random.seed(s),
 *    reproducing the reference trajectory from the seed alone).
 */
#ifndef PBN_ABI_H
#define PBN_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBN_ABI_VERSION 26

enum {
    PBN_OK = 0,
    PBN_E_INVALID = -1,     /* bad argument / descriptor */
    PBN_E_RANGE = -2,       /* node or action out of range (reference: ValueError, base.py:283-284) */
    PBN_E_HIP = -3,         /* HIP runtime failure */
    PBN_E_NOMEM = -4,       /* device allocation failed */
    PBN_E_UNSUPPORTED = -5, /* network outside kernel limits (N > 512, tables > LDS budget) */
    PBN_E_STATE = -6        /* wrong mode / uninitialised (reference: Exception, base.py:90-91) */
};

enum { PBN_KIND_PREDICTOR_MIX = 1, PBN_KIND_PROB_TABLE = 2 };

typedef struct pbn_net pbn_net;
typedef struct pbn_batch pbn_batch;
typedef struct pbn_envcfg pbn_envcfg;
typedef struct pbn_reach pbn_reach;

/* Network tables (see gym_pbn_amd/network.py for how they are derived).
 * PREDICTOR_MIX replaces base.Node.predictors (base.py:30-45) + Predstep (:89-119):
 *   pred_offsets [N+1], pred_inputs [P][3] node indices, pred_tt [P] 16-entry truth
 *   table over (x0<<3|x1<<2|x2<<1|x_self), pred_thr [P] exact 53-bit selection
 *   thresholds (predictor j is selected for the first j with k53 < thr[j]).
 * PROB_TABLE replaces common/node.py Node (input_mask, function; :22-38):
 *   node_k [N], input_offsets [N+1], inputs [sum k] (ascending, first = MSB),
 *   thr_offsets [N+1], thr [sum 2^k] = ceil(p * 2^53). */
typedef struct {
    int32_t kind;
    int32_t n_nodes;
    int32_t n_preds;
    const int32_t *pred_offsets;
    const int32_t *pred_inputs;
    const uint16_t *pred_tt;
    const uint64_t *pred_thr;
    const int32_t *node_k;
    const int32_t *input_offsets;
    const int32_t *inputs;
    const int64_t *thr_offsets;
    const uint64_t *thr;
} pbn_net_desc;

typedef struct {
    int32_t n_nodes, n_words, kind, device;
    uint64_t n_envs, env_id_base, seed;
    uint64_t update_count; /* Philox updates applied so far (batch-wide counter) */
    uint32_t env_call_count, reset_count;
    int32_t mt_ready; /* 1 after pbn_mt_seed */
    int32_t env_lanes; /* last R6 env-step launch: 1 = one lane per env (k_env), 2/4/8 = lanes per env (k_env_grp) */
    int32_t roll_lanes; /* rollout kernel: 1 = one lane per env (k_rollout), 2/4/8 = lanes per env (k_rollout_grp) */
    int32_t env_grid;   /* last R6 env-step launch: workgroups (256 lanes each; lanes refill from a work counter) */
    int32_t env_kernel; /* last R6 env-step launch: 0 = cube matching, 1 = byte counters, 2 = byte counters +
                           wave-generated draws, 3 = group mode (k_env_grp), 4 = 2 with one counter word (<= 4 cubes) */
    int32_t env_lane_limit; /* last R6 env-step launch, env_kernel 4: lanes per wave taking envs from the work
                               queue (64 = every lane; 1 = one env per wave at a time, resolved 64 updates per block) */
    int32_t env_handoff;    /* last R6 env-step launch, env_kernel 4: 1 if a wave in tail mode could hand envs it had
                               not started on to idle waves of its workgroup (PBNSIM_ENV_STEAL=0 turns it off);
                               count: pbn_env_handoffs */
    int32_t env_chunk;      /* last R6 env-step launch, env_kernel 2/4: updates per lane between draw rounds (32 or 48;
                               PBNSIM_ENV_CHUNK overrides) */
    int32_t step_chains;    /* pbn_step: launch chains a call of two or more updates runs as (contiguous env ranges,
                               one stream each, joined at the end of the call; PBNSIM_STEP_CHAINS forces 1, 2 or 4) */
} pbn_batch_info;

/* Attractor / goal description for the multi-flip env step (R6).
 * cubes: union of the attractor hypercubes (cabean output, '*' = don't care),
 *   care/value [n_cubes][W]: state s is attracting iff (s & care) == value for
 *   some cube -- the membership test of the expanded set built at
 *   pbn_target_multi.py:437-455 and queried at :489-492.
 * reset cubes: all_attractors[0] (reset draws one and fills '*' bits, :237-249).
 * target: all_attractors[-1][0] -- in_target() only ever tests target[0] (:190-199). */
typedef struct {
    int32_t n_cubes;
    const uint64_t *cube_care;
    const uint64_t *cube_value;
    int32_t n_reset_cubes;
    const uint64_t *reset_care;
    const uint64_t *reset_value;
    const uint64_t *target_care;  /* [W] */
    const uint64_t *target_value; /* [W] */
    int32_t horizon;              /* truncated = n_steps == horizon (:224) */
    int32_t reward_success;       /* +1000 (:218-219) */
    int32_t action_cost;          /* 1 per unique action value (:222) */
    /* 0: the first update's result is never tested -- the test after it is on the pre-update
     *    snapshot (PBNTargetMultiEnv, :133-134);
     * 1: the state after every update is tested (PBNTargetEnv.step(force=False), pbn_target.py:267-271). */
    int32_t first_update_tested;
} pbn_envcfg_desc;

/* flags returned per env by pbn_env_step_multi* */
enum { PBN_FLAG_TERMINATED = 1, PBN_FLAG_TRUNCATED = 2, PBN_FLAG_CAPPED = 4 };

/* ---- library ---- */
int pbn_abi_version(void);
const char *pbn_last_error(void);
int pbn_device_count(int *count);

/* ---- networks: replaces graph construction, bittner/utils.py:81-91 / pbn.py:78-87 ---- */
int pbn_net_create(const pbn_net_desc *desc, pbn_net **out);
void pbn_net_destroy(pbn_net *net);
/* Predictor-mix networks: the predictor record (in0 | in1<<16 | in2<<32 | tt<<48) that choice
 * word a selects for node `node`, read from the compact image the Philox kernels stage (u32
 * thresholds, saturated, overshoot slot) by the kernels' own rule -- host side, no device. For
 * tests: equals the record of predictor min(#{q : u32_k53(a) >= thr_q}, count - 1)
 * (Predstep's choice, base.py:94-97). */
int pbn_net_select_u32(const pbn_net *net, int32_t node, uint32_t a, uint64_t *record);
/* The support graphs' edge rule (see "attractor discovery" below) on the host copy of the network image, no
 * device: states [S][W] -> masks [S][W], bit i set iff node i can flip at that state. It is the one definition
 * the kernels of pbn_reach_* evaluate (csrc/pbn_reach_rule.hpp), so it pins the rule on a machine without a GPU.
 * PROB_TABLE networks: graph = PBN_TABLE_GRAPH_STG or PBN_TABLE_GRAPH_STEP, anything else PBN_E_INVALID.
 * PREDICTOR_MIX networks have one graph: `graph` is ignored. */
enum { PBN_TABLE_GRAPH_STG = 1, PBN_TABLE_GRAPH_STEP = 2 };
int pbn_net_unstable(const pbn_net *net, int32_t graph, const uint64_t *states, uint64_t n_states, uint64_t *masks);
/* The law behind that support (see "exact transition graph" below), host side, no device: states [S][W] -> mass
 * [S][N] uint64 in [0, 2^53], the probability in units of 2^-53 that node i takes the value 1 - x_i at that state
 * given that node i is the one updated. It is the one definition k_stg_rows evaluates (csrc/pbn_mass_rule.hpp), and
 * mass > 0 exactly where pbn_net_unstable sets the bit. `graph` as for pbn_net_unstable; under PBN_TABLE_GRAPH_STEP
 * node 0 has mass 0. */
int pbn_net_edge_mass(const pbn_net *net, int32_t graph, const uint64_t *states, uint64_t n_states, uint64_t *mass);

/* ---- batches of independent envs (the reference holds one Graph per env) ---- */
/* Tuning knobs, read from the environment once here (measurement and tests only):
 * PBNSIM_STORE_MODE, PBNSIM_ENVS_PER_THREAD, PBNSIM_STEP_BLOCK (step kernel);
 * PBNSIM_ENV_NO_GEN, PBNSIM_ENV_GROUP, PBNSIM_ENV_BPC, PBNSIM_ENV_CHUNK, PBNSIM_ENV_GRID, PBNSIM_ENV_TAIL,
 * PBNSIM_ENV_LANES, PBNSIM_ENV_STEAL, PBNSIM_ENV_HELPERS, PBNSIM_ENV_GRID_STEAL, PBNSIM_ENV_KERNEL_IMAGE (R6 env kernel);
 * every one is set by a `-m gpu` test; A/B-only knobs are compiled in by -DPBN_MEASURE_KNOBS (tools/build_exp.sh);
 * PBNSIM_SSD_WAVE, PBNSIM_SSD_SERIAL, PBNSIM_SSD_SHARED (SSD); PBNSIM_ROLL_GROUP (rollout lanes per env);
 * PBNSIM_STEP_GRAPH=0 (pbn_step without HIP graphs); PBNSIM_STEP_CHAINS (pbn_step's launch chains); PBNSIM_MT_LANES=1 (MT-mode steps of predictor-mix networks
 * on k_mt_step's per-lane loads instead of k_mt_staged's LDS windows). */
int pbn_batch_create(const pbn_net *net, int device, uint64_t n_envs, uint64_t env_id_base, uint64_t seed,
                     pbn_batch **out);
void pbn_batch_destroy(pbn_batch *b);
int pbn_batch_get_info(const pbn_batch *b, pbn_batch_info *info);
/* A batch's position in its Philox streams: every draw is keyed by (seed, global env id, one of these counters), so
 * the state words (pbn_get_state), n_steps (pbn_get_n_steps) and this struct are all a bit-exact checkpoint needs;
 * a batch created with the same network, seed and env_id_base and given the three back continues as the first would
 * have. update_count: pbn_step / pbn_rollout / pbn_step_forced updates so far; ssd_iters: pbn_ssd_run iterations;
 * sync_steps: pbn_synch_step steps (the choice stream has room for sync_steps < 2^48; the two flip streams,
 * pbn_ssd_run's and pbn_synch_step's perturbations, take the low 32 bits of their counter); env_call_count: env steps
 * launched (pbn_env_step_multi*, += n_steps for a fused rollout); reset_count: pbn_randomize_state / pbn_env_reset*
 * calls. The two 32-bit counters wrap modulo 2^32, also inside a fused rollout (env step t of a launch draws with
 * (uint32_t)(env_call_count + t)). pbn_batch_set_counters takes effect from the next call on: no captured step
 * graph holds a counter (replays read it from device memory, written by every pbn_step that replays one). Calls on
 * the batch are serialised by the caller, as everywhere. */
typedef struct {
    uint64_t update_count, ssd_iters, sync_steps;
    uint32_t env_call_count, reset_count;
} pbn_batch_counters;
int pbn_batch_get_counters(const pbn_batch *b, pbn_batch_counters *out);
int pbn_batch_set_counters(pbn_batch *b, const pbn_batch_counters *in);
/* Run every later call of this batch on `stream` (a hipStream_t, e.g. torch's current stream, so
 * kernels order with the caller's own work without host syncs; NULL = the default stream), or on
 * the batch's own stream again (own != 0). Work queued on the previous stream is waited for first. */
int pbn_batch_set_stream(pbn_batch *b, int own, void *stream);
/* Waits for the batch stream. PBN_E_HIP if a device-path R6 launch since the last pbn_sync dropped an env in
 * the grid pool (see pbn_env_grid_stats; never expected). */
int pbn_sync(pbn_batch *b);

/* ---- state I/O: Graph.setState / getState (base.py:364-366, 320-324), PBN.reset(state) (pbn.py:96-119) ---- */
int pbn_set_state(pbn_batch *b, const uint64_t *words);          /* host [B][W] */
int pbn_get_state(pbn_batch *b, uint64_t *words);                /* host [B][W] */
int pbn_set_state_device(pbn_batch *b, const void *dev_words);   /* device [B][W], same device */
int pbn_get_state_device(pbn_batch *b, void *dev_words);
/* One byte per node, device [B][N] uint8, from device words [B][W] (NULL = the batch's state);
 * Graph.getState (base.py:320-324) for the whole batch without leaving the GPU. Asynchronous. */
int pbn_unpack_bits_device(pbn_batch *b, const void *d_words, void *d_bits);
/* Graph.genRandState (base.py:368-370) / PBN.reset(None) (pbn.py:105-118) in Philox mode */
int pbn_randomize_state(pbn_batch *b);

/* ---- intervention: Graph.flipNode (base.py:280-284), PBN.flip (pbn.py:121-127) ----
 * actions [B][A] host int32; value 0 = no action, value v flips node v - offset
 * (offset 1: gym-PBN target envs, pbn_target.py:266-267; offset 0: PBNEnv, pbn_env.py:141-142).
 * dedup 1: act on unique values per row (torch-tensor input, pbn_target_multi.py:120-121). */
int pbn_flip(pbn_batch *b, const int32_t *actions, int A, int offset, int dedup);
/* Same with the actions already on the device (d_actions [B][A] int32, e.g. a torch policy's
 * output), on the batch stream. A row holding an out-of-range value is left untouched (the other
 * rows are flipped) and noted in a device flag. check 1: wait for the kernel, return PBN_E_RANGE
 * if the flag is set (by this call or by earlier check-0 calls) and clear it; check 0: return
 * at once (asynchronous; a later check-1 call reports). */
int pbn_flip_device(pbn_batch *b, const int32_t *d_actions, int A, int offset, int dedup, int check);

/* ---- the hot path: Graph.step (base.py:306-312) / PBN.step (pbn.py:129-133) ---- */
/* Philox mode, n_updates launches of one update each (state round-trips HBM). For batches under
 * 2^20 state words (launch-bound kernels) calls of two or more launches replay captured HIP graphs
 * (not on the null stream, nor with per-launch timing): one graph of exactly n_updates (<= 64)
 * launches when one is cached (pbn_step_prepare, or a call with the same n_updates as the previous
 * call), otherwise graphs of 64, 32, ..., 2 launches by the binary digits of n_updates. Larger batches
 * launch plainly (PBNSIM_STEP_GRAPH=0/1 overrides). Results are identical either way.
 * Launch chains: a batch large enough for each half to fill the GPU (pbn_batch_info.step_chains == 2) runs a
 * call of 128 or more updates as two chains of launches, one half of the envs each, chain 0 on the batch's
 * stream (pbn_batch_set_stream's, if set) and the other on a stream of the batch's own; the call forks that
 * stream off the batch's stream and joins it back, so anything queued on the batch's stream before or after the
 * call keeps its order against the whole batch. Such a batch replays per-chain graphs below 2^24 state words.
 * One chain: one update, per-launch timing, a call inside the caller's stream capture (the caller's graph gets
 * a linear run of launches). PBNSIM_STEP_CHAINS=1/2/4 forces the count for every call of two or more updates. */
int pbn_step(pbn_batch *b, uint32_t n_updates);
/* Captures the graphs pbn_step(b, n_updates) will replay now (setup only: nothing runs, the state
 * is untouched): for n_updates <= 64 one graph of exactly that many launches (the batch keeps the
 * four most recently used lengths), above that the 64, 32, ..., 2-launch graphs. Batches that
 * launch plainly (see pbn_step): a no-op. n_updates < 2 is a no-op; above PBN_STEP_PREPARE_MAX,
 * PBN_E_INVALID. A failed capture is not an error (pbn_step then launches without it). */
#define PBN_STEP_PREPARE_MAX 4096
int pbn_step_prepare(pbn_batch *b, uint32_t n_updates);
/* Philox mode, one launch applying n_updates in registers; bit-identical to pbn_step. */
int pbn_rollout(pbn_batch *b, uint32_t n_updates);
/* Replay mode: node_idx [T][B] (randint result) and k53 [T][B] (random() * 2^53), host arrays. */
int pbn_step_replay(pbn_batch *b, const uint32_t *node_idx, const uint64_t *k53, uint32_t n_updates);
/* Forced node (replaces Graph.step(i=k), base.py:306-308: `i = randint(...) if i is None else i`):
 * node_idx [T][B] host array (PROB_TABLE: >= 1); update t of env e updates node node_idx[t][e] with
 * the choice word of the Philox step draw pbn_step would have used for that update (its node word
 * is discarded), and the batch's update counter advances by T like pbn_step's. Out-of-range
 * indices: PBN_E_RANGE, nothing launched. Synchronous. */
int pbn_step_forced(pbn_batch *b, const uint32_t *node_idx, uint32_t n_updates);
/* MT mode: seeds [B] (host). random.seed(seeds[e]) (and np.random.seed for PROB_TABLE).
 * init_state 1 also runs Graph.genRandState / PBN.reset(None) from that stream. */
int pbn_mt_seed(pbn_batch *b, const uint64_t *seeds, int init_state);
int pbn_mt_step(pbn_batch *b, uint32_t n_updates); /* asynchronous; seeds >= 2^32 rejected for PROB_TABLE */

/* ---- multi-flip until-attractor env step: PBNTargetMultiEnv.step (pbn_target_multi.py:119-154) ---- */
int pbn_envcfg_create(const pbn_net *net, const pbn_envcfg_desc *desc, pbn_envcfg **out);
void pbn_envcfg_destroy(pbn_envcfg *cfg);
/* PBNTargetMultiEnv.reset (:227-259), Philox mode: envs with mask[e] != 0 (mask NULL = all)
 * get a reset cube chosen uniformly, '*' bits drawn fair, n_steps = 0. */
int pbn_env_reset(pbn_batch *b, const pbn_envcfg *cfg, const uint8_t *mask);
/* Same on the device, asynchronous: d_mask device uint8 [B] (NULL = all envs). */
int pbn_env_reset_device(pbn_batch *b, const pbn_envcfg *cfg, const uint8_t *d_mask);
int pbn_set_n_steps(pbn_batch *b, const int64_t *n_steps);  /* host [B] */
int pbn_get_n_steps(pbn_batch *b, int64_t *n_steps);        /* host [B] */
/* Host arrays: actions [B][A]; outputs obs [B][W], reward [B], flags [B], n_updates [B] (any may be NULL). */
int pbn_env_step_multi(pbn_batch *b, const pbn_envcfg *cfg, const int32_t *actions, int A, int dedup, int offset,
                       uint32_t update_cap, uint64_t *obs, int32_t *reward, uint8_t *flags, uint32_t *n_updates);
/* Device arrays on the batch's device (e.g. torch tensors); asynchronous. */
int pbn_env_step_multi_device(pbn_batch *b, const pbn_envcfg *cfg, const int32_t *d_actions, int A, int dedup,
                              int offset, uint32_t update_cap, uint64_t *d_obs, int32_t *d_reward, uint8_t *d_flags,
                              uint32_t *d_n_updates);
/* n_steps consecutive env steps in one launch (open-loop trajectory collection): device arrays
 * d_actions [n_steps][B][A], outputs [n_steps][B][W] / [n_steps][B]; identical to n_steps calls of
 * pbn_env_step_multi_device with the actions' slices (same Philox draws, env_call_count += n_steps).
 * An env step with an out-of-range action is skipped for that env (error flag set, outputs left). */
int pbn_env_rollout_multi_device(pbn_batch *b, const pbn_envcfg *cfg, uint32_t n_steps, const int32_t *d_actions,
                                 int A, int dedup, int offset, uint32_t update_cap, uint64_t *d_obs, int32_t *d_reward,
                                 uint8_t *d_flags, uint32_t *d_n_updates);
/* Replay mode (parity): draw_offsets [B+1] (int64), draws_i / draws_k the reference's draws, host arrays. */
int pbn_env_step_multi_replay(pbn_batch *b, const pbn_envcfg *cfg, const int32_t *actions, int A, int dedup,
                              int offset, const int64_t *draw_offsets, const uint32_t *draws_i,
                              const uint64_t *draws_k, uint64_t *obs, int32_t *reward, uint8_t *flags,
                              uint32_t *n_updates);

/* ---- synchronous update: Graph.synch_step (base.py:286-303), Philox mode ----
 * every node from the pre-step snapshot, each with its own random(); perturb_gap_thr [N]
 * (T_k = floor((1-p)^k 2^32), NULL = perturbations off): if any node is perturbed, the
 * perturbed nodes flip and no update happens in that step (base.py:288-295). */
int pbn_synch_step(pbn_batch *b, uint32_t n_steps, const uint32_t *perturb_gap_thr);

/* ---- steady-state distribution: compute_ssd_hist / _ssd_run (gym_PBN/utils/eval.py:20-103) ----
 * Every env runs `iters` iterations of: count the bucket of target_nodes (first = MSB), flip each
 * node with probability p, one async transition (Philox). flip_gap_thr [N]: T_k = floor((1-p)^k 2^32),
 * k = 1..N (NULL: no flips). hist [2^n_targets] host counts, ACCUMULATED (+=). n_targets <= 12. */
int pbn_ssd_run(pbn_batch *b, const int32_t *target_nodes, int n_targets, const uint32_t *flip_gap_thr,
                uint32_t iters, uint64_t *hist);

/* ---- measurement: HIP events on the batch stream. mode 1: a pair around every kernel launch;
 *      mode 2: one region from before the first launch to after the last (launch gaps included) ---- */
int pbn_timing_enable(pbn_batch *b, int enable);
int pbn_timing_read(pbn_batch *b, double *kernel_ms, uint64_t *launches); /* syncs, then resets */
/* mode 1 only: each timed launch's kernel ms in launch order (up to cap; *launches = how many were timed);
 * syncs, then resets like pbn_timing_read. Lets a timed loop keep per-launch figures without host reads
 * inside it. */
int pbn_timing_read_each(pbn_batch *b, double *ms_each, uint64_t cap, uint64_t *launches);
/* Envs handed from a tail-mode wave to an idle one during the last R6 env-step launch (env_kernel 4;
 * 0 when the hand-off was off). Syncs the batch stream. Diagnostics: the reference has no counterpart
 * (its until-attractor loop, pbn_target_multi.py:135-146, runs one env in one process). */
int pbn_env_handoffs(pbn_batch *b, uint32_t *count);
/* Tail helpers recruited during the last R6 env-step launch (env_kernel 4): idle waves of a workgroup that
 * prepared a long tail session's blocks ahead of the session wave (draws, records, writer masks; the session
 * wave only resolves). Syncs the batch stream. Diagnostics; PBNSIM_ENV_HELPERS=0 turns them off. */
int pbn_env_tail_helpers(pbn_batch *b, uint32_t *count);
/* The last R6 launch's tail counters, stats[4]: envs handed off, helpers recruited, tail blocks the
 * sessions read from their helpers' rings, and of those the blocks not yet written when the session reached
 * them (the session waited). Syncs the batch stream. Diagnostics. */
int pbn_env_tail_stats(pbn_batch *b, uint32_t *stats);
/* The last R6 launch's grid-pool counters, stats[4] (env_kernel 4 with the hand-off on; on by default for fused
 * launches and update caps >= 16,384, PBNSIM_ENV_GRID_STEAL=0/1 forces it): envs a tail wave handed to a workgroup
 * that had run out of work (anywhere on the GPU), tickets those workgroups took, waits given up (0 unless a launch
 * failed with PBN_E_HIP), the live count at the launch's end (0). Syncs the batch stream. Diagnostics. A given-up
 * wait drops the env it waited for: host-path env calls return PBN_E_HIP at once, device-path launches
 * (pbn_env_step_multi_device, pbn_env_rollout_multi_device) at the next pbn_sync. */
int pbn_env_grid_stats(pbn_batch *b, uint32_t *stats);

/* ---- attractor discovery: Graph.getNextStates / genSTG (base.py:221-242) + findAttractors (base.py:398-399) ----
 * The reference enumerates all 2^N states on the host ("too big for PBN > 10") and otherwise shells out to the
 * cabean binary. Here a pbn_reach is an exact set of packed states on the device, grown by reachability in the
 * SUPPORT GRAPH of a network.
 * PREDICTOR_MIX: x -> x ^ (1 << i) iff some live predictor of node i outputs 1 - x_i at
 * x (getNextStates keeps an edge when prob > 0). A predictor is live iff its selection interval on the 53-bit
 * grid is non-empty (pred_thr, the last threshold taken as 2^53) -- the rule is defined on the 53-bit thresholds,
 * not on the Philox stream's 32-bit choice grid.
 * PROB_TABLE: with T = thr[entry of node i's table at x] = ceil(p * 2^53), x -> x ^ (1 << i) iff (x_i = 0 and
 * T > 0) or (x_i = 1 and T < 2^53) -- exactly the reference's prob_true > 0. / prob_true < 1. (pbn.py:186-199): a
 * double p > 0 has ceil(p * 2^53) >= 1, a double p < 1 has p * 2^53 <= 2^53 - 1 with no rounding. The family has
 * two graphs and the caller names one: PBN_TABLE_GRAPH_STG, nodes 0 .. N-1 may move (PBN._compute_next_states, the
 * graph behind PBNEnv.compute_attractors); PBN_TABLE_GRAPH_STEP, nodes 1 .. N-1 only (the graph PBN.step walks,
 * pbn.py:90 randint(1, N-1); reset clears node 0).
 * An attractor is a terminal strongly connected component
 * (nx.attracting_components on the reference's STG); gym_pbn_amd/attractors.py finds them with these calls.
 * One pbn_reach = one device + one HIP stream; calls on it are synchronous and must be serialised by the caller. */
#define PBN_REACH_MAX_STATES ((uint64_t)1 << 28)
typedef struct {
    int32_t n_nodes, n_words, device;
    int32_t complete;      /* last closure: 1 = fixed point reached, 0 = it stopped at capacity */
    uint64_t max_states;   /* live states the set accepts */
    uint64_t table_slots;  /* open-addressing slots: the power of two >= 2 * max_states (>= 64) */
    uint64_t key_capacity; /* key entries, live and dead (an entry that lost a publish race is dead until a later
                              BFS level takes it again) */
    uint64_t n_states;     /* live states */
    uint64_t n_entries;    /* key entries in use */
    int32_t kind;          /* the network's PBN_KIND_* */
    int32_t table_graph;   /* PBN_TABLE_GRAPH_* of a PROB_TABLE set, 0 for PREDICTOR_MIX */
} pbn_reach_info;
/* PREDICTOR_MIX networks. PROB_TABLE networks: PBN_E_UNSUPPORTED (their set takes a graph: pbn_reach_create_table).
 * device < 0: PBN_E_RANGE. */
int pbn_reach_create(const pbn_net *net, int device, uint64_t max_states, pbn_reach **out);
/* PROB_TABLE networks: the set over the support graph `graph` (PBN_TABLE_GRAPH_STG / _STEP); every other
 * pbn_reach_* call works on the result as on a predictor-mix set. A PREDICTOR_MIX network or an unknown graph:
 * PBN_E_INVALID. The kernels stage the whole network image in LDS (TT-200: 28.8 KiB); an image that does not fit
 * what they request is refused here with PBN_E_UNSUPPORTED. */
int pbn_reach_create_table(const pbn_net *net, int device, uint64_t max_states, int32_t graph, pbn_reach **out);
void pbn_reach_destroy(pbn_reach *r);
int pbn_reach_get_info(const pbn_reach *r, pbn_reach_info *info);
/* The edge rule alone (base.py:221-242, one state's row of getNextStates): host states [S][W] -> masks [S][W], bit i
 * set iff node i can flip at that state. Does not touch the set. */
int pbn_reach_unstable(pbn_reach *r, const uint64_t *states, uint64_t n_states, uint64_t *masks);
/* genSTG restricted to what the seeds reach (base.py:221-242): clears the set, inserts seeds [S][W] and expands to
 * the fixed point, one launch sequence per BFS level. *count = states in the set; *complete = 0 when max_states (or
 * the key array) was reached first -- a normal return (PBN_OK), the set then holds the states seen so far. */
int pbn_reach_closure(pbn_reach *r, const uint64_t *seeds, uint64_t n_seeds, uint64_t *count, int32_t *complete);
/* Marks every state of the set that reaches `state` [W] inside the set (backward BFS over the same edges; with a
 * complete closure F of s, |marked| == |F| iff F is an attractor, findAttractors base.py:398-399). Earlier marks
 * are dropped. `state` not in the set: PBN_E_INVALID. *n_marked counts `state` itself. */
int pbn_reach_mark_backward(pbn_reach *r, const uint64_t *state, uint64_t *n_marked);
/* Read-back (base.py:398-399 returns the components as state lists): states [n][W] and marks [n] (1 = marked by the
 * last pbn_reach_mark_backward), in an order that stays fixed until the next closure; either may be NULL. capacity = rows the arrays hold; both NULL
 * just returns *n_states. */
int pbn_reach_read(pbn_reach *r, uint64_t *states, uint32_t *marks, uint64_t capacity, uint64_t *n_states);
/* Hull cube of the set (base.py:398-399's components as one cabean-style cube): all_words / any_words [W] = AND / OR
 * over all states; node i is fixed in the hull iff bit i of all ^ any is 0. Valid for an incomplete closure too. */
int pbn_reach_hull(pbn_reach *r, uint64_t *all_words, uint64_t *any_words);

/* ---- exact state sets: `state in attractor` / `state in target_nodes` (pbn_env.py:57-59, 161) for a whole batch ----
 * The reference envs keep their attractors and targets as Python sets of state tuples. A pbn_stateset is the same
 * thing for packed states: an exact, read-only, labelled set that a kernel can query (csrc/pbn_stateset.hpp has
 * the one definition of its layout and walk, for host and kernels). Open addressing, linear probing, table_slots =
 * the power of two >= 2 * n_states (at least 64); label = the caller's int per state (e.g. the attractor's index).
 * Bits past node N-1 must be zero in members (PBN_E_INVALID) and in queries (such a query is no member). */
#define PBN_STATESET_MAX_STATES ((uint64_t)1 << 24)
typedef struct pbn_stateset pbn_stateset;
typedef struct {
    int32_t n_nodes, n_words, device; /* device -1: host copy only */
    uint64_t n_states;                /* distinct members */
    uint64_t table_slots;
    uint32_t max_probe;               /* the longest walk of any member (1 = at its home slot; 0: the empty set) */
} pbn_stateset_info;
/* states [S][W] host, labels [S] (NULL = all 0), S <= PBN_STATESET_MAX_STATES. Built on the host, sequentially, in
 * input order (a deterministic layout). A duplicate row with the same label is dropped; with another label, or a
 * label < 0: PBN_E_INVALID. device >= 0: host copy + upload; device == -1: host copy only (the pbn_net_unstable
 * precedent: pins the definition on a machine without a GPU; device calls then return PBN_E_STATE). */
int pbn_stateset_create(int32_t n_nodes, int device, const uint64_t *states, const int32_t *labels, uint64_t n_states,
                        pbn_stateset **out);
void pbn_stateset_destroy(pbn_stateset *s);
int pbn_stateset_get_info(const pbn_stateset *s, pbn_stateset_info *info);
/* Host lookup over the host copy: labels [n] = the label of states [n][W], -1 for a non-member. */
int pbn_stateset_lookup(const pbn_stateset *s, const uint64_t *states, uint64_t n, int32_t *labels);
/* Device lookup, one launch: d_labels [B] int32 (device) = labels of the batch's state (d_words NULL) or of device
 * words [B][W] (16-byte aligned). Asynchronous, on the batch's stream. Set and batch on different devices or with
 * different n_nodes: PBN_E_INVALID; a host-only set: PBN_E_STATE. */
int pbn_stateset_lookup_device(pbn_batch *b, const pbn_stateset *s, const void *d_words, int32_t *d_labels);

/* ---- PBN-v0 on the device: PBNEnv.step / _get_reward (pbn_env.py:125-188) for every env in one launch ----
 * PROB_TABLE batches only (PREDICTOR_MIX: PBN_E_UNSUPPORTED). Device arrays, asynchronous, on the batch's stream.
 * d_actions [B] int32: 0 = none, a in [1, N-1] flips node a (PBNEnv flips `action`, :141-142); then one PBN.step
 * update with exactly the draw pbn_step would make (the batch's update counter advances by 1, so pbn_flip +
 * pbn_step(1) and this call give the same state bit for bit, and the calls mix freely); then per env
 * terminated = state in target, reward = terminated ? reward_target : -(step_cost + (a != 0 ? action_cost : 0))
 * (the reference's literals: 20, 4, 1), flags = PBN_FLAG_TERMINATED or 0 (PBN-v0 never truncates).
 * d_obs [B][W] (the state after the step) and d_labels [B] (the target set's label, -1 outside) may be NULL.
 * An env whose action is outside [0, N-1] is skipped whole -- no flip, no update, its outputs left as they were --
 * and noted in a sticky device flag (the pbn_flip_device convention): check 1 waits, returns PBN_E_RANGE if the flag
 * is set and clears it; check 0 returns at once. The update counter advances either way. */
int pbn_tenv_step_device(pbn_batch *b, const pbn_stateset *target, const int32_t *d_actions, int32_t reward_target,
                         int32_t step_cost, int32_t action_cost, int check, uint64_t *d_obs, int32_t *d_reward,
                         uint8_t *d_flags, int32_t *d_labels);
/* Envs with d_mask[e] != 0 (NULL = all) take a state drawn uniformly from d_states [n_states][W] (device, 16-byte
 * aligned; e.g. the attracting states), node 0 cleared as PBN.reset does (pbn.py:118). Draw: Philox stream 9,
 * counter {0, reset_count, global env id}, row = mulhi(word 0, n_states); reset_count advances by 1 per call
 * (modulo 2^32). n_states == 0 or >= 2^32: PBN_E_INVALID. */
int pbn_tenv_reset_device(pbn_batch *b, const uint64_t *d_states, uint64_t n_states, const uint8_t *d_mask);

/* ---- the macro-action envs on the device: PBNSampledDataEnv.step (sampled_data.py:52-88) and
 * PBNSelfTriggeringEnv.step (self_triggering.py:56-92) for every env in one launch ----
 * PROB_TABLE batches only. Device arrays, asynchronous, on the batch's stream. Env e repeats, for i = 0, 1, ...:
 * flip node a - 1 if a = d_actions[e] != 0 (both reference envs flip `action - 1`, so node 0 can be flipped here;
 * PBN-v0 above flips node `action`); one PBN.step update with exactly the draw pbn_step would make for update
 * update_count + i; terminated_i = state in target; r_i = terminated_i ? reward_target : -(step_cost + (a != 0 ?
 * action_cost : 0)). After k rounds the state is what k rounds of pbn_flip (offset 1) + pbn_step(1) give.
 *   PBN_MACRO_INTERVAL: d_limit[e] in [1, t_max] rounds; d_reward_i32[e] = the sum of r_i.
 *   PBN_MACRO_TRIGGER:  d_limit[e] = p in [1, 10], the stop probability in tenths. The env stops after round i if
 *     k53 <= d_stop_thr[p] or i + 1 == t_max, with k53 = (w0 >> 5) << 26 | w1 >> 6 from the Philox call of stream
 *     10, counter {lo, hi of update_count + i, global env id}. d_stop_thr: 11 values floor((p / 10) * 2^53), entry 0
 *     unused, which makes the compare the reference's uniform(0, 1) <= p / 10. d_reward_f64[e] = the sum of
 *     d_gpow[i] * r_i accumulated in order from 0.0, one IEEE multiply and one IEEE add per round (never fused);
 *     d_gpow: t_max doubles, gamma ** i. Both tables are the caller's device memory.
 * The mode's reward array and its tables must be given, the other mode's may be NULL. d_flags [B]:
 * PBN_FLAG_TERMINATED iff the LAST round's state is in the target (what the reference returns), never truncated.
 * Optional (NULL to skip): d_obs [B][W] the final state, d_interval [B] the rounds run, d_first_hit [B] the first i
 * with terminated_i or -1, d_labels [B] the target set's label of the final state.
 * An env whose action is outside [0, N] or whose limit is outside its range is skipped whole -- state and outputs
 * left as they were -- and noted in pbn_tenv_step_device's sticky flag; `check` as there.
 * The batch's update counter advances by t_max, not by the longest run of rounds (which the host does not know),
 * and also when an env was refused: the next call's draws stay disjoint from this one's, and the call mixes freely
 * with pbn_step, pbn_flip and pbn_tenv_step_device. mode or t_max outside their range: PBN_E_INVALID. */
enum { PBN_MACRO_INTERVAL = 0, PBN_MACRO_TRIGGER = 1 };
#define PBN_TENV_MACRO_MAX_T 65536u
int pbn_tenv_macro_device(pbn_batch *b, const pbn_stateset *target, int mode, uint32_t t_max, const int32_t *d_actions,
                          const int32_t *d_limit, const double *d_gpow, const uint64_t *d_stop_thr,
                          int32_t reward_target, int32_t step_cost, int32_t action_cost, int check, uint64_t *d_obs,
                          int32_t *d_reward_i32, double *d_reward_f64, uint8_t *d_flags, int32_t *d_interval,
                          int32_t *d_first_hit, int32_t *d_labels);

/* ---- the until-attractor multi-flip env over an exact labelled state set: PBNTargetMultiEnv.step
 * (pbn_target_multi.py:119-154) with `tuple(state) in self.attracting_states` (:437-455, :489-492) as membership in
 * a pbn_stateset whose label is the attractor's index, and the target attractor chosen per env (the reference's
 * reset draws target_attractor_id per episode, :232-235) ----
 * Both network kinds. Device arrays, asynchronous, on the batch's stream; one launch per call.
 *
 * The set's hull (pbn_reach_hull's convention): all_words / any_words [W] = AND / OR over the members (the empty set:
 * the N-bit mask and 0); *max_label = the largest label (-1: the empty set). Any of the three may be NULL. */
int pbn_stateset_get_hull(const pbn_stateset *s, uint64_t *all_words, uint64_t *any_words, int32_t *max_label);
/* Per env exactly pbn_env_step_multi_device's step (same arguments, same draws: Philox stream 3, counter {update >> 1,
 * env_call_count, global env id}; env_call_count advances by 1, so the two calls interleave freely), with "matches
 * some cube" read as "is a member of set": n_steps += 1; the flips of row d_actions[e] (A values, offset, dedup,
 * Python indexing); obs = the state after the flips; updates until the tested state is a member or update_cap updates
 * were made -- after update 1 the observation before the update is tested (:134; first_update_tested != 0: the state
 * after it, PBNTargetEnv.step), from update 2 on the state itself. Outputs: d_obs [B][W] the state tested last,
 * d_labels [B] (may be NULL) the set's label of it or -1 when the cap ended the loop, d_flags PBN_FLAG_TERMINATED iff
 * that label equals the env's target -- d_target_labels[e], or target_label for every env when d_target_labels is
 * NULL -- | PBN_FLAG_TRUNCATED iff n_steps == horizon | PBN_FLAG_CAPPED, d_reward = (terminated ? reward_success : 0)
 * - action_cost * (dedup ? distinct actions : A), d_n_updates the updates made.
 * An env whose row holds an action that names no node is skipped whole, as pbn_env_step_multi_device skips it --
 * state, n_steps and outputs left as they were -- and noted in a sticky device flag (pbn_env_set_check).
 * PBN_E_INVALID, before anything is launched or any counter moves: A < 1 (or > 4096, offset not 0 / 1), a set of
 * another n_nodes or device, a host-only set, target_label outside [0, the set's largest label] with d_target_labels NULL. */
int pbn_env_set_step_device(pbn_batch *b, const pbn_stateset *set, const int32_t *d_actions, int A, int dedup,
                            int offset, uint32_t update_cap, int32_t horizon, int32_t reward_success,
                            int32_t action_cost, int first_update_tested, int32_t target_label,
                            const int32_t *d_target_labels, uint64_t *d_obs, int32_t *d_reward, uint8_t *d_flags,
                            uint32_t *d_n_updates, int32_t *d_labels);
/* PBNTargetMultiEnv.reset (:227-259) over state lists: envs with d_mask[e] != 0 (NULL = all) take a state drawn
 * uniformly from their source attractor (the reference's state_attractor_id, :232-235) -- d_source_labels[e], or
 * source_label for every env when d_source_labels is NULL -- and n_steps = 0. d_rows [S][W] (device, 16-byte aligned)
 * holds the attractors' states ordered by label, d_row_off [n_labels + 1] uint32 (device) the first row of each.
 * Draw: Philox stream 9, counter {0, reset_count, global env id}, row = d_row_off[src] + mulhi(word 0, rows of src);
 * node 0 is cleared for PROB_TABLE networks only (PBN.reset, pbn.py:118). reset_count advances by 1 per call. An env
 * whose source is outside [0, n_labels) or names an attractor without rows is left untouched and noted in the sticky
 * flag. n_labels < 1: PBN_E_INVALID. */
int pbn_env_set_reset_device(pbn_batch *b, const uint64_t *d_rows, const uint32_t *d_row_off, int32_t n_labels,
                             int32_t source_label, const int32_t *d_source_labels, const uint8_t *d_mask);
/* Waits for the batch's stream; PBN_E_RANGE if an env was skipped by either call since the last check (the flag is
 * cleared: reported once). */
int pbn_env_set_check(pbn_batch *b);

/* ---- state census: statistical_attractors (pbn_target.py:538-560, pbn_target_multi.py:465-487), whose
 * `state_log[tuple(state)] += 1` over 100 resets x 1,000 steps becomes an exact device table of visit counts keyed by
 * the packed full state (W = 1..8 words, both network kinds), fed by every env of a batch in one launch ----
 * One uint64 count per distinct state, up to max_states of them (at most PBN_CENSUS_MAX_STATES = 2^24, what a
 * pbn_stateset takes); the hash table has the power of two >= 2 max_states slots, at least 64. Counts accumulate over
 * pbn_census_run_device calls until pbn_census_clear.
 * Overflow is counted, never silent: the census reports the first max_states states it took in, and a visit of any
 * other state adds to `dropped`. Guarantees:
 *   (a) n_states <= max_states;
 *   (b) sum of the counts + dropped == visits, exactly;
 *   (c) dropped == 0: every count is exact;
 *   (d) dropped > 0: every reported count is <= the true count of that state. Up to 2^19 states past max_states are
 *       still held (unreported, their visits counted as dropped), so that no state is inserted twice. Once those
 *       entries are used up too, or every slot of a state's probe sequence holds another state, a visit is dropped on
 *       the spot. Only then can a reported state's count fall short: a lane that finds no free entry looks at the
 *       slot once more, and a publish of the same state that lands after that second look is missed.
 * One census is fed by one batch at a time: the caller serialises pbn_census_* calls on a census, and two batches
 * feeding one census must not overlap (wait for the first batch's stream, or use one stream). */
typedef struct pbn_census pbn_census;
typedef struct {
    int32_t n_nodes, n_words, device; /* device -1: a host-only handle */
    uint64_t max_states, table_slots;
    uint64_t n_states; /* distinct states held */
    uint64_t visits;   /* sample points of every run since the last clear: n_envs x samples per run */
    uint64_t dropped;
} pbn_census_info;
#define PBN_CENSUS_MAX_STATES (1ull << 24)
#define PBN_CENSUS_MAX_UPDATES 65536u
/* The defaultdict(int) of pbn_target.py:546 / pbn_target_multi.py:473, empty. n_nodes outside [1, 512] or max_states
 * outside [1, PBN_CENSUS_MAX_STATES]: PBN_E_INVALID. device == -1: a host-only handle (the pbn_stateset_create
 * precedent): the argument checks of pbn_census_run_device run without a GPU, and the call then returns PBN_E_STATE. */
int pbn_census_create(int32_t n_nodes, int device, uint64_t max_states, pbn_census **out);
void pbn_census_destroy(pbn_census *c);
/* Empties the table and zeroes visits and dropped; waits for the last run first. */
int pbn_census_clear(pbn_census *c);
/* Waits for the stream the last run went to. */
int pbn_census_get_info(pbn_census *c, pbn_census_info *info);
/* The loop of pbn_target.py:548-556 (`state_log[tuple(state)] += 1; self.step(...)`) for every env of the batch, one
 * launch, asynchronous, on the batch's stream. Env e makes n_updates updates, update i with exactly the draw pbn_step
 * makes for update update_count + i of the env: afterwards the state is bit for bit pbn_step(n_updates)'s and the
 * batch's update counter has advanced by n_updates, so the call mixes freely with pbn_step, pbn_flip and the env
 * calls. "The state after i updates" is counted for i = first, first + stride, first + 2 stride, ... <= n_updates;
 * first = 0 counts the state as it was before the call (the reference logs before it steps); n_updates = 0 with
 * first = 0 counts the current state and moves nothing. mask_words (host [W], NULL = every node): the key is
 * state & mask, a projection onto a node subset.
 * PBN_E_INVALID, before anything is launched or any counter moves: n_updates above PBN_CENSUS_MAX_UPDATES (longer runs
 * loop on the host), stride == 0, first > n_updates, mask bits past node N-1, a batch of another n_nodes or device.
 * A host-only census: PBN_E_STATE. */
int pbn_census_run_device(pbn_batch *b, pbn_census *c, uint32_t n_updates, uint32_t first, uint32_t stride,
                          const uint64_t *mask_words);
/* `state_log.items()` (pbn_target.py:558): the states held [n][W] and their counts [n], in no particular order; waits
 * for the last run. *n_states is always set; with states and counts NULL nothing else happens; cap < *n_states:
 * PBN_E_INVALID. Either array may be NULL. */
int pbn_census_read(pbn_census *c, uint64_t *states, uint64_t *counts, uint64_t cap, uint64_t *n_states);
/* Measurement, no reference counterpart; either pointer may be NULL. *adds: count adds the runs issued since the last
 * clear. A lane adds once per run of equal consecutive keys, so adds / visits is the share of sample points that
 * touched memory. *entries: entries taken from the end of the key array since the last clear: the states held
 * (n_states, plus those past max_states) and the entries taken in vain by lanes that lost a publish race, at most one
 * per lane of a launch and handed out again by later launches. Waits for the last run. */
int pbn_census_get_stats(pbn_census *c, uint64_t *adds, uint64_t *entries);

/* ---- exact transition graph of a state set: Graph.getNextStates (bittner/base.py:221-242, `{next_state: prob}` of
 * one state; genSTG :199-218 builds the weighted graph from it), PBN._compute_next_states (common/pbn.py:186-199) and
 * PBCN._async_compute_next_states (common/pbcn.py:72-93) for truth tables, for every state of an enumerated set in
 * one launch ----
 * The reference loops over 2^N states in Python; here the set is whatever the caller enumerated (an attractor of
 * pbn_reach_*, a closure, a census' states), S <= PBN_STG_MAX_STATES rows, and the graph is two dense arrays:
 *   mass [S][N] uint64  the edge mass of node i at row s (pbn_net_edge_mass: an exact integer in [0, 2^53]);
 *   succ [S][N] int32   the row of x_s ^ (1 << i) where mass > 0 and that state is a member; -1 where mass > 0 and
 *                       it is not (a leak: the set is not closed under the dynamics); s itself where mass == 0 (no
 *                       edge, and no probe is made for it).
 * The probability of the edge is mass / (2^53 * n_movable): the updated node is drawn uniformly from the n_movable =
 * N - first_node nodes that may move (base.py:308 randint(0, N-1), getNextStates' 1 / len(state); pbn.py:131
 * randint(1, N-1) for PBN_TABLE_GRAPH_STEP). For PBN_TABLE_GRAPH_STG the uniform choice is this library's: the
 * reference's async STG carries prob_true unnormalised.
 * Both network kinds, W = 1..8 words. */
#define PBN_STG_MAX_STATES ((uint64_t)1 << 24)
#define PBN_STG_MAX_CELLS ((uint64_t)1 << 31)
typedef struct pbn_stg pbn_stg;
typedef struct {
    int32_t n_nodes, n_words, first_node, n_movable;
    int32_t device;      /* -1: a host-only handle */
    int32_t table_graph; /* PBN_TABLE_GRAPH_*, 0 for a predictor-mix network */
    uint64_t n_states;
    uint64_t leaks;      /* -1 entries written by pbn_stg_rows_device since the last pbn_stg_clear_leaks */
} pbn_stg_info;
/* states [S][W] host, 1 <= S <= PBN_STG_MAX_STATES; row r of the graph is states[r]. The handle keeps the states and a
 * pbn_stateset-style table over them whose label is the row index (csrc/pbn_stateset.hpp, built as pbn_stateset_create
 * builds it). A row given twice, or bits set past node N-1: PBN_E_INVALID. `graph` as for pbn_net_unstable:
 * PBN_TABLE_GRAPH_STG / _STEP for a PROB_TABLE network (anything else PBN_E_INVALID), ignored for PREDICTOR_MIX.
 * device == -1: a host-only handle (the pbn_stateset_create precedent): pbn_stg_get_info works, the argument checks of
 * pbn_stg_rows_device run without a GPU and the call then returns PBN_E_STATE. */
int pbn_stg_create(const pbn_net *net, int device, int32_t graph, const uint64_t *states, uint64_t n_states,
                   pbn_stg **out);
void pbn_stg_destroy(pbn_stg *g);
/* Waits for the rows launched so far (it reads the leak counter). */
int pbn_stg_get_info(pbn_stg *g, pbn_stg_info *info);
int pbn_stg_clear_leaks(pbn_stg *g);
/* Fills d_mass [n_rows][N] uint64 and d_succ [n_rows][N] int32 (device memory of the graph's device, 8- / 4-byte
 * aligned) for rows [first_row, first_row + n_rows), and adds the -1 entries it wrote to the leak counter. One launch
 * on the device's default stream, asynchronous. The caller chunks by rows, so its memory stays bounded: n_rows * N
 * above PBN_STG_MAX_CELLS is PBN_E_INVALID. Rows past S: PBN_E_RANGE; a NULL array: PBN_E_INVALID; a host-only
 * handle: PBN_E_STATE; n_rows == 0: nothing is launched. */
int pbn_stg_rows_device(pbn_stg *g, uint64_t first_row, uint64_t n_rows, void *d_mass, void *d_succ);

/* ---- Exact optimal control over a transition graph (csrc/pbn_control.hip): the per-sweep work of value
 * iteration for the single-flip MDP of PBNEnv.step + _get_reward (pbn_env.py:125-188) on the arrays above. The
 * reference trains agents against this MDP and has no code that solves it. An action is the no-op or the flip of one
 * allowed node; the flip is a map between rows of the set (nbr), the update that follows is the graph's law (mass,
 * succ). Values are float64; nbr and the action restriction are exact.
 * All four calls are one launch on the device's default stream, asynchronous, as pbn_stg_rows_device is. A NULL array:
 * PBN_E_INVALID; a host-only handle: PBN_E_STATE, decided after the argument checks. ---- */
#define PBN_STG_LOOKUP_MAX ((uint64_t)1 << 32)
/* Fills d_nbr [n_rows][N] int32 for rows [first_row, first_row + n_rows): the row of x_s ^ (1 << i) whatever the mass of
 * that flip under the dynamics; -1 where that state is no row, and -1 without a probe for a node whose bit in
 * action_mask (host [W] words, NULL = every node) is clear. A mask bit past node N-1: PBN_E_INVALID; rows past S:
 * PBN_E_RANGE; n_rows == 0: nothing is launched. */
int pbn_stg_flip_rows_device(pbn_stg *g, uint64_t first_row, uint64_t n_rows, const uint64_t *action_mask, void *d_nbr);
/* The fused pull over all S rows: d_out[s] = v[s] + (sum_i (double)mass[s][i] * (v[succ[s][i]] - v[s])) * 2^-53 /
 * n_movable, from d_mass [S][N] uint64, d_succ [S][N] int32 (what pbn_stg_rows_device wrote for the whole graph) and
 * d_v [S]. With d_pen [S] it also writes d_out_pen[s] = d_out[s] - cost * d_pen[s] (d_out_pen NULL then:
 * PBN_E_INVALID). d_out may not alias d_v. The sum of a row is taken in an order fixed by N alone: the result is
 * bit-identical from call to call and under any grid. A successor that is no row is read as "stays": the caller
 * checks that the set is closed (pbn_stg_info.leaks == 0). */
int pbn_stg_expect_device(pbn_stg *g, const void *d_mass, const void *d_succ, const double *d_v, double *d_out,
                          const double *d_pen, double cost, double *d_out_pen);
/* d_v[s] = max(d_u[s], max over nodes i with d_nbr[s][i] >= 0 of d_ua[d_nbr[s][i]]) and d_policy[s] = the arg max: -1
 * for the no-op, else the node; on a tie the no-op first, then the lowest node. d_v may not alias d_u or d_ua. */
int pbn_stg_backup_device(pbn_stg *g, const void *d_nbr, const double *d_u, const double *d_ua, double *d_v,
                          int32_t *d_policy);
/* d_rows[e] = the row of d_words[e] ([n][W] device words), -1 for a state that is no row: pbn_stateset_lookup_device's
 * kernel over the graph's own table. n above PBN_STG_LOOKUP_MAX: PBN_E_RANGE; n == 0: nothing is launched. */
int pbn_stg_lookup_device(pbn_stg *g, const void *d_words, uint64_t n, int32_t *d_rows);

/* ---- Absorption over a transition graph (csrc/pbn_absorb.hip): one Jacobi sweep of the first-hit
 * recursion over the arrays above, for n_cols columns at once. d_label [S] int32: -1 a transient row, k >= 0 a row of
 * class k (any labelled row is held: the classes are first-hit classes and need not be closed). For column c of row s,
 * with d_x and d_out [S][ld] float64, row-major:
 *   d_out[s][c] = d_x[s][c]                                                          where d_label[s] >= 0 (the same bits)
 *   d_out[s][c] = (d_x[s][c] + (sum_i (double)mass[s][i] * (d_x[t_i][c] - d_x[s][c])) * 2^-53 / n_movable) + src[c]
 *                 elsewhere, t_i = succ[s][i]; a successor that is no row is read as "stays", as in
 *                 pbn_stg_expect_device.
 * n sweeps from 1{label == k} with src 0 give P(first labelled row is hit within n updates, in class k); from
 * 1{label < 0} with src 0, P(no labelled row within n updates); from 0 with src 1, E[min(hitting time, n)]: the law of
 * "update until the state is in an attractor, at most update_cap times" (pbn_target_multi.py:133-146) from every row.
 * Columns [n_cols, ld) of d_out are not written. src: n_cols host doubles, NULL = all zero. The sum of a row is taken,
 * per column, in pbn_stg_expect_device's order, fixed by N alone: the result is bit-identical from call to call, under
 * any grid, and column c of a launch of several columns is bit-identical to the same column swept alone; with no
 * labelled row, n_cols == 1 and src 0 it is pbn_stg_expect_device's (but -0.0 comes out +0.0: src is added). One launch on the device's default stream,
 * asynchronous. A NULL handle or array, n_cols outside [1, PBN_STG_ABSORB_MAX_COLS], ld < n_cols, or d_out == d_x (a
 * Jacobi sweep reads every row it has not yet written): PBN_E_INVALID; a host-only handle: PBN_E_STATE, decided after
 * the argument checks. ---- */
#define PBN_STG_ABSORB_MAX_COLS 8
int pbn_stg_absorb_device(pbn_stg *g, const void *d_mass, const void *d_succ, const int32_t *d_label,
                          const double *d_x, double *d_out, uint32_t n_cols, uint64_t ld, const double *src);

/* ---- The max over multi-flip action sets (csrc/pbn_flipset.hip, csrc/pbn_flipset_rule.hpp): the action
 * of PBNTargetMultiEnv.step (pbn_target_multi.py:105-131) is a set F of 1 <= |F| <= A distinct allowed nodes, worth
 * m[row of s ^ F] - cost * |F| with m [S] the worth of arriving at a row. d_nbr [S][N] int32 is what
 * pbn_stg_flip_rows_device wrote for the allowed nodes over a set that is closed under those flips (-1 exactly on the
 * nodes that are not allowed: the caller checks it; a cell that is no row adds nothing). A summary T_j is d_base [S][2]
 * float64 and d_tag [S][2] int32, 16- and 8-byte aligned: the best two entries with distinct end rows among the ends
 * within j flips of each row, the better first; tag = end row | flips << 24, -1 none; base = m[end]. The order: larger
 * base - cost * flips (one multiply, one subtract, not contracted), then fewer flips, then the lower end row.
 * Both calls are one launch on the device's default stream, asynchronous; results are bit-identical from call to call
 * and under any grid. A NULL handle or array, a cost that is negative, NaN or infinite, or an output summary that
 * aliases the input: PBN_E_INVALID; a host-only handle: PBN_E_STATE, decided after the argument checks. ---- */
#define PBN_STG_FLIPSET_MAX_FLIPS 15
/* T_j from T_{j-1}: d_out[s] = top-two-distinct of d_in[s] and, with one more flip, d_in[d_nbr[s][i]] for every i.
 * d_in_base and d_in_tag NULL: level 0 -> 1, T_0[s] = (s, 0, d_m[s]) (d_m is not read otherwise and may be NULL then).
 * At most PBN_STG_FLIPSET_MAX_FLIPS levels fit the tag. */
int pbn_stg_flipset_level_device(pbn_stg *g, const void *d_nbr, const double *d_m, double cost, const double *d_in_base,
                                 const int32_t *d_in_tag, double *d_out_base, int32_t *d_out_tag);
/* The best action from T_A: the first entry whose end is not the row itself (the empty set is no action), so d_v[s] =
 * its value, d_policy_end[s] its end row, d_policy_flips[s] its flip count; F = states[s] ^ states[policy_end[s]].
 * noop_cost (a host double, NULL: none) makes the empty set an action worth d_m[s] - *noop_cost, taken on a tie:
 * policy_end = s, policy_flips = 0. A row with no action at all: -inf, -1, 0. */
int pbn_stg_flipset_select_device(pbn_stg *g, const double *d_base, const int32_t *d_tag, const double *d_m, double cost,
                                  const double *noop_cost, double *d_v, int32_t *d_policy_end, int32_t *d_policy_flips);

#ifdef __cplusplus
}
#endif
#endif /* PBN_ABI_H */
