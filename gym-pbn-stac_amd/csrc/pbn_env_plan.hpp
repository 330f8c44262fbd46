// pbn_env_plan.hpp -- the decision half of an R6 launch (k_env / k_env_grp), from plain integers: kernel mode,
// lanes per env, draw-round chunk, lane limit, grid, the workgroup hand-off and the grid pool, and the LDS bytes
// of a workgroup (env_lds_bytes: its one definition, for the plan, the occupancy query and the launch). Uploads,
// memsets and the launch itself stay with the caller (pbn_abi_env.cpp env_launch), and so does the occupancy
// query: env_plan takes it as a function.
//
// No HIP and no other project header but the shared structs: tests/host/env_plan_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>

#include "pbn_params.hpp"

namespace pbn {

// LDS bytes of one workgroup of the R6 kernel: the image (image_bytes: with the env records' shift, if any), the
// state planes or group rows, and the cooperative-draw modes' per-wave draw buffers.
inline uint32_t env_lds_bytes(int W, uint32_t image_bytes, int mode, int grp, uint32_t chunk = ENV_CHUNK_LARGE) {
    if (mode == ENV_MODE_GROUP) return image_bytes + 8u * (uint32_t)W * (BLOCK / (uint32_t)grp);  // one row per group
    const uint32_t planes = image_bytes + 8u * (uint32_t)W * ENV_BLOCK;
    // ENV_MODE_TAIL: 16 B of workgroup hand-off control (WgCtl) after the per-wave draw buffers
    const bool coop = mode == ENV_MODE_COOP || mode == ENV_MODE_TAIL;
    return coop ? planes + (ENV_BLOCK / 64) * env_gen_wave_bytes(chunk) + (mode == ENV_MODE_TAIL ? 16u : 0u) : planes;
}

// Workgroups of `block` threads for `items` work items: at most the resident count (n_cu x bpc), at least one.
inline int resident_grid(uint64_t items, int n_cu, int bpc, int block) {
    const uint64_t need = (items + block - 1) / block;
    const uint64_t cap = (uint64_t)n_cu * (uint64_t)bpc;
    return (int)std::max<uint64_t>(std::min<uint64_t>(need, cap), 1);
}

// The PBNSIM_ENV_* knobs env_plan reads (measurement / tests; read_knobs, pbn_abi.cpp). The grid pool's own knobs
// stay in Knobs (pbn_host.hpp); of those the plan reads PBNSIM_ENV_GRID_STEAL (EnvPlanIn::grid_steal).
struct EnvKnobs {
    bool no_gen = false;        // PBNSIM_ENV_NO_GEN: no cooperative draw generation
    int group = 0;              // PBNSIM_ENV_GROUP: lanes per env (1 = lane mode), 0 = by batch size
    int bpc = 0;                // PBNSIM_ENV_BPC: cap on resident workgroups per CU, 0 = none
    int chunk = 0;              // PBNSIM_ENV_CHUNK: draw-round chunk 32 / 48 of the cooperative-draw kernels, 0 = auto
    int grid_cap = 0;           // PBNSIM_ENV_GRID: the R6 kernel's workgroups (tests: lane refill, hand-offs), 0 = by size
    int tail = -1;              // PBNSIM_ENV_TAIL: the R6 kernel's tail-mode threshold (live envs per wave), -1 = default
    int lane_limit = 0;         // PBNSIM_ENV_LANES: lanes per wave taking envs in the tail-mode kernel, 0 = auto
    bool steal = true;          // PBNSIM_ENV_STEAL=0: no hand-off of tail envs between a workgroup's waves (k_env, ENV_MODE_TAIL)
    bool kernel_image = false;  // PBNSIM_ENV_KERNEL_IMAGE=1: k_env builds its LDS image (no host-built image)
};

// Everything env_plan reads.
struct EnvPlanIn {
    // the batch
    uint64_t B = 0;
    int W = 0, N = 0, kind = 0, n_cu = 0;
    // the env config (pbn_envcfg): L.* of its NetLayout, rs = thr32_layout(L).rs (record slots per node)
    bool counters_ok = false;  // <= 8 cubes, each caring about <= 255 nodes: the byte counters apply
    int H = 0;                 // cubes
    uint32_t pmax = 0, image_bytes = 0, off_rec = 0, off_cubes = 0, rs = 0;
    // the call
    bool replay = false;
    uint32_t cap = 0, n_calls = 1;
    // the knobs
    EnvKnobs knob;
    int grid_steal = -1;  // Knobs::env_grid_steal
};

// What env_plan decides for one R6 launch; the batch keeps the last launched one (pbn_batch_get_info reads it).
struct EnvPlan {
    int mode = -1;            // EnvArgs::mode, an EnvMode (pbn_params.hpp); pbn_batch_info.env_kernel
    int grp = 0;              // lanes per env
    uint32_t erec_shift = 0;  // LDS bytes the 16-B env records add (ENV_MODE_COOP / _TAIL)
    uint32_t chunk = 0;       // draw-round chunk (ENV_MODE_COOP / _TAIL)
    int bpc = 1;              // resident workgroups per CU
    uint32_t lane_limit = 0, tail_max = 0;
    int grid = 0;             // workgroups
    bool host_image = false;  // the kernel stages the host-built image (env_gen_image)
    bool handoff = false;     // tail hand-off between a workgroup's waves
    bool gpool = false;       // grid-wide hand-off (grid pool)
    int error = 0;            // hipError_t of a failed occupancy query: no launch
};

// Lanes per env for the R6 kernel: 1 (lane mode, k_env) while the batch fills the chip
// several times over; group mode where it does not and the until-attractor tail would
// leave lanes idle (measured: DESIGN.md section 6).
// Per-step call, Bittner-200, 1 MI355X (256 CUs): G = 8 beats lane mode up to 32k envs (0.21 vs
// 0.33 ms at B = 1, 0.88 vs 1.99 ms at 8k, 1.85 vs 2.04 ms at 32k) and loses from 64k on (2.31 vs
// 2.07 ms; 131k: 3.28 vs 2.60 ms) -- the crossover sits near 48k envs.
// Group mode (G = 8 lanes per env) for small batches -- except where the tail kernel (k_env ENV_MODE_TAIL:
// <= 4 cubes and its 16-B env records fit) applies: its tail mode with one env per wave
// (env_lane_limit) is faster at every batch size measured (profiles/r03_r6_lanes_sweep.json)
inline int env_group_size(uint64_t B, int n_cu, bool tail_kernel) {
    if (tail_kernel) return 1;
    return B * 8 <= (uint64_t)n_cu * 1536 ? 8 : 1;
}

// Reads `in` and queries occupancy -- occupancy(mode, grp, image_bytes, chunk, &blocks_per_cu) returns a hipError_t
// as int --; writes no buffer and does not touch a stream. p.error: a failed occupancy query.
template <class Occ>
EnvPlan env_plan(const EnvPlanIn& in, Occ&& occupancy) {
    EnvPlan p;
    const EnvKnobs& k = in.knob;
    // without cooperative draws: the byte counters where they apply, else every cube matched after a change
    const int plain = in.counters_ok ? (int)ENV_MODE_COUNTERS : (int)ENV_MODE_CUBES;
    // cooperative draw generation: predictor mix, Philox, record index fits the u16 entry
    int mode = (in.counters_ok && !in.replay && in.kind == KIND_PREDICTOR_MIX && in.pmax <= 16 && in.N <= 512 &&
                !k.no_gen)
                   ? (int)ENV_MODE_COOP
                   : plain;
    // cooperative-draw mode keeps 16-B env records in LDS where the 8-B predictor records were
    // (env_record_words, pbn_params.hpp): the tables after them move up by erec_shift. Whether they fit is
    // decided first, so that the group-size rule below knows whether the tail kernel (ENV_MODE_TAIL) applies
    uint32_t erec_shift = 0;
    bool erec_fits = false;
    if (mode == ENV_MODE_COOP) {
        // rows of rs records (thr32_layout: tp4 + 1 slots at least, for the saturated choice)
        const uint32_t nrec = (uint32_t)in.N * in.rs;
        erec_shift = in.off_rec + 16u * nrec - in.off_cubes;
        erec_fits = nrec <= 65535u &&
                    env_lds_bytes(in.W, in.image_bytes + erec_shift, ENV_MODE_COOP, 1, ENV_CHUNK_SMALL) <= ENV_LDS_MAX;
    }
    // group mode (k_env_grp: G lanes per env, G updates per round trip; its rows need no env records)
    int grp = 1;
    if (mode == ENV_MODE_COOP && in.N <= 256) {
        grp = k.group ? k.group : env_group_size(in.B, in.n_cu, erec_fits && in.H <= 4);
        if (grp != 2 && grp != 4 && grp != 8) grp = 1;
        if (grp > 1) mode = ENV_MODE_GROUP;
    }
    if (mode == ENV_MODE_COOP) {
        if (!erec_fits)
            mode = plain;  // too large for the u16 record index / one workgroup's LDS
        else if (in.H <= 4)
            mode = ENV_MODE_TAIL;  // the same kernel with one packed counter word (<= 4 cubes)
        // ENV_MODE_TAIL adds the workgroup hand-off control words: re-check the fit with the final mode
        if (mode == ENV_MODE_TAIL &&
            env_lds_bytes(in.W, in.image_bytes + erec_shift, ENV_MODE_TAIL, 1, ENV_CHUNK_SMALL) > ENV_LDS_MAX)
            mode = plain;
    }
    const bool coop = mode == ENV_MODE_COOP || mode == ENV_MODE_TAIL;
    if (!coop) erec_shift = 0;
    const uint32_t img = in.image_bytes + erec_shift;
    // PBNSIM_ENV_KERNEL_IMAGE=1: the kernel builds its LDS image itself (tests keep that path covered)
    p.host_image = coop && img % 16u == 0u && !k.kernel_image;
    int bpc = 1;
    uint32_t chunk = ENV_CHUNK_SMALL;
    if (coop) {
        // the draw-round chunk (pbn_params.hpp ENV_CHUNK_SMALL / _LARGE): the large one unless the small
        // one's draw buffers let more workgroups onto a CU and the launch is a throughput-bound fused run
        // (>= 16 env steps per env over a queue of >= 4 envs per lane of the large one's grid), or the large
        // one does not fit one workgroup's 64 KiB; PBNSIM_ENV_CHUNK=32 / 48 overrides
        int bpc_s = 1, bpc_l = 1;
        p.error = occupancy(mode, grp, img, ENV_CHUNK_SMALL, &bpc_s);
        const bool large_fits = env_lds_bytes(in.W, img, mode, 1, ENV_CHUNK_LARGE) <= ENV_LDS_MAX;
        if (large_fits && !p.error) p.error = occupancy(mode, grp, img, ENV_CHUNK_LARGE, &bpc_l);
        const uint64_t lanes_l = (uint64_t)in.n_cu * (uint64_t)bpc_l * ENV_BLOCK;
        const bool throughput = in.n_calls >= 16u && in.B >= 4u * lanes_l && bpc_s > bpc_l;
        chunk = large_fits && !throughput ? ENV_CHUNK_LARGE : ENV_CHUNK_SMALL;
        if (k.chunk == (int)ENV_CHUNK_SMALL || (k.chunk == (int)ENV_CHUNK_LARGE && large_fits)) chunk = (uint32_t)k.chunk;
        bpc = chunk == ENV_CHUNK_LARGE ? bpc_l : bpc_s;
    } else {
        p.error = occupancy(mode, grp, img, ENV_CHUNK_LARGE, &bpc);  // these modes have no draw buffers: any chunk
    }
    if (k.bpc) bpc = std::min(bpc, k.bpc);
    p.tail_max = k.tail >= 0 ? (uint32_t)k.tail : ENV_TAIL_DEFAULT;
    // tail-mode kernel: small batches (ENV_ONE_LANE_ENVS_PER_SLOT envs per wave slot) take one env per
    // wave at a time -- every wave resolves its env 64 updates per block and takes the next from the
    // queue when it is done (PBNSIM_ENV_LANES overrides; 64 = lane mode, the tail at the end)
    p.lane_limit = 64u;
    if (mode == ENV_MODE_TAIL) {
        const uint64_t slots = (uint64_t)in.n_cu * (uint64_t)bpc * (ENV_BLOCK / 64);
        if (k.lane_limit > 0)
            p.lane_limit = (uint32_t)k.lane_limit;
        else if (p.tail_max >= 1 && in.B <= ENV_ONE_LANE_ENVS_PER_SLOT * slots)
            p.lane_limit = 1u;
    }
    // lanes per env (group mode) or, with a lane limit, 64 / limit lane slots per env
    p.grid = resident_grid(p.lane_limit < 64u ? (in.B * 64u + p.lane_limit - 1u) / p.lane_limit : in.B * (uint64_t)grp,
                           in.n_cu, bpc, env_block(mode));
    // PBNSIM_ENV_GRID: exactly that many workgroups (at most the resident count; persistent waves: any grid
    // drains the counter, and surplus workgroups find the queue empty)
    if (k.grid_cap) p.grid = std::min(k.grid_cap, in.n_cu * bpc);
    // tail hand-off (k_env ENV_MODE_TAIL): a wave holding several envs in tail mode passes envs it has not
    // started on to idle waves of its workgroup (LDS). One lane per wave taking envs (small batches)
    // never holds two: off there
    p.handoff = mode == ENV_MODE_TAIL && k.steal && p.tail_max >= 1u && p.lane_limit >= 2u;
    // grid pool: forced on or off, else fused launches and update caps from GPOOL_MIN_CAP (pbn_params.hpp)
    p.gpool = p.handoff && (in.grid_steal > 0 || (in.grid_steal < 0 && (in.cap >= GPOOL_MIN_CAP || in.n_calls > 1u)));
    p.mode = mode;
    p.grp = grp;
    p.erec_shift = erec_shift;
    p.chunk = chunk;
    p.bpc = bpc;
    return p;
}

}  // namespace pbn
