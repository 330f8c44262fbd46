// pbn_env_words.hpp -- the words k_env's waves share, by name: the hand-off box (its layout defined here, once),
// the workgroup's and the grid pool's control words, a pool slot's states, the ring's control words, the
// diagnostics counters and the measurement builds' stamp slots. The protocols that use them: pbn_env.hip.
#pragma once
#include "pbn_device.hpp"
#include "pbn_params.hpp"

namespace pbn {

// grid pool: global-address-space views, so agent-scope atomics lower to global_ (not flat_) sc1 accesses
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;

// ---- the hand-off box: one env as u64 words, the lane's registers and then its state. In LDS it is a wave's
// mailbox (its draw buffer's counter-table bytes); in the grid pool its 2 * box_words u32 halves are a slot's granules.
enum HandoffBox {
    BOX_E = 0,
    BOX_NST = 1,
    BOX_T_USED = 2,  // t | used << 32
    BOX_M_HIT0 = 3,  // m_lo | hit0 << 32
    BOX_N_ACT = 4,
    BOX_O0 = 5  // o0[W], then the state s[W]
};
// a helper request uses the same mailbox: HELP_MARK in word BOX_E, session wave | helper index << 8 in word HELP_REQ
constexpr uint32_t HELP_REQ = 1;
constexpr uint32_t box_words(uint32_t W) { return (uint32_t)BOX_O0 + 2u * W; }  // u64 words
constexpr uint32_t box_nbw(uint32_t W) { return 2u * box_words(W); }  // hand-off words (u32) per env
constexpr uint64_t HELP_MARK = 0xFFFFFFFFFFFFFFFEull;                 // BOX_E of a wave recruited as a helper

// A wave's draw buffer (env_gen_wave_bytes(chunk)) in tail mode: the per-node 64-bit writer masks from
// byte 0 (N <= 512 nodes: 4 KiB), the hand-off flag at chunk * 128 and the hand-off box
// 64 B after it; lane mode's draw table [chunk][64] u16 and counter table use the same bytes
static_assert(8u * 512u <= ENV_CHUNK_SMALL * 128u, "tail writer masks (N <= 512) overlap the hand-off flag");
static_assert(ENV_CHUNK_SMALL * 128u + 64u + 8u * box_words(MAX_WORDS) <= env_gen_wave_bytes(ENV_CHUNK_SMALL),
              "the hand-off box (W <= 8) overflows the wave's draw buffer");
static_assert(box_nbw(MAX_WORDS) <= GPOOL_GRANULES && box_nbw(MAX_WORDS) <= 64u, "grid pool slot: one granule per lane");

// the env of a lane (its registers; its state from the plane column P) into a box
template <int W, class P_t>
__device__ __forceinline__ void box_pack(uint64_t* box, const P_t& P, int64_t e, int64_t nst, uint32_t t, uint32_t used,
                                         uint32_t m_lo, bool hit0, int n_act, const uint64_t (&o0)[W]) {
    uint64_t s[W];
    from_plane<W>(P, s);
    box[BOX_E] = (uint64_t)e;
    box[BOX_NST] = (uint64_t)nst;
    box[BOX_T_USED] = (uint64_t)t | (uint64_t)used << 32;
    box[BOX_M_HIT0] = (uint64_t)m_lo | (hit0 ? 1ull << 32 : 0ull);
    box[BOX_N_ACT] = (uint64_t)(int64_t)n_act;
#pragma unroll
    for (int k2 = 0; k2 < W; ++k2) {
        box[BOX_O0 + k2] = o0[k2];
        box[BOX_O0 + W + k2] = s[k2];
    }
}

// a box's env into a lane's registers and its plane column
template <int W, class P_t>
__device__ __forceinline__ void box_unpack(const uint64_t* box, const P_t& P, int64_t& e, int64_t& nst, uint32_t& t,
                                           uint32_t& used, uint32_t& m_lo, bool& hit0, int& n_act, uint64_t (&o0)[W]) {
    e = (int64_t)box[BOX_E];
    nst = (int64_t)box[BOX_NST];
    const uint64_t tu = box[BOX_T_USED], mh = box[BOX_M_HIT0];
    t = (uint32_t)tu;
    used = (uint32_t)(tu >> 32);
    m_lo = (uint32_t)mh;
    hit0 = ((mh >> 32) & 1ull) != 0ull;
    n_act = (int)(int64_t)box[BOX_N_ACT];
    uint64_t s[W];
#pragma unroll
    for (int k2 = 0; k2 < W; ++k2) {
        o0[k2] = box[BOX_O0 + k2];
        s[k2] = box[BOX_O0 + W + k2];
    }
    to_plane<W>(P, s);
}

// ---- workgroup control words (LDS, after the waves' draw buffers)
enum WgCtl {
    WCTL_BUSY = 0,     // busy waves
    WCTL_IDLE = 1,     // idle mask
    WCTL_WAITING = 2,  // grid pool: a wave of this workgroup is waiting on a ticket
    WCTL_POOL = 3      // grid pool: WG_DONE | WG_LEFT_CU
};
constexpr uint32_t WG_DONE = 1u;     // the launch's work is done, leave
constexpr uint32_t WG_LEFT_CU = 2u;  // this workgroup left its CU's count

// ---- grid pool control words (EnvArgs::gpool_ctl: device memory, every access a global agent-scope atomic,
// sc1: past the CU's L1)
enum PoolCtl {
    GCTL_RESERVED = 0,  // slots reserved by pushers
    GCTL_TICKETS = 1,   // tickets taken by idle workgroups
    GCTL_LIVE = 2,      // workgroups working + envs in the pool
    GCTL_PUSHED = 3,    // envs pushed
    GCTL_TIMEOUTS = 4,  // waits given up on a claimed slot (error flag 2)
    GCTL_MIGRATED = 5   // of the pushed, sessions moved mid-way (tools/patches/r05_session_migration.patch)
};
// a slot's state word (EnvArgs::gpool_state): epoch << 2 | one of these; any other epoch: unclaimed
constexpr uint32_t SLOT_CLAIMED = 1u;   // a pusher claimed it: its granules are on their way
constexpr uint32_t SLOT_GIVEN_UP = 2u;  // its ticket holder gave up on it
// (raised by an atomic max, epochs only grow: whichever of the two lands first tells the other)

// ---- diagnostics (EnvArgs::steal_count)
enum StealCount {
    STEAL_ENVS = 0,         // envs handed off inside workgroups (pbn_env_handoffs)
    STEAL_HELPERS = 1,      // helpers recruited (pbn_env_tail_helpers)
    STEAL_RING_BLOCKS = 2,  // ring blocks resolved (pbn_env_tail_stats)
    STEAL_RING_WAITS = 3    // of them, blocks the session wave had to wait for
};

// ---- the ring's control words, after its ring_R slots in the session wave's draw buffer
enum RingCtl {
    RING_TAGS = 0,     // [0, 8): the block index held by each slot
    RING_CONS = 8,     // ring blocks below it are consumed
    RING_STOP = 9,
    RING_ACKS = 10,    // helpers' acks
    RING_U0 = 12,      // the ring's first update (even: a block boundary)
    RING_C1 = 13,      // the session's Philox call index
    RING_GID_LO = 14,  // the env's global id
    RING_GID_HI = 15,
    RING_HELPERS = 17  // the session's helpers
};

// ---- measurement builds (tools/build_exp.sh -DPBN_STAMPS): per-wave stamps. tools/env_stamps.py and
// tools/tail_stamps.py read them by index, so the numbers stay.
enum EnvStampSlot {
    EST_START = 0,          // after the staging barrier (s_memrealtime, 100 MHz, as the other times)
    EST_BELOW_OWN = 1,      // first chunk below ENV_OWN_DRAWS_MIN active lanes
    EST_QUEUE_EMPTY = 2,    // first chunk after a lane of the wave found the work queue empty
    EST_LE32 = 3,           // first chunk with <= 32 / 16 / 8 / 2 active lanes
    EST_LE16 = 4,
    EST_LE8 = 5,
    EST_LE2 = 6,
    EST_END = 7,
    EST_CHUNKS = 8,
    EST_ACTIVE_SUM = 9,     // sum of active lanes over chunks
    EST_TAIL_CHUNKS = 10,   // chunks in the tail (queue empty)
    EST_TAIL_ACTIVE = 11,   // sum of active lanes there
    EST_BLOCK = 12,
    EST_HW_ID = 13,
    EST_CAPPED = 14,        // env steps of the wave that hit the update cap
    EST_POPS = 15,          // hand-offs received
    EST_PUSHED = 16,        // envs handed off (low half), envs received from the grid pool (high half)
    EST_POP_TICKS = 17,     // ticks waiting in local_pop
    EST_FIRST_POP = 18,     // time of the first local_pop
    // tail block phases (shader clocks, s_memtime)
    EST_TB_BLOCKS = 19,
    EST_TB_CYCLES = 20,     // cycles in blocks
    EST_TB_ROUNDS = 21,     // fixed-point rounds
    EST_TB_FP = 22,         // cycles of the resolution (fixed point)
    EST_TB_PREP = 23,       // cycles from the block's top to the later blocks' stages issued
    EST_TB_BY_ROUNDS = 24,  // 24..31: blocks by rounds (0..6, 7+)
    EST_TB_TICKS = 32,      // realtime ticks (10 ns) in tail blocks
    EST_ENTRY = 33,         // kernel entry (before the image is staged)
    EST_TB_FIRST = 34,      // time of the first tail block's top
    EST_TB_LAST = 35,       // time of the last tail block's end
    EST_SESS_START = 36,    // the wave's longest session: start, blocks, end, prior updates
    EST_SESS_BLOCKS = 37,
    EST_SESS_END = 38,
    EST_SESS_U0 = 39,
    ENV_STAMPS = 40
};

#ifdef PBN_STAMPS
// a tail block's clocks (s_memtime c_*, s_memrealtime r_top) and its fixed-point rounds
struct BlockClocks {
    uint64_t c_top, r_top, c_prep, c_fp;
    uint32_t nround;
};
__device__ __forceinline__ BlockClocks stamp_block_top(uint64_t (&est)[ENV_STAMPS]) {
    BlockClocks bc;
    bc.c_top = __builtin_amdgcn_s_memtime();
    bc.r_top = __builtin_amdgcn_s_memrealtime();  // 100 MHz: calibrates s_memtime
    if (!est[EST_TB_FIRST]) est[EST_TB_FIRST] = bc.r_top;
    bc.c_prep = bc.c_fp = 0;
    bc.nround = 0;
    return bc;
}
// the block epilogue of the self-prepared loop and of ring128 (there, rounds count fround calls)
__device__ __forceinline__ void stamp_block_end(uint64_t (&est)[ENV_STAMPS], const BlockClocks& bc) {
    const uint64_t c_end = __builtin_amdgcn_s_memtime();
    const uint64_t r_end = __builtin_amdgcn_s_memrealtime();
    est[EST_TB_TICKS] += r_end - bc.r_top;
    est[EST_TB_LAST] = r_end;
    est[EST_TB_BLOCKS] += 1;
    est[EST_TB_CYCLES] += c_end - bc.c_top;
    est[EST_TB_ROUNDS] += bc.nround;
    est[EST_TB_FP] += bc.c_fp - bc.c_prep;
    est[EST_TB_PREP] += bc.c_prep - bc.c_top;
    est[EST_TB_BY_ROUNDS + min(bc.nround, 7u)] += 1;
}
#endif

}  // namespace pbn
