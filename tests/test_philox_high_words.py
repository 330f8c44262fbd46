"""The high words of every Philox draw: 64-bit seeds, global env ids past 2^32 and counters past 2^32.

Every kernel family draws from Philox4x32-10 with key ``{seed_lo, seed_hi}`` and counter ``{c0, c1, gid_lo,
(gid_hi & 0xFFFFFF) | stream << 24}`` (csrc/pbn_device.hpp); c0 (and for some streams c1) hold a 64-bit update,
iteration or step counter. The rest of the suite keeps all of those high words at zero. Here:

* CPU (unmarked): the oracle's own draws are rebuilt word for word from the documented layout
  (csrc/pbn_params.hpp's stream comments) with nothing but ``oracle.philox4x32_10`` (pinned by the Random123
  known-answer test) and numpy, at the edge settings below -- so the GPU half compares against a pinned oracle.
* GPU: every drawing path, with the batch moved to the edge by ``PBNBatch.seek``, bit for bit against the oracle.

Every edge case also asserts that it can fail: the oracle's result with the high word zeroed (``seed &
0xFFFFFFFF``; env ids modulo 2^32, modulo 2^33 for the step stream, which draws per id pair; counter modulo 2^32)
differs from the true result.
"""

import numpy as np
import pytest

from conftest import cubes_to_attractors, golden, r6_config
from gym_pbn_amd.network import load_network
from r6_cases import (ENV_VARIANT_CASES, FORCED_TAIL_CASES, env_variant_setup, forced_tail_knobs,
                      long_first_step_actions, random_cubes)

M32 = 1 << 32
STREAM_STEP, STREAM_INIT, STREAM_ENV, STREAM_RESET, STREAM_SYNC = 1, 2, 3, 4, 7

# ----------------------------------------------------------------- the edge settings, one table
SEED_A = 0x9E3779B97F4A7C15  # both halves non-zero and different
SEED_B = 0xDEADBEEF00000000  # low half zero
SEED_PLAIN, BASE_PLAIN = 4242, 77
WRAP_EVEN, WRAP_ODD = 150, 101  # base = 2^w - k: the id wrap falls on env k of the batch, off any 64- / 256-lane
#                                 boundary; k even: an even base (paired step draws), k odd: an odd one
CTR_FAR = (1 << 40) + 12345     # a start well above the wrap
# (seed, k or None, counters: "a" wrap r with an odd start / "b" wrap r with an even start / "far" / None)
EDGES = {
    "all_a": (SEED_A, WRAP_EVEN, "a"),       # every edge on: 64-bit seed, straddling base, straddling counter
    "all_b": (SEED_B, WRAP_ODD, "b"),
    "all_top": (SEED_A, "top", "far"),       # base 2^56 - B: every bit of the 24-bit id field set
    "seed_only": (SEED_A, None, None),       # one edge alone, so a failure names the word
    "seed_b_only": (SEED_B, None, None),
    "base_only": (SEED_PLAIN, WRAP_EVEN, None),
    "base_odd_only": (SEED_PLAIN, WRAP_ODD, None),
    "ctr_only": (SEED_PLAIN, None, "a"),
    "ctr_far_only": (SEED_PLAIN, None, "far"),
}
ALONE = ["seed_only", "seed_b_only", "base_only", "base_odd_only", "ctr_only", "ctr_far_only"]
# the counter's distance below 2^32 per family, (odd start, even start): the wrap falls inside one call and launch
WRAP_R = {"step": (37, 38), "ssd": (40, 41), "sync": (3, 4)}


def edge(name, B, family, k=None):
    """(seed, env_id_base, counter) of setting ``name`` for a batch of B envs. family "step": ids are halved,
    the base straddles 2^33; otherwise 2^32. ``k`` overrides the table's wrap position (same parity)."""
    seed, kk, c = EDGES[name]
    w = 33 if family == "step" else 32
    if kk is None:
        base = BASE_PLAIN
    elif kk == "top":
        base = (1 << 56) - B
    else:
        kk = k if k is not None else kk
        assert 0 < kk < B
        base = (1 << w) - kk
    r = WRAP_R.get(family, (0, 0))
    ctr = {None: 0, "a": M32 - r[0], "b": M32 - r[1], "far": CTR_FAR}[c]
    return seed, base, ctr


# ----------------------------------------------------------------- the oracle with one high word zeroed
def _segments(start, n, mod, split):
    """[(offset, count, start')]: runs of start + i, i < n, in which (start + i) // mod is constant, each from
    (start + i) % mod -- what a draw sees whose word above ``mod`` is forced to zero. split False: one run."""
    if not split:
        return [(0, n, start)]
    out, i = [], 0
    while i < n:
        v = start + i
        c = min(n - i, mod - v % mod)
        out.append((i, c, v % mod))
        i += c
    return out


def orc_run(fn, st, seed, base, ctr, T, zero="", id_mod=M32):
    """fn(env slice, state rows, seed, base, ctr, n, t0) -> (state rows, extra or None) over the batch. ``zero``
    names the high words to force to zero ("seed", "base", "ctr"): the run is then cut where a high word would
    change and every piece restarts from the low word. Extras (histograms) are summed."""
    sd = seed & 0xFFFFFFFF if "seed" in zero else seed
    out, extra = np.empty_like(st), None
    for e0, n_e, b in _segments(base, len(st), id_mod, "base" in zero):
        s = st[e0:e0 + n_e]
        for t0, n_t, c in _segments(ctr, T, M32, "ctr" in zero):
            s, x = fn(slice(e0, e0 + n_e), s, sd, b, c, n_t, t0)
            if x is not None:
                extra = x if extra is None else extra + x
        out[e0:e0 + n_e] = s
    return out, extra


def on_edges(seed, base, B, ctr, T, id_mod=M32, ctr64=True):
    """The high words that are non-zero somewhere in this run."""
    z = []
    if seed >> 32:
        z.append("seed")
    if base + B - 1 >= id_mod:
        z.append("base")
    if ctr64 and ctr + max(T, 1) - 1 >= M32:
        z.append("ctr")
    return z


def orc_checked(fn, st, seed, base, ctr, T, id_mod=M32, ctr64=True):
    """The oracle's true result, after asserting that zeroing any one live high word changes it (a shape at which
    it did not would test nothing)."""
    true = orc_run(fn, st, seed, base, ctr, T)
    zs = on_edges(seed, base, len(st), ctr, T, id_mod, ctr64)
    assert zs, "not an edge setting"
    for z in zs:
        alt = orc_run(fn, st, seed, base, ctr, T, zero=z, id_mod=id_mod)
        same = np.array_equal(true[0], alt[0]) and (true[1] is None or np.array_equal(true[1], alt[1]))
        assert not same, f"vacuous: zeroing the high word of {z} changes nothing"
    return true


def step_fn(o):
    return lambda sl, s, sd, b, c, n, t0: (o.step_philox(s, sd, b, c, n), None)


# ----------------------------------------------------------------- CPU: the oracle's draws from the layout
def draw(oracle_mod, seed, c0, c1, gid, stream):
    """One Philox call by the documented layout, nothing of the oracle's but the bare generator."""
    return oracle_mod.philox4x32_10([c0 & 0xFFFFFFFF, c1 & 0xFFFFFFFF, gid & 0xFFFFFFFF,
                                     ((gid >> 32) & 0xFFFFFF) | (stream << 24)], [seed & 0xFFFFFFFF, seed >> 32])


def u32_k53(a):
    return (a << 21) | (a >> 11)


def k53_pair(hi, lo):
    return ((hi >> 5) << 26) | (lo >> 6)


def node_of(net, w):
    return (w * net.n_nodes) >> 32 if net.kind == 1 else 1 + ((w * (net.n_nodes - 1)) >> 32)


def test_segments_cut_at_the_wrap():
    assert _segments(M32 - 3, 8, M32, True) == [(0, 3, M32 - 3), (3, 5, 0)]
    assert _segments((1 << 33) - 2, 4, 1 << 33, True) == [(0, 2, (1 << 33) - 2), (2, 2, 0)]
    assert _segments(CTR_FAR, 5, M32, True) == [(0, 5, CTR_FAR % M32)]
    assert _segments(M32 - 3, 8, M32, False) == [(0, 8, M32 - 3)]


@pytest.mark.parametrize("setting", ["all_a", "all_b", "all_top", "ctr_far_only"])
@pytest.mark.parametrize("name", ["bittner28", "tt8"])
def test_step_stream_rebuilt_from_the_layout(oracle_mod, name, setting):
    """STREAM_STEP: update u of env g takes call {u_lo, u_hi, (g >> 1)_lo, (g >> 1)_hi | STEP << 24}, the node
    from word 2(g & 1) by philox_node's rule and k53 from word 2(g & 1) + 1 by u32_k53. Replayed through
    step_replay, the draws give step_philox's states."""
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B, T = 192, 48
    seed, base, ctr = edge(setting, B, "step")
    st = o.init_philox(B, seed=3)
    ni = np.empty((T, B), np.uint32)
    kk = np.empty((T, B), np.uint64)
    for e in range(B):
        g = base + e
        for t in range(T):
            u = ctr + t
            w = draw(oracle_mod, seed, u, u >> 32, g >> 1, STREAM_STEP)
            ni[t, e] = node_of(net, w[2 * (g & 1)])
            kk[t, e] = u32_k53(w[2 * (g & 1) + 1])
    want, _ = orc_checked(step_fn(o), st, seed, base, ctr, T, id_mod=1 << 33)
    assert np.array_equal(o.step_replay(st, ni, kk), want)
    assert np.array_equal(o.step_forced(st, ni, seed, base, ctr), want)  # the forced path: same choice words


@pytest.mark.parametrize("setting", ["all_a", "all_b", "all_top"])
@pytest.mark.parametrize("name", ["bittner199", "tt8"])
def test_init_and_reset_streams_rebuilt_from_the_layout(oracle_mod, name, setting):
    """STREAM_INIT: call {m, reset_count, g} gives state words 2m (w1 << 32 | w0) and 2m + 1 (w3 << 32 | w2).
    STREAM_RESET: call {0, reset_count, g} picks cube umulhi(w0, n_cubes), calls {m + 1, ...} the free bits.
    reset_count is a uint32 (0xFFFFFFFF here)."""
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B, W, N, rc = 160, net.n_words, net.n_nodes, 0xFFFFFFFF
    seed, base, _ = edge(setting, B, "direct")
    from gym_pbn_amd.batch import cube_arrays

    care, value = cube_arrays(random_cubes(np.random.default_rng(5), N, 3, max(2, N // 4)), N)
    top = (1 << (N & 63)) - 1 if N & 63 else (1 << 64) - 1
    init = np.zeros((B, W), np.uint64)
    reset = np.zeros((B, W), np.uint64)
    for e in range(B):
        g = base + e
        ws, wr = [], []
        for m in range((W + 1) // 2):
            a = draw(oracle_mod, seed, m, rc, g, STREAM_INIT)
            r = draw(oracle_mod, seed, m + 1, rc, g, STREAM_RESET)
            ws += [a[1] << 32 | a[0], a[3] << 32 | a[2]]
            wr += [r[1] << 32 | r[0], r[3] << 32 | r[2]]
        c = (draw(oracle_mod, seed, 0, rc, g, STREAM_RESET)[0] * 3) >> 32
        for k in range(W):
            cm = int(care[c, k])
            x, y = ws[k], (int(value[c, k]) & cm) | (wr[k] & ~cm)
            if k == W - 1:
                x, y = x & top, y & top
            if k == 0 and net.kind == 2:
                x, y = x & ~1, y & ~1
            init[e, k], reset[e, k] = x, y
    init_fn = lambda sl, s, sd, b, c, n, t0: (o.init_philox(len(s), sd, b, rc), None)
    reset_fn = lambda sl, s, sd, b, c, n, t0: (o.env_reset_philox(s, np.ones(len(s), np.int64), care, value, seed=sd,
                                                                   env_base=b, reset_count=rc)[0], None)
    z = np.zeros((B, W), np.uint64)
    assert np.array_equal(orc_checked(init_fn, z, seed, base, 0, 1, ctr64=False)[0], init)
    assert np.array_equal(orc_checked(reset_fn, z, seed, base, 0, 1, ctr64=False)[0], reset)


@pytest.mark.parametrize("step", [M32 + 5, M32 - 1, CTR_FAR, (1 << 48) - 1])
@pytest.mark.parametrize("name", ["bittner28", "tt8"])
def test_sync_stream_rebuilt_at_high_step_counters(oracle_mod, name, step):
    """STREAM_SYNC: node i of step s draws call {s_lo, (i >> 1) | s_hi << 16, g}, words (0, 1) for even i and
    (2, 3) for odd i, and reads the pre-step snapshot -- test_sync_uses_snapshot_not_running_state's per-node
    check, for every node, at step counters whose high half is live (room for s_hi < 2^16)."""
    from gym_pbn_amd.batch import unpack_bits

    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B = 12
    seed, base, _ = edge("all_a", B, "direct", k=6)
    x = o.init_philox(B, seed=9)
    sync_fn = lambda sl, s, sd, b, c, n, t0: (oracle_mod.sync_philox(o, s, sd, b, c, n), None)
    got = unpack_bits(orc_checked(sync_fn, x, seed, base, step, 1)[0], net.n_nodes)
    for e in range(B):
        for i in range(net.n_nodes):
            w = draw(oracle_mod, seed, step, (i >> 1) | ((step >> 32) << 16), base + e, STREAM_SYNC)
            k53 = k53_pair(w[0], w[1]) if i % 2 == 0 else k53_pair(w[2], w[3])
            one = o.step_replay(x[e:e + 1], np.array([[i]], np.uint32), np.array([[k53]], np.uint64))
            assert unpack_bits(one, net.n_nodes)[0, i] == got[e, i], (e, i)


@pytest.mark.parametrize("call_idx", [0xFFFFFFFE, 0xFFFFFFFF, 0])
@pytest.mark.parametrize("setting", ["all_a", "all_b", "all_top"])
def test_env_stream_rebuilt_from_the_layout(oracle_mod, setting, call_idx):
    """STREAM_ENV: update j of an env step takes call {j >> 1, call index, g}, node from word 2(j & 1), k53 from
    word 2(j & 1) + 1 (u32_k53). One env step's draws, rebuilt and fed to env_step_multi(replay=...), give the
    Philox mode's outputs. The call index is a uint32."""
    z = golden("r6_bittner28.npz")
    net = load_network("bittner28")
    o = oracle_mod.Oracle(net)
    cfgd = r6_config(z)
    B, cap = 192, 96
    seed, base, _ = edge(setting, B, "direct")
    st = o.init_philox(B, seed=11)
    ns = np.zeros(B, np.int64)
    acts = np.random.default_rng(2).integers(0, 29, size=(B, 2)).astype(np.int32)
    ref = o.env_step_multi(cfgd, st, ns, acts, seed=seed, env_base=base, call_idx=call_idx, update_cap=cap)
    off = np.concatenate([[0], np.cumsum(ref["n_updates"])]).astype(np.int64)
    di = np.empty(off[-1], np.uint32)
    dk = np.empty(off[-1], np.uint64)
    for e in range(B):
        for j in range(int(ref["n_updates"][e])):
            w = draw(oracle_mod, seed, j >> 1, call_idx, base + e, STREAM_ENV)
            di[off[e] + j] = node_of(net, w[2 * (j & 1)])
            dk[off[e] + j] = u32_k53(w[2 * (j & 1) + 1])
    rep = o.env_step_multi(cfgd, st, ns, acts, replay=(off, di, dk))
    capped = ref["flags"] & 4
    assert capped.any() and not capped.all()
    for k in ("state", "obs", "reward", "n_updates", "n_steps"):
        assert np.array_equal(rep[k], ref[k]), k
    assert np.array_equal(rep["flags"], ref["flags"])  # replay: out of draws == capped
    for zero in ("seed", "base"):
        alt = r6_oracle(o, cfgd, st, ns, acts, seed, base, call_idx, cap, zero=zero)
        assert not np.array_equal(alt["state"], ref["state"]), zero
    if call_idx:
        alt = o.env_step_multi(cfgd, st, ns, acts, seed=seed, env_base=base, call_idx=0, update_cap=cap)
        assert not np.array_equal(alt["state"], ref["state"])


def r6_oracle(o, cfgd, st, ns, acts, seed, base, call_idx, cap, zero=""):
    """oracle.env_step_multi over the batch, optionally with one high word zeroed (see orc_run)."""
    sd = seed & 0xFFFFFFFF if "seed" in zero else seed
    parts = []
    for e0, n, b in _segments(base, len(st), M32, "base" in zero):
        sl = slice(e0, e0 + n)
        parts.append(o.env_step_multi(cfgd, st[sl], ns[sl], acts[sl], seed=sd, env_base=b, call_idx=call_idx,
                                      update_cap=cap, n_threads=16))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.parametrize("seed", [SEED_A, SEED_B])
@pytest.mark.parametrize("base", [M32 - WRAP_ODD, M32 - WRAP_EVEN, (1 << 56) - 160])
def test_env_actions_high_words(oracle_mod, seed, base):
    """actions.env_actions with a 64-bit seed and env ids past 2^32 against the layout of its docstring:
    call {t, c1, g, STREAM_ACTIONS}, c1 = 0 the node words, c1 = 1 the keep words."""
    from gym_pbn_amd.actions import STREAM_ACTIONS, env_actions

    T, B, A, N = 3, 160, 4, 199
    got = env_actions(T, base, B, A, N, seed=seed).numpy()
    want = np.empty((T, B, A), np.int32)
    for t in range(T):
        for e in range(B):
            w0 = draw(oracle_mod, seed, t, 0, base + e, STREAM_ACTIONS)
            w1 = draw(oracle_mod, seed, t, 1, base + e, STREAM_ACTIONS)
            want[t, e] = [(1 + ((w0[a] * N) >> 32)) if w1[a] >= 3 << 30 else 0 for a in range(A)]
    assert np.array_equal(got, want)
    assert not np.array_equal(got, env_actions(T, base, B, A, N, seed=seed & 0xFFFFFFFF).numpy())
    low = [env_actions(T, b, n, A, N, seed=seed).numpy() for _, n, b in _segments(base, B, M32, True)]
    assert not np.array_equal(got, np.concatenate(low, axis=1))


# ================================================================= GPU
@pytest.fixture(scope="module")
def G():
    from gym_pbn_amd import _lib, batch

    assert _lib.device_count() >= 1, "gpu tests need a HIP device"
    return batch


gpu = pytest.mark.gpu


@gpu
def test_counters_and_seek(G):
    """counters() / seek(): only the named fields move, 32-bit counters wrap modulo 2^32, info() agrees, NULL
    arguments are refused."""
    import ctypes as C

    from gym_pbn_amd import _lib

    b = G.PBNBatch("bittner28", 64, seed=1)
    zero = dict(update_count=0, ssd_iters=0, sync_steps=0, env_call_count=0, reset_count=0)
    assert b.counters() == zero
    b.seek(update_count=CTR_FAR, reset_count=0xFFFFFFFF)
    assert b.counters() == dict(zero, update_count=CTR_FAR, reset_count=0xFFFFFFFF)
    b.seek(ssd_iters=M32 - 40, sync_steps=(1 << 64) - 1, env_call_count=M32 + 7)
    assert b.counters() == dict(update_count=CTR_FAR, ssd_iters=M32 - 40, sync_steps=(1 << 64) - 1,
                                env_call_count=7, reset_count=0xFFFFFFFF)
    b.randomize()
    b.step(3)
    i = b.info()
    assert i["reset_count"] == 0 and i["update_count"] == CTR_FAR + 3 and i["env_call_count"] == 7
    assert b.counters()["reset_count"] == 0 and b.counters()["update_count"] == CTR_FAR + 3
    with pytest.raises(TypeError):
        b.seek(updates=1)
    with pytest.raises(ValueError):
        b.seek(update_count=-1)
    assert _lib.lib.pbn_batch_get_counters(b.handle, None) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "out is NULL"
    assert _lib.lib.pbn_batch_set_counters(b.handle, None) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "in is NULL"
    c = _lib.BatchCounters()
    assert _lib.lib.pbn_batch_get_counters(None, C.byref(c)) == _lib.PBN_E_INVALID
    b.close()


# ----------------------------------------------------------------- init and reset
@gpu
@pytest.mark.parametrize("setting", ["all_a", "all_b", "all_top", "seed_only", "seed_b_only", "base_only",
                                     "base_odd_only"])
@pytest.mark.parametrize("name", ["bittner199", "bittner28", "tt8", "tt200"])
def test_init_and_reset_at_the_edges(G, oracle_mod, name, setting):
    """randomize (STREAM_INIT), then env_reset with cubes and a mask twice (STREAM_RESET), from reset_count
    0xFFFFFFFF: the count wraps to 0 and 1 on both sides."""
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    N, B = net.n_nodes, 700
    seed, base, _ = edge(setting, B, "direct")
    gnet = G.Net(net)
    att = [random_cubes(np.random.default_rng(5), N, 3, max(2, N // 4))]
    cfg = G.EnvConfig(gnet, att, horizon=5)
    b = G.PBNBatch(gnet, B, seed=seed, env_id_base=base)
    b.seek(reset_count=0xFFFFFFFF)
    b.randomize()
    fn = lambda rc: (lambda sl, s, sd, bb, c, n, t0: (o.init_philox(len(s), sd, bb, rc), None))
    st, _ = orc_checked(fn(0xFFFFFFFF), np.zeros((B, net.n_words), np.uint64), seed, base, 0, 1, ctr64=False)
    assert np.array_equal(b.get_state(), st)
    assert b.counters()["reset_count"] == 0
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    for rc, m in ((0, None), (1, mask)):
        rfn = lambda sl, s, sd, bb, c, n, t0: (o.env_reset_philox(
            s, np.ones(len(s), np.int64), cfg.reset_care, cfg.reset_value, mask=None if m is None else m[sl],
            seed=sd, env_base=bb, reset_count=rc)[0], None)
        b.env_reset(cfg, m)
        st, _ = orc_checked(rfn, st, seed, base, 0, 1, ctr64=False)
        assert np.array_equal(b.get_state(), st), rc
    assert b.counters()["reset_count"] == 2 and not b.get_n_steps()[mask != 0].any()
    b.close()


# ----------------------------------------------------------------- step mode
# path -> (knob, value, network, B, wrap position k or None for the table's)
STEP_PATHS = {
    "plain": ("PBNSIM_STEP_GRAPH", "0", "bittner199", 700, None),
    "plain_tt": ("PBNSIM_STEP_GRAPH", "0", "tt200", 700, None),
    "plain_w1": ("PBNSIM_STEP_GRAPH", "0", "bittner28", 700, None),
    "graph": ("PBNSIM_STEP_GRAPH", "1", "bittner199", 700, None),
    "graph_tt": ("PBNSIM_STEP_GRAPH", "1", "tt8", 700, None),
    "block256": ("PBNSIM_STEP_BLOCK", "256", "bittner199", 1500, None),
    "block1024": ("PBNSIM_STEP_BLOCK", "1024", "bittner199", 2500, None),
    "ept1": ("PBNSIM_ENVS_PER_THREAD", "1", "bittner28", 700, None),
    "ept4": ("PBNSIM_ENVS_PER_THREAD", "4", "bittner199", 3001, None),
    # the id wrap inside chain 1 of 2 (envs 1024 ..) / chain 2 of 4 (envs 1024 .. 1535): each chain's env_base
    # is the batch's plus its offset, and the chain that holds the wrap is not the first
    "chains2": ("PBNSIM_STEP_CHAINS", "2", "bittner199", 2048, 1500),
    "chains4": ("PBNSIM_STEP_CHAINS", "4", "bittner28", 2048, 1350),
}
STEP_RUNS = ([(p, s) for p in STEP_PATHS for s in ("all_a", "all_b")]
             + [(p, "all_top") for p in ("plain", "graph", "chains2")] + [("plain", s) for s in ALONE]
             + [("graph", s) for s in ("ctr_only", "ctr_far_only")])


@gpu
@pytest.mark.parametrize("path,setting", STEP_RUNS)
def test_step_paths_at_the_edges(G, oracle_mod, monkeypatch, path, setting):
    """pbn_step's draw paths (k_step_single paired / unpaired, plain launches and graph replays reading the
    device counter, block sizes, envs per thread, launch chains) from a counter 37 or 38 below 2^32: one update,
    a call of 70 that straddles the wrap (inside the 64-launch graph where graphs replay), and a second call after
    it, which starts from the carried counter."""
    knob, val, name, B, k = STEP_PATHS[path]
    monkeypatch.setenv(knob, val)
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    if k is not None and EDGES[setting][1] in (WRAP_EVEN, WRAP_ODD):
        k += (k + EDGES[setting][1]) & 1  # keep the table's base parity
    seed, base, ctr = edge(setting, B, "step", k)
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    if knob == "PBNSIM_STEP_CHAINS":
        assert b.info()["step_chains"] == int(val)
    b.randomize()
    s0 = b.get_state()
    b.seek(update_count=ctr)
    b.step(1)
    assert np.array_equal(b.get_state(), o.step_philox(s0, seed, base, ctr, 1))
    b.step(70)
    want, _ = orc_checked(step_fn(o), s0, seed, base, ctr, 71, id_mod=1 << 33)
    assert np.array_equal(b.get_state(), want)
    b.step(5)
    b.step(5)  # the same length twice: an exact-length graph where graphs replay
    assert np.array_equal(b.get_state(), o.step_philox(want, seed, base, ctr + 71, 10))
    assert b.counters()["update_count"] == ctr + 81
    b.close()


@gpu
@pytest.mark.parametrize("setting", ["all_a", "all_b", "ctr_only"])
def test_exact_length_graphs_at_the_edges(G, oracle_mod, monkeypatch, setting):
    """Graphs captured before a seek -- prepare_steps(50)'s exact-length graph and the power-of-two graphs of a
    call of 70 -- replay from the counter the seek left (nothing captured holds a host counter): two replays of
    50, the first straddling the wrap, then a call of 70 from a second seek to below the wrap."""
    monkeypatch.setenv("PBNSIM_STEP_GRAPH", "1")
    net = load_network("bittner199")
    o = oracle_mod.Oracle(net)
    B = 900
    seed, base, ctr = edge(setting, B, "step")
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    b.randomize()
    s0 = b.get_state()
    b.prepare_steps(50)
    b.step(50)  # from 0
    b.step(70)  # ... and the power-of-two graphs (64 + 4 + 2), captured at this call
    assert np.array_equal(b.get_state(), o.step_philox(s0, seed, base, 0, 120))
    b.set_state(s0)
    b.seek(update_count=ctr)
    b.step(50)
    want, _ = orc_checked(step_fn(o), s0, seed, base, ctr, 50, id_mod=1 << 33)
    assert np.array_equal(b.get_state(), want)
    b.step(50)
    want = o.step_philox(want, seed, base, ctr + 50, 50)
    assert np.array_equal(b.get_state(), want)
    b.seek(update_count=ctr - 30)  # back below the wrap: the 64-launch graph replays across it
    b.step(70)
    assert np.array_equal(b.get_state(), o.step_philox(want, seed, base, ctr - 30, 70))
    assert b.counters()["update_count"] == ctr + 40
    b.close()


@gpu
@pytest.mark.parametrize("setting", ["all_a", "all_b", "all_top", "ctr_far_only"])
@pytest.mark.parametrize("name", ["bittner199", "tt200"])
def test_step_forced_at_the_edges(G, oracle_mod, name, setting):
    """pbn_step_forced: the caller's nodes, the choice words of updates ctr .. ctr + T - 1 in one launch."""
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B, T = 700, 60
    seed, base, ctr = edge(setting, B, "step")
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    b.randomize()
    s0 = b.get_state()
    ni = np.random.default_rng(B).integers(1 if net.kind == 2 else 0, net.n_nodes, size=(T, B)).astype(np.uint32)
    b.seek(update_count=ctr)
    b.step_forced(ni)
    fn = lambda sl, s, sd, bb, c, n, t0: (o.step_forced(s, ni[t0:t0 + n, sl], sd, bb, c), None)
    want, _ = orc_checked(fn, s0, seed, base, ctr, T, id_mod=1 << 33)
    assert np.array_equal(b.get_state(), want)
    b.step(3)  # the counter carried on
    assert np.array_equal(b.get_state(), o.step_philox(want, seed, base, ctr + T, 3))
    b.close()


# ----------------------------------------------------------------- rollout
@gpu
@pytest.mark.parametrize("setting", ["all_a", "all_b"])
@pytest.mark.parametrize("group,name", [(None, "bittner28"), (None, "tt200"), ("1", "bittner28"), ("1", "bittner199"),
                                        ("1", "tt8"), ("2", "bittner28"), ("4", "bittner199"), ("8", "bittner28"),
                                        ("2", "bittner199"), ("4", "bittner28"), ("8", "bittner199")])
def test_rollout_at_the_edges(G, oracle_mod, monkeypatch, group, name, setting):
    """rollout(128) from 37 (38) below 2^32: k_rollout's words2 -- with an even base the lane pair splits updates
    u, u + 1, and from an odd start the even lane holds u = 0xFFFFFFFF while its partner's u + 1 carries into
    the high word -- and k_rollout_grp's step_words(update_base + used + k); a second call after the wrap. Group
    unset: the library's choice for the batch (8 lanes per env here for predictor-mix networks, lane mode for
    truth tables); "1": k_rollout."""
    if group is None:
        monkeypatch.delenv("PBNSIM_ROLL_GROUP", raising=False)
    else:
        monkeypatch.setenv("PBNSIM_ROLL_GROUP", group)
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B = 1000
    seed, base, ctr = edge(setting, B, "step")
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    if group is not None:
        assert b.info()["roll_lanes"] == (1 if net.kind == 2 else int(group))
    b.randomize()
    s0 = b.get_state()
    b.seek(update_count=ctr)
    b.rollout(128)
    want, _ = orc_checked(step_fn(o), s0, seed, base, ctr, 128, id_mod=1 << 33)
    assert np.array_equal(b.get_state(), want)
    b.rollout(7)
    assert np.array_equal(b.get_state(), o.step_philox(want, seed, base, ctr + 128, 7))
    b.close()


@gpu
@pytest.mark.parametrize("setting", ["all_top"] + ALONE)
def test_rollout_single_edges(G, oracle_mod, monkeypatch, setting):
    """k_rollout (one lane per env) with each edge alone, and at the top of the id field."""
    monkeypatch.setenv("PBNSIM_ROLL_GROUP", "1")
    net = load_network("bittner199")
    o = oracle_mod.Oracle(net)
    B = 1000
    seed, base, ctr = edge(setting, B, "step")
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    b.randomize()
    s0 = b.get_state()
    b.seek(update_count=ctr)
    b.rollout(128)
    want, _ = orc_checked(step_fn(o), s0, seed, base, ctr, 128, id_mod=1 << 33)
    assert np.array_equal(b.get_state(), want)
    b.close()


# ----------------------------------------------------------------- R6 env step
R6_T = 4  # env steps per run: Philox call indices 0xFFFFFFFE, 0xFFFFFFFF, 0, 1
R6_CALL0 = 0xFFFFFFFE
_R6_REF = {}  # per case: inputs and the oracle's results, shared by the per-step and the fused run


def _r6_fused(b, cfg, acts, cap, W):
    import torch

    T, B, A = acts.shape
    dev = torch.device("cuda", 0)
    d_a = torch.from_numpy(acts).to(dev)
    o_ = torch.empty((T, B, W), dtype=torch.int64, device=dev)
    r_ = torch.empty((T, B), dtype=torch.int32, device=dev)
    f_ = torch.empty((T, B), dtype=torch.uint8, device=dev)
    n_ = torch.empty((T, B), dtype=torch.int32, device=dev)
    b.env_rollout_multi_device(cfg, T, d_a.data_ptr(), A, o_.data_ptr(), r_.data_ptr(), f_.data_ptr(), n_.data_ptr(),
                               update_cap=cap)
    b.sync()
    return [(o_[t].cpu().numpy().view(np.uint64), r_[t].cpu().numpy(), f_[t].cpu().numpy(),
             n_[t].cpu().numpy().view(np.uint32)) for t in range(T)]


def _r6_reference(key, o, cfgd, st, ns, acts, seed, base, cap):
    """The oracle's R6_T env steps from call index R6_CALL0 (uint32: wraps to 0), once per key; the first step is
    also run with each live high word zeroed and must differ."""
    if key not in _R6_REF:
        refs, s, n = [], st, ns
        for t in range(len(acts)):
            r = o.env_step_multi(cfgd, s, n, acts[t], seed=seed, env_base=base,
                                 call_idx=(R6_CALL0 + t) & 0xFFFFFFFF, update_cap=cap, n_threads=16)
            refs.append(r)
            s, n = r["state"], r["n_steps"]
        for z in on_edges(seed, base, len(st), 0, 0, ctr64=False):
            alt = r6_oracle(o, cfgd, st, ns, acts[0], seed, base, R6_CALL0, cap, zero=z)
            assert not np.array_equal(alt["state"], refs[0]["state"]), f"vacuous: {z}"
        alt = o.env_step_multi(cfgd, st, ns, acts[0], seed=seed, env_base=base, call_idx=0, update_cap=cap,
                               n_threads=16)
        assert not np.array_equal(alt["state"], refs[0]["state"]), "vacuous: call index"
        _R6_REF[key] = refs
    return _R6_REF[key]


def _r6_compare(b, got, refs):
    for t, (ref, g) in enumerate(zip(refs, got)):
        obs, rew, flags, nup = g
        assert np.array_equal(nup, ref["n_updates"]), t
        assert np.array_equal(obs, ref["obs"]) and np.array_equal(rew, ref["reward"]), t
        assert np.array_equal(flags, ref["flags"]), t
    assert np.array_equal(b.get_state(), refs[-1]["state"])
    assert np.array_equal(b.get_n_steps(), refs[-1]["n_steps"])
    assert b.counters()["env_call_count"] == (R6_CALL0 + len(refs)) & 0xFFFFFFFF


R6_SETTINGS = ["all_a", "all_b", "all_top"]


@gpu
@pytest.mark.parametrize("mode", ["per_step", "fused"])
@pytest.mark.parametrize("case", ENV_VARIANT_CASES)
def test_env_kernel_variants_at_the_edges(G, oracle_mod, monkeypatch, case, mode):
    """The case table of test_env_kernel_variants_match_oracle (kernel images 0, 1, 2 and 4, group mode, tail
    thresholds, lanes per wave; tests/r6_cases.py) with a 64-bit seed and env ids straddling 2^32 (or at the top
    of the id field), four env steps from env_call_count 0xFFFFFFFE -- per step, and as one fused launch, in which
    call_idx + t wraps inside the kernel."""
    setting = R6_SETTINGS[ENV_VARIANT_CASES.index(case) % 3]
    c = env_variant_setup(case, monkeypatch)
    net, N, B = c.net, c.net.n_nodes, c.B
    seed, base, _ = edge(setting, B, "direct")
    gnet = G.Net(net)
    cfg = G.EnvConfig(gnet, c.attractors, horizon=3, first_update_tested=c.first)
    o = oracle_mod.Oracle(net)
    cfgd = dict(care=cfg.cube_care, value=cfg.cube_value, target_care=cfg.target_care,
                target_value=cfg.target_value, horizon=3, first_tested=c.first)
    acts = c.rng.integers(0, N + 1, size=(R6_T, B, c.A)).astype(np.int32)
    acts[c.rng.random(acts.shape) < 0.5] = 0
    b = G.PBNBatch(gnet, B, seed=seed, env_id_base=base)
    b.randomize()
    st, ns = b.get_state(), np.zeros(B, np.int64)
    assert np.array_equal(st, o.init_philox(B, seed, base, 0))
    b.set_n_steps(ns)
    b.seek(env_call_count=R6_CALL0)
    refs = _r6_reference(case, o, cfgd, st, ns, acts, seed, base, c.cap)
    if mode == "fused":
        got = _r6_fused(b, cfg, acts, c.cap, net.n_words)
    else:
        got = [b.env_step_multi(cfg, acts[t], update_cap=c.cap) for t in range(R6_T)]
    if "_grp" in c.case:
        assert b.info()["env_lanes"] == int(c.case.split("_grp")[1][0])
    if c.case in ("b28_gen_cap", "b28_first_tested", "b28_gen_cap41") or c.case.startswith("b199_gen_long"):
        assert b.info()["env_kernel"] == 4
    if c.case in ("b28_h8_gen", "b199_h6_gen_first_tested"):
        assert b.info()["env_kernel"] == 2
    _r6_compare(b, got, refs)
    assert (refs[0]["n_updates"] > 1).any()
    b.close()


@gpu
@pytest.mark.parametrize("setting", ["seed_only", "seed_b_only", "base_only", "base_odd_only"])
def test_env_step_single_edges(G, oracle_mod, monkeypatch, setting):
    """One plain R6 path (the tail kernel at its defaults) with each edge alone."""
    c = env_variant_setup("b199_gen_long", monkeypatch)
    net, N, B = c.net, c.net.n_nodes, c.B
    seed, base, _ = edge(setting, B, "direct")
    gnet = G.Net(net)
    cfg = G.EnvConfig(gnet, c.attractors, horizon=3)
    o = oracle_mod.Oracle(net)
    cfgd = dict(care=cfg.cube_care, value=cfg.cube_value, target_care=cfg.target_care,
                target_value=cfg.target_value, horizon=3)
    acts = c.rng.integers(0, N + 1, size=(2, B, c.A)).astype(np.int32)
    b = G.PBNBatch(gnet, B, seed=seed, env_id_base=base)
    b.randomize()
    st, ns = b.get_state(), np.zeros(B, np.int64)
    b.set_n_steps(ns)
    b.seek(env_call_count=R6_CALL0)
    refs = _r6_reference(("single", setting), o, cfgd, st, ns, acts, seed, base, c.cap)
    got = [b.env_step_multi(cfg, acts[t], update_cap=c.cap) for t in range(2)]
    _r6_compare(b, got, refs)
    b.close()


@gpu
@pytest.mark.parametrize("mode", ["per_step", "fused"])
@pytest.mark.parametrize("case", FORCED_TAIL_CASES)
def test_forced_tail_cases_at_the_edges(G, oracle_mod, monkeypatch, case, mode):
    """The forced hand-off / helper / grid-pool shapes of test_tail_handoff_forced_happens_and_matches_oracle (a
    tail session's hand-unrolled Philox rounds, a helper wave's env id rebuilt from the ring's words, the counter
    records re-read by the block draws) with a 64-bit seed and the id wrap inside the batch, from env_call_count
    0xFFFFFFFE. The hand-off (helpers, pool pushes) must happen as there."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench

    B = forced_tail_knobs(case, monkeypatch)
    net = load_network("bittner199")
    gnet = G.Net(net)
    atts, _ = bench.r6_attractors("fixture", net.n_nodes)
    cfg = G.EnvConfig(gnet, atts, horizon=100)
    cfgd = dict(care=cfg.cube_care, value=cfg.cube_value, target_care=cfg.target_care, target_value=cfg.target_value,
                horizon=100)
    o = oracle_mod.Oracle(net)
    # the id wrap inside the batch (env 3 of 6, 5 of 16, 1 of 2); the _off cases at the top of the id field
    seed, base = (SEED_B, (1 << 56) - B) if case.endswith("_off") else (SEED_A, M32 - {6: 3, 16: 5, 2: 1}[B])
    T, A, cap = 2, 4, bench.R6_HIGH_CAP
    st, ns = o.env_reset_philox(np.zeros((B, net.n_words), np.uint64), np.ones(B, np.int64), cfg.reset_care,
                                cfg.reset_value, seed=seed, env_base=base, reset_count=0)
    if ("tail_acts", case) not in _R6_REF:
        _R6_REF["tail_acts", case] = long_first_step_actions(o, cfgd, st, ns, net.n_nodes, (T, B, A), seed, base, cap,
                                                             call_idx=R6_CALL0)
    acts = _R6_REF["tail_acts", case]
    refs = _r6_reference(("tail", case), o, cfgd, st, ns, acts, seed, base, cap)
    b = G.PBNBatch(gnet, B, seed=seed, env_id_base=base)
    b.env_reset(cfg)
    assert np.array_equal(b.get_state(), st)
    b.seek(env_call_count=R6_CALL0)
    if mode == "fused":
        got = _r6_fused(b, cfg, acts, cap, net.n_words)
        handed, helpers, pool = [b.env_handoffs()], [b.env_tail_helpers()], [b.env_grid_stats()]
    else:
        got, handed, helpers, pool = [], [], [], []
        for t in range(T):
            got.append(b.env_step_multi(cfg, acts[t], update_cap=cap))
            handed.append(b.env_handoffs())
            helpers.append(b.env_tail_helpers())
            pool.append(b.env_grid_stats())
    info = b.info()
    assert info["env_kernel"] == 4 and info["env_handoff"] == 1
    assert handed[0] > 0, handed
    assert all(p["gave_up"] == 0 and p["live_at_end"] == 0 for p in pool), pool
    if case == "grid":
        assert pool[0]["pushed"] > 0, pool
    if case == "helpers":
        assert helpers[0] > 0, helpers
    _r6_compare(b, got, refs)
    b.close()


# ----------------------------------------------------------------- SSD
SSD_MODES = {"lane": ("0", "0", "0"), "wave": ("1", "0", "0"), "shared": ("1", "0", "4"), "shared8": ("1", "0", "8"),
             "wave_serial": ("1", "1", "0")}  # PBNSIM_SSD_WAVE, _SERIAL, _SHARED as test_ssd_matches_oracle sets them
SSD_RUNS = ([(m, n, p, s) for m in SSD_MODES for n, p in (("bittner199", 0.0), ("bittner199", 0.01), ("tt8", 0.05))
             for s in ("all_a",)] + [(m, "bittner28", 0.02, "all_b") for m in SSD_MODES]
            + [("lane", "bittner199", 0.01, s) for s in ["all_top"] + ALONE]
            + [("wave", "bittner199", 0.01, s) for s in ("ctr_only", "ctr_far_only")])


@gpu
@pytest.mark.parametrize("mode,name,p,setting", SSD_RUNS)
def test_ssd_at_the_edges(G, oracle_mod, monkeypatch, mode, name, p, setting):
    """The three SSD kernels (one lane, one wave, several waves per env) from ssd_iters 40 (41) below 2^32: 150
    iterations straddle the wrap; a second run continues. The flip stream takes
    the low 32 bits of the counter by design (its c1 is the draw index): pinned as the oracle has it."""
    from gym_pbn_amd.batch import flip_gap_table

    for k, v in zip(("PBNSIM_SSD_WAVE", "PBNSIM_SSD_SERIAL", "PBNSIM_SSD_SHARED"), SSD_MODES[mode]):
        monkeypatch.setenv(k, v)
    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B, iters = 300, 150
    targets = [1, 3, 7] if net.n_nodes < 28 else [0, 5, 9, 20]
    seed, base, ctr = edge(setting, B, "ssd")
    gap = flip_gap_table(net.n_nodes, p)
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    b.randomize()
    s0 = b.get_state()
    b.seek(ssd_iters=ctr)
    h1 = b.ssd_counts(targets, iters, p)
    fn = lambda sl, s, sd, bb, c, n, t0: oracle_mod.ssd_philox(o, s, targets, gap, sd, bb, c, n)
    st, r1 = orc_checked(fn, s0, seed, base, ctr, iters)
    assert np.array_equal(h1, r1) and np.array_equal(b.get_state(), st)
    h2 = b.ssd_counts(targets, 20, p)
    st, r2 = oracle_mod.ssd_philox(o, st, targets, gap, seed, base, ctr + iters, 20)
    assert np.array_equal(h2, r2) and np.array_equal(b.get_state(), st)
    assert b.counters()["ssd_iters"] == ctr + iters + 20
    b.close()


# ----------------------------------------------------------------- synchronous step
SYNC_RUNS = ([(n, p, s) for n, p in (("bittner199", 0.0), ("bittner199", 0.002), ("tt8", 0.05), ("tt200", 0.0))
              for s in ("all_a", "all_b", "all_top")] + [("bittner199", 0.002, s) for s in ALONE])


@gpu
@pytest.mark.parametrize("name,p,setting", SYNC_RUNS)
def test_sync_at_the_edges(G, oracle_mod, name, p, setting):
    """k_sync from sync_steps 3 (4) below 2^32: synch_step(8, p) straddles the wrap in one launch (step_hi << 16
    sits in c1 next to the node pair index); a second call continues. The perturbation stream takes the low 32
    bits of the counter by design: pinned as the oracle has it."""
    from gym_pbn_amd.batch import flip_gap_table

    net = load_network(name)
    o = oracle_mod.Oracle(net)
    B = 600
    seed, base, ctr = edge(setting, B, "sync")
    gap = flip_gap_table(net.n_nodes, p)
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    b.randomize()
    s0 = b.get_state()
    b.seek(sync_steps=ctr)
    b.synch_step(8, p)
    fn = lambda sl, s, sd, bb, c, n, t0: (oracle_mod.sync_philox(o, s, sd, bb, c, n, gap), None)
    want, _ = orc_checked(fn, s0, seed, base, ctr, 8)
    assert np.array_equal(b.get_state(), want)
    b.synch_step(2, p)
    assert np.array_equal(b.get_state(), oracle_mod.sync_philox(o, want, seed, base, ctr + 8, 2, gap))
    assert b.counters()["sync_steps"] == ctr + 10
    b.close()


# ----------------------------------------------------------------- device adapter
@gpu
@pytest.mark.parametrize("setting", ["all_a", "all_b"])
def test_torch_vec_env_at_the_edges(G, oracle_mod, setting):
    """TorchVecPBNTargetMultiEnv (device path, torch's stream) and the host vec env with seed and env_id_base at
    the edge: the same reset and step, and the reset is the oracle's."""
    import torch

    from gym_pbn_amd.envs import VecPBNTargetMultiEnv
    from gym_pbn_amd.torch_env import TorchVecPBNTargetMultiEnv

    z = golden("r6_bittner28.npz")
    att = cubes_to_attractors(z, 28)
    net = load_network("bittner28")
    B, A = 777, 2
    seed, base, _ = edge(setting, B, "direct")
    tv = TorchVecPBNTargetMultiEnv("bittner28", att, B, horizon=3, seed=seed, env_id_base=base, update_cap=4096)
    hv = VecPBNTargetMultiEnv(net, att, B, horizon=3, seed=seed, env_id_base=base, update_cap=4096)
    o_t, o_h = tv.reset(), hv.reset()
    assert np.array_equal(o_t.cpu().numpy(), o_h)
    o = oracle_mod.Oracle(net)
    cfgd = r6_config(z)
    rfn = lambda sl, s, sd, bb, c, n, t0: (o.env_reset_philox(s, np.ones(len(s), np.int64), cfgd["reset_care"],
                                                             cfgd["reset_value"], seed=sd, env_base=bb)[0], None)
    st, _ = orc_checked(rfn, np.zeros((B, 1), np.uint64), seed, base, 0, 1, ctr64=False)
    assert np.array_equal(hv.batch.get_state(), st)
    a = np.random.default_rng(4).integers(0, 29, size=(B, A)).astype(np.int32)
    ot, rt, tt, trt, it = tv.step(torch.from_numpy(a).cuda())
    oh, rh, th, trh, ih = hv.step(a)
    ref = o.env_step_multi(dict(cfgd, horizon=3), st, np.zeros(B, np.int64), a, seed=seed, env_base=base, call_idx=0,
                           update_cap=4096)
    assert np.array_equal(ot.cpu().numpy(), oh) and np.array_equal(rt.cpu().numpy(), rh)
    assert np.array_equal(tt.cpu().numpy(), th) and np.array_equal(trt.cpu().numpy(), trh)
    assert np.array_equal(it["n_updates"].cpu().numpy().view(np.uint32), ih["n_updates"])
    assert np.array_equal(ih["n_updates"], ref["n_updates"]) and np.array_equal(rh, ref["reward"])
    assert np.array_equal(tv.batch.get_state(), ref["state"]) and np.array_equal(hv.batch.get_state(), ref["state"])
    tv.close()
