"""The until-attractor multi-flip env over an exact labelled state set: k_env_set, k_env_set_reset, their entry
points and ``TorchVecPBNTargetMultiSetEnv``. Every comparison is bit-exact.

Expected values never come from the new code: ``test_matches_oracle`` takes them from the C oracle
(``orc_env_step_multi`` with the set handed over as one full-care cube per member), the twin tests from the cube
kernel ``k_env`` on a batch of the same seed, the reset test from the documented draw (``bitmodel.draw``, stream 9).
"""

import functools

import numpy as np
import pytest

import bitmodel
from shape_cases import edge_actions, shape_net

pytestmark = pytest.mark.gpu

SENTINEL = -77
SEED = (3 << 32) | 17
B, A, CAP, HORIZON, CALLS = 549, 3, 64, 3, 4  # 549 = 2 x 256 + 37: one workgroup strides three times, the last ragged
BIG_BASE = (1 << 40) + 3
CASES = [(k, n, 0) for k in ("pm", "tt") for n in (63, 65, 257, 512)] + [("tt", 257, BIG_BASE)]
PROBE_CAPS = (0, 1, 2, 3, 5, 9)
FREE = (0, 2, 5)  # free nodes of the three attractors' cubes: 1, 4 and 32 states
BLOCK_C = np.arange(100, 400)  # envs started one flip away from attractor 2 (see _case)
STREAM_ENV, STREAM_TENV_RESET = 3, 9


def _dev(a):
    import torch

    a = np.array(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _bit(W, i):
    m = np.zeros(W, np.uint64)
    m[i // 64] = np.uint64(1) << np.uint64(i % 64)
    return m


def _full(N, W):
    m = np.full(W, ~np.uint64(0))
    if N % 64:
        m[-1] = (np.uint64(1) << np.uint64(N % 64)) - np.uint64(1)
    return m


def _flip_mask(row, N, W):
    """The words k_flip / apply_actions change for one action row (offset 1, dedup, Python indexing)."""
    m = np.zeros(W, np.uint64)
    for a in sorted(set(int(v) for v in row)):
        if a != 0:
            m ^= _bit(W, (a - 1) % N)
    return m


def _cube(x, free, N, W):
    """(care [W], value [W], members [2^f][W]) of the cube around state x with ``free`` nodes free."""
    care = _full(N, W)
    for i in free:
        care &= ~_bit(W, i)
    value = x & care
    rows = [value.copy()]
    for i in free:
        rows = rows + [r | _bit(W, i) for r in rows]
    return care, value, np.array(rows, np.uint64)


def _cfg(care, value, target_care, target_value):
    return dict(care=care, value=value, target_care=target_care, target_value=target_value, horizon=HORIZON)


@functools.lru_cache(maxsize=None)
def _case(kind, N, base):
    """Everything test_matches_oracle needs, from the oracle alone (no GPU call is made here).

    Call 0's states after exactly 0, 1, 2, 3, 5 and 9 updates come from oracle runs against one cube nothing matches.
    Three attractors, each one cube around such a state, so the oracle's single target cube can be any of them:
      0  (no free node)    the snapshot of env pA: that env ends at update 1 through the snapshot test
      1  (2 free nodes)    the state of env pB after update 2, where update 1 changed a node and update 2 none, and
                           the free nodes are not the changed one: the snapshot is no member, and the env ends at
                           exactly update 2 only if update 2 looks up although it changed nothing
      2  (5 free nodes)    a state X of env 50 after 9 updates. The envs of BLOCK_C start (after their flips) at X
                           with the node their third update draws flipped, so those whose first two updates change
                           nothing outside the free nodes and whose third restores the node end at update 3, others
                           later or never
    The remaining envs start at random states and are capped.
    """
    import oracle as O

    net = shape_net(kind, N)
    W = net.n_words
    orc = O.Oracle(net)
    rng = np.random.default_rng(1000 * N + (kind == "tt") + base % 7)
    acts = [edge_actions(rng, B, A, N) for _ in range(CALLS)]
    for a in acts:
        a[4] = [-1, 0, 5]  # a negative index: -1 - 1 -> node N - 2
        a[5] = [7, 7, 7]   # duplicates: node 6 flips once
    init = orc.init_philox(B, SEED, base)
    none = _cfg(np.zeros((1, W), np.uint64), np.array([[1] + [0] * (W - 1)], np.uint64), np.zeros(W, np.uint64),
                np.array([1] + [0] * (W - 1), np.uint64))
    zeros = np.zeros(B, np.int64)

    def probe(state):
        return {c: orc.env_step_multi(none, state, zeros, acts[0], seed=SEED, env_base=base, call_idx=0,
                                      update_cap=c)["state"] for c in PROBE_CAPS}

    X = probe(init)[9][50]
    free2 = sorted(int(i) for i in rng.choice(np.arange(1, N), size=FREE[2], replace=False))
    for q in BLOCK_C:
        w = bitmodel.draw(SEED, 1, 0, base + int(q), STREAM_ENV)  # update 3 = index 2: call 2 >> 1, words 0 and 1
        node = (w[0] * N) >> 32 if kind == "pm" else 1 + ((w[0] * (N - 1)) >> 32)
        init[q] = X ^ _bit(W, node) ^ _flip_mask(acts[0][q], N, W)
    T = probe(init)
    assert all(sum(bin(int(w)).count("1") for w in T[0][q] ^ X) == 1 for q in BLOCK_C), "a snapshot is not X ^ one node"
    rest = [e for e in range(6, B) if e not in set(BLOCK_C.tolist()) and e != 50]
    pA = rest[0]
    pB = next(e for e in rest[1:] if np.array_equal(T[1][e], T[2][e]) and not np.array_equal(T[0][e], T[1][e]))
    changed = T[0][pB] ^ T[2][pB]
    assert sum(bin(int(w)).count("1") for w in changed) == 1
    free1 = []
    while len(free1) < FREE[1]:
        i = int(rng.integers(1, N))
        if i not in free1 and not (changed & _bit(W, i)).any():
            free1.append(i)
    cubes = [_cube(T[0][pA], [], N, W), _cube(T[2][pB], free1, N, W), _cube(X, free2, N, W)]
    members = np.concatenate([c[2] for c in cubes])
    labels = np.concatenate([np.full(len(c[2]), k, np.int32) for k, c in enumerate(cubes)])
    full = np.tile(_full(N, W), (len(members), 1))
    target = rng.integers(0, 3, size=B).astype(np.int32)
    target[pA], target[pB] = 0, 2  # one lands in its target, one in another attractor

    # the oracle, once per target label: the dynamics do not depend on the target
    runs, state, ns = [], init, zeros
    for c in range(CALLS):
        per = [orc.env_step_multi(_cfg(full, members, cubes[t][0], cubes[t][1]), state, ns, acts[c], seed=SEED,
                                  env_base=base, call_idx=c, update_cap=CAP) for t in range(3)]
        for k in ("state", "n_steps", "obs", "n_updates"):
            assert np.array_equal(per[0][k], per[1][k]) and np.array_equal(per[0][k], per[2][k])
        e = np.arange(B)
        r = dict(per[0])
        r["reward"] = np.stack([p["reward"] for p in per])[target, e]
        r["flags"] = np.stack([p["flags"] for p in per])[target, e]
        runs.append(r)
        state, ns = r["state"], r["n_steps"]

    # a weak input cannot hide a failure: the oracle's own outputs of call 0 reach every path
    r0 = runs[0]
    nup, capped = r0["n_updates"], (r0["flags"] & 4) != 0
    assert nup[pA] == 1 and np.array_equal(r0["obs"][pA], T[0][pA]), "no env ends through the snapshot test"
    assert nup[pB] == 2 and np.array_equal(T[1][pB], T[2][pB]), "no env ends at an unchanged update 2"
    assert ((nup >= 3) & (nup < CAP) & ~capped).sum() >= 8, "too few envs end in [3, cap)"
    assert capped.sum() >= 8 and (nup[capped] == CAP).all()
    assert (r0["flags"][pA] & 1) and not (r0["flags"][pB] & 1)
    assert any(((r["flags"] & 2) != 0).any() for r in runs[:3]), "no env is truncated by call 3"
    for a in (init, members, labels, target, *acts):
        a.setflags(write=False)
    return net, init, acts, members, labels, target, runs


@pytest.mark.parametrize("kind,N,base", CASES)
def test_matches_oracle(kind, N, base, monkeypatch):
    """N = 63: W = 1; 65: a word boundary; 257: odd W = 5, 8-byte-aligned set rows; 512: W = 8, no tail mask."""
    import torch

    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    net, init, acts, members, labels, target, runs = _case(kind, N, base)
    W = net.n_words
    host = StateSet(members, N, labels=labels, device=None)
    landed = host.lookup(runs[0]["obs"])
    assert set(landed[(runs[0]["flags"] & 4) == 0].tolist()) == {0, 1, 2}, "a label is never landed in"
    monkeypatch.setenv("PBNSIM_ENVSET_GRID", "1")
    b = PBNBatch(Net(net), B, env_id_base=base, seed=SEED)
    b.set_state(init)
    sset = StateSet(members, N, labels=labels, device=0)
    full = functools.partial(torch.full, device="cuda:0")
    obs, rew = full((B, W), SENTINEL, dtype=torch.int64), full((B,), SENTINEL, dtype=torch.int32)
    flags, nup = full((B,), 99, dtype=torch.uint8), full((B,), SENTINEL, dtype=torch.int32)
    lab = full((B,), SENTINEL, dtype=torch.int32)
    d_target = _dev(target)
    for c in range(CALLS):
        d_act = _dev(acts[c])
        torch.cuda.synchronize()
        b.env_set_step_device(sset, d_act.data_ptr(), A, obs.data_ptr(), rew.data_ptr(), flags.data_ptr(),
                              nup.data_ptr(), lab.data_ptr(), d_target_labels=d_target.data_ptr(), update_cap=CAP,
                              horizon=HORIZON)
        b.sync()
        ref = runs[c]
        got_nup = nup.cpu().numpy().view(np.uint32)
        print(f"call {c}: n_updates mismatches {(got_nup != ref['n_updates']).sum()}")
        assert np.array_equal(got_nup, ref["n_updates"]), c
        assert np.array_equal(b.get_state(), ref["state"]), c
        assert np.array_equal(b.get_n_steps(), ref["n_steps"]), c
        assert np.array_equal(obs.cpu().numpy().view(np.uint64), ref["obs"]), c
        assert np.array_equal(rew.cpu().numpy(), ref["reward"]), c
        assert np.array_equal(flags.cpu().numpy(), ref["flags"]), c
        want_label = np.where((ref["flags"] & 4) != 0, -1, host.lookup(ref["obs"]))
        assert np.array_equal(lab.cpu().numpy(), want_label), c
        assert b.counters()["env_call_count"] == c + 1
    b.env_set_check()  # no row was invalid
    b.close()
    sset.close()


# ---------------------------------------------------------------------------------------------- against k_env
class _Out:
    """Device outputs of one env step, prefilled so that an untouched row shows."""

    def __init__(self, n, W):
        import torch

        full = functools.partial(torch.full, device="cuda:0")
        self.obs = full((n, W), SENTINEL, dtype=torch.int64)
        self.rew = full((n,), SENTINEL, dtype=torch.int32)
        self.flags = full((n,), 99, dtype=torch.uint8)
        self.nup = full((n,), SENTINEL, dtype=torch.int32)
        self.lab = full((n,), SENTINEL, dtype=torch.int32)
        torch.cuda.synchronize()

    def cube_step(self, batch, cfg, d_act, n_act, cap):
        batch.env_step_multi_device(cfg, d_act.data_ptr(), n_act, self.obs.data_ptr(), self.rew.data_ptr(),
                                    self.flags.data_ptr(), self.nup.data_ptr(), update_cap=cap)
        batch.sync()
        return self.host()

    def set_step(self, batch, sset, d_act, n_act, cap, **kw):
        batch.env_set_step_device(sset, d_act.data_ptr(), n_act, self.obs.data_ptr(), self.rew.data_ptr(),
                                  self.flags.data_ptr(), self.nup.data_ptr(), self.lab.data_ptr(), update_cap=cap,
                                  **kw)
        batch.sync()
        return self.host()

    def host(self):
        return dict(obs=self.obs.cpu().numpy().view(np.uint64), reward=self.rew.cpu().numpy(),
                    flags=self.flags.cpu().numpy(), n_updates=self.nup.cpu().numpy(), label=self.lab.cpu().numpy())


def _same_step(cube, sset_out, cube0_only, n_labels, sset, ok):
    """k_env's outputs against k_env_set's with target = the last attractor. k_env's target is the last attractor's
    first cube alone (in_target, pbn_target_multi.py:190-199): with a last attractor of one cube every field is
    equal; with more, k_env's terminated implies the set's, and reward and flags agree once that bit is taken out."""
    for k in ("obs", "n_updates"):
        assert np.array_equal(cube[k], sset_out[k]), k
    term_c, term_s = cube["flags"] & 1, sset_out["flags"] & 1
    assert np.array_equal(cube["flags"] & 6, sset_out["flags"] & 6)
    assert np.array_equal(cube["reward"] - 1000 * term_c.astype(np.int32),
                          sset_out["reward"] - 1000 * term_s.astype(np.int32))
    if cube0_only:
        assert np.array_equal(cube["flags"], sset_out["flags"]) and np.array_equal(cube["reward"], sset_out["reward"])
    assert (term_c[ok] <= term_s[ok]).all()
    want = np.where((sset_out["flags"][ok] & 4) != 0, -1, sset.lookup(sset_out["obs"][ok]))
    assert np.array_equal(sset_out["label"][ok], want)
    assert np.array_equal(term_s[ok] != 0, sset_out["label"][ok] == n_labels - 1)


def test_equals_cube_kernel_on_found_attractors():
    from gym_pbn_amd.attractors import find_attractors
    from gym_pbn_amd.batch import EnvConfig, Net, PBNBatch

    n, n_act, cap = 4096, 2, 4096
    net = Net("bittner28")
    N, W = net.n_nodes, net.n_words
    res = find_attractors("bittner28", n_seeds=256)
    assert res.attractors
    cubes = res.all_attractors()
    cfg = EnvConfig(net, cubes)
    sset = res.state_set()
    K = len(res.attractors)
    assert sset.n_labels == K
    rng = np.random.default_rng(28)
    one, two = PBNBatch(net, n, seed=9), PBNBatch(net, n, seed=9)
    one.randomize()
    two.set_state(one.get_state())
    two.seek(reset_count=one.counters()["reset_count"])
    bad = 77
    for call in range(3):
        acts = rng.integers(0, N + 1, size=(n, n_act)).astype(np.int32)
        acts[bad] = [3, N + 1]  # names no node: the env is skipped by both kernels
        d_act = _dev(acts)
        ok = np.arange(n) != bad
        o1, o2 = _Out(n, W), _Out(n, W)
        c = o1.cube_step(one, cfg, d_act, n_act, cap)
        s = o2.set_step(two, sset, d_act, n_act, cap, target_label=K - 1)
        _same_step(c, s, len(cubes[-1]) == 1, K, sset, ok)
        for h in (c, s):  # the bad row: untouched by both
            assert (h["obs"][bad].view(np.int64) == SENTINEL).all() and h["flags"][bad] == 99
            assert h["reward"][bad] == SENTINEL and h["n_updates"][bad] == SENTINEL
        assert s["label"][bad] == SENTINEL
        assert np.array_equal(one.get_state(), two.get_state())
        assert np.array_equal(one.get_n_steps(), two.get_n_steps()) and one.get_n_steps()[bad] == 0
        assert one.counters() == two.counters()
    with pytest.raises(ValueError, match="Invalid action"):
        two.env_set_check()
    two.env_set_check()  # reported once
    # one call of each kind on the same batch against the twin that makes both with k_env
    ok = np.ones(n, bool)
    for kind_first in ("set", "cube"):
        acts = rng.integers(0, N + 1, size=(n, n_act)).astype(np.int32)
        d_act = _dev(acts)
        o1, o2 = _Out(n, W), _Out(n, W)
        c = o1.cube_step(one, cfg, d_act, n_act, cap)
        if kind_first == "set":
            s = o2.set_step(two, sset, d_act, n_act, cap, target_label=K - 1)
            _same_step(c, s, len(cubes[-1]) == 1, K, sset, ok)
        else:
            s = o2.cube_step(two, cfg, d_act, n_act, cap)
            for k in ("obs", "reward", "flags", "n_updates"):
                assert np.array_equal(c[k], s[k]), k
        assert np.array_equal(one.get_state(), two.get_state())
        assert one.counters() == two.counters()
    one.close()
    two.close()
    sset.close()


# ---------------------------------------------------------------------------------------------- reset
@pytest.mark.parametrize("kind", ["pm", "tt"])
def test_reset_draws_the_documented_rows(kind):
    import torch

    from gym_pbn_amd.batch import Net, PBNBatch

    N, n, base, seed = 65, 300, 5, 11
    net = shape_net(kind, N)
    W = net.n_words
    rng = np.random.default_rng(65 + (kind == "tt"))
    sizes = [1, 4, 7]
    rows = rng.integers(0, 1 << 63, size=(sum(sizes), W), dtype=np.uint64)
    rows[:, -1] &= np.uint64(1)  # N = 65: one node in the last word
    rows[:, 0] |= np.uint64(1)   # node 0 set in every row: cleared for tables only
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    src = rng.integers(0, 3, size=n).astype(np.int32)
    src[[7, 260]] = [3, -1]  # no such attractor
    mask = (rng.random(n) < 0.6).astype(np.uint8)
    mask[[7, 260, 0]] = 1
    mask[1] = 0
    b = PBNBatch(Net(net), n, env_id_base=base, seed=seed)
    b.randomize()
    b.set_n_steps(np.full(n, 5))
    s0 = b.get_state()
    rc = b.counters()["reset_count"]
    d_rows, d_off, d_src, d_mask = _dev(rows), _dev(row_off), _dev(src), _dev(mask)
    torch.cuda.synchronize()
    clear = ~np.uint64(1) if kind == "tt" else ~np.uint64(0)

    def picks(reset_count, source):
        out = np.empty((n, W), np.uint64)
        for e in range(n):
            k = int(source[e]) if 0 <= source[e] < 3 else 0
            w = bitmodel.draw(seed, 0, reset_count, base + e, STREAM_TENV_RESET)
            out[e] = rows[int(row_off[k]) + ((w[0] * sizes[k]) >> 32)]
        out[:, 0] &= clear
        return out

    b.env_set_reset_device(d_rows.data_ptr(), d_off.data_ptr(), 3, d_source_labels=d_src.data_ptr(),
                           d_mask=d_mask.data_ptr())
    b.sync()
    took = (mask != 0) & (src >= 0) & (src < 3)
    assert took.sum() > 100 and (~took).sum() > 50
    assert np.array_equal(b.get_state(), np.where(took[:, None], picks(rc, src), s0))
    assert np.array_equal(b.get_n_steps(), np.where(took, 0, 5))
    assert b.counters()["reset_count"] == rc + 1
    with pytest.raises(ValueError, match="source attractor"):
        b.env_set_check()
    b.env_set_check()  # reported once
    # every env, one source for all
    b.env_set_reset_device(d_rows.data_ptr(), d_off.data_ptr(), 3, source_label=2)
    b.sync()
    assert np.array_equal(b.get_state(), picks(rc + 1, np.full(n, 2)))
    assert (b.get_n_steps() == 0).all() and b.counters()["reset_count"] == rc + 2
    b.env_set_check()
    b.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    import torch

    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.stateset import StateSet

    n = 8
    b = PBNBatch("bittner28", n, seed=1)
    b.randomize()
    s0, c0 = b.get_state(), b.counters()
    out = _Out(n, 1)
    good = StateSet(np.array([[1], [2]], np.uint64), 28, labels=[0, 1], device=0)
    d_act = _dev(np.zeros((n, 2), np.int32))
    d_target = _dev(np.zeros(n, np.int32))
    torch.cuda.synchronize()

    def call(sset=good, n_act=2, **kw):
        b.env_set_step_device(sset, d_act.data_ptr(), n_act, out.obs.data_ptr(), out.rew.data_ptr(),
                              out.flags.data_ptr(), out.nup.data_ptr(), out.lab.data_ptr(), **kw)

    with pytest.raises(ValueError, match="A=0"):
        call(n_act=0)
    with pytest.raises(ValueError, match="27 nodes"):
        call(sset=StateSet(np.array([[1]], np.uint64), 27, device=0))
    with pytest.raises(ValueError, match="host-only"):
        call(sset=StateSet(np.array([[1]], np.uint64), 28, device=None))
    for t in (-1, 2):
        with pytest.raises(ValueError, match="target_label"):
            call(target_label=t)
    with pytest.raises(ValueError, match="n_labels"):
        b.env_set_reset_device(d_act.data_ptr(), d_act.data_ptr(), 0)
    b.sync()
    assert np.array_equal(b.get_state(), s0) and b.counters() == c0
    h = out.host()
    assert (h["reward"] == SENTINEL).all() and (h["flags"] == 99).all() and (h["label"] == SENTINEL).all()
    call(target_label=7, d_target_labels=d_target.data_ptr())  # the scalar is not read when per-env targets are given
    b.sync()
    assert b.counters()["env_call_count"] == c0["env_call_count"] + 1
    b.close()
    good.close()


# ---------------------------------------------------------------------------------------------- env class
def _tt8_attractors():
    from gym_pbn_amd.network import load_network
    from gym_pbn_amd.stg import compute_attractors

    return [sorted(a) for a in compute_attractors(load_network("tt8"))]


@pytest.mark.parametrize("name", ["tt8", "bittner28"])
def test_env_class(name):
    import torch

    import gym_pbn_amd
    from gym_pbn_amd.batch import PBNBatch

    n, seed, n_act = 300, 4, 2
    attractors = _tt8_attractors() if name == "tt8" else "find"
    kw = dict(n_envs=n, seed=seed, horizon=2, update_cap=512)
    env = gym_pbn_amd.TorchVecPBNTargetMultiSetEnv(name, attractors, **kw)
    N, W, K = env.N, env.W, env.n_attractors
    assert K >= 1 and env.set.n_labels == K and len(env.set) == int(env.row_off[-1])
    assert env.observation_space.shape == (N,) and type(env.action_space).__name__ == "MultiDiscrete"
    assert (env.source == 0).all().item() and (env.target == K - 1).all().item()
    twin = PBNBatch(env.net, n, seed=seed)
    rng = np.random.default_rng(8)
    src = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    tgt = torch.full((n,), K - 1, dtype=torch.int32, device="cuda:0")

    def twin_reset(mask=None):
        torch.cuda.synchronize()
        twin.env_set_reset_device(env._rows.data_ptr(), env._row_off.data_ptr(), K, d_source_labels=src.data_ptr(),
                                  d_mask=0 if mask is None else mask.data_ptr())
        twin.sync()

    def same_state():
        torch.cuda.synchronize()
        assert np.array_equal(env.observation_words().cpu().numpy().view(np.uint64), twin.get_state())
        assert np.array_equal(env.batch.get_n_steps(), twin.get_n_steps())
        assert env.batch.counters() == twin.counters()

    obs = env.reset()
    twin_reset()
    same_state()
    assert obs.dtype == torch.uint8 and obs.shape == (n, N)
    mask = _dev((rng.random(n) < 0.5).astype(np.uint8))
    new_src = _dev(rng.integers(0, K, size=n).astype(np.int32))
    new_tgt = _dev(rng.integers(0, K, size=n).astype(np.int32))
    env.reset(mask=mask, source=new_src, target=new_tgt)
    src = torch.where(mask != 0, new_src, src).contiguous()
    tgt = torch.where(mask != 0, new_tgt, tgt).contiguous()
    assert torch.equal(env.source, src) and torch.equal(env.target, tgt)
    twin_reset(mask)
    same_state()
    env.reset(mask=mask, target=0)  # an int, for the masked envs; the sources are kept
    tgt = torch.where(mask != 0, torch.zeros_like(tgt), tgt).contiguous()
    assert torch.equal(env.source, src) and torch.equal(env.target, tgt)
    twin_reset(mask)
    same_state()
    ended = 0
    for t in range(3):
        acts = rng.integers(0, N + 1, size=(n, n_act)).astype(np.int32)
        d_act = _dev(acts)
        obs, reward, term, trunc, info = env.step(d_act)
        out = _Out(n, W)
        got = out.set_step(twin, env.set, d_act, n_act, 512, d_target_labels=tgt.data_ptr(), horizon=2)
        same_state()
        assert obs.dtype == torch.uint8 and obs.shape == (n, N)
        assert reward.dtype == torch.int32 and reward.shape == (n,)
        assert term.dtype == torch.bool and trunc.dtype == torch.bool and term.shape == trunc.shape == (n,)
        assert info["obs_words"].dtype == torch.int64 and info["obs_words"].shape == (n, W)
        assert info["n_updates"].dtype == torch.int32 and info["label"].dtype == torch.int32
        assert info["capped"].dtype == torch.bool
        assert np.array_equal(info["obs_words"].cpu().numpy().view(np.uint64), got["obs"])
        assert np.array_equal(reward.cpu().numpy(), got["reward"])
        assert np.array_equal(term.cpu().numpy(), (got["flags"] & 1) != 0)
        assert np.array_equal(trunc.cpu().numpy(), (got["flags"] & 2) != 0)
        assert np.array_equal(info["capped"].cpu().numpy(), (got["flags"] & 4) != 0)
        assert np.array_equal(info["n_updates"].cpu().numpy(), got["n_updates"])
        assert np.array_equal(info["label"].cpu().numpy(), got["label"])
        label = info["label"].cpu().numpy()
        assert np.array_equal(term.cpu().numpy(), (label >= 0) & (label == tgt.cpu().numpy()))
        bits = (got["obs"][:, 0:1] >> np.arange(N, dtype=np.uint64)) & np.uint64(1)
        assert np.array_equal(obs.cpu().numpy(), bits.astype(np.uint8))
        assert trunc.all().item() == (t == 1)  # horizon 2: the second step of every env
        ended += int(term.sum().item())
    assert ended > 0
    with pytest.raises(ValueError, match="attractor"):
        env.reset(source=K)
    rows = env._rows.cpu().numpy().view(np.uint64)
    packed = [rows[int(env.row_off[k]):int(env.row_off[k + 1])].copy() for k in range(K)]
    env.close()

    # auto_reset (attractors as packed arrays): the envs that ended are reset as a masked reset of the twin resets them
    env = gym_pbn_amd.TorchVecPBNTargetMultiSetEnv(name, packed, auto_reset=True, **kw)
    twin2 = PBNBatch(env.net, n, seed=seed)
    env.reset()
    twin_src = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    tgt = torch.full((n,), K - 1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    twin2.env_set_reset_device(env._rows.data_ptr(), env._row_off.data_ptr(), K, d_source_labels=twin_src.data_ptr())
    done_total = 0
    for t in range(3):
        d_act = _dev(rng.integers(0, N + 1, size=(n, n_act)).astype(np.int32))
        _, _, term, trunc, _ = env.step(d_act)
        got = _Out(n, W).set_step(twin2, env.set, d_act, n_act, 512, d_target_labels=tgt.data_ptr(), horizon=2)
        done = _dev((((got["flags"] & 3) != 0)).astype(np.uint8))
        assert np.array_equal((term | trunc).cpu().numpy(), done.cpu().numpy() != 0)
        torch.cuda.synchronize()
        twin2.env_set_reset_device(env._rows.data_ptr(), env._row_off.data_ptr(), K,
                                   d_source_labels=twin_src.data_ptr(), d_mask=done.data_ptr())
        twin2.sync()
        torch.cuda.synchronize()
        assert np.array_equal(env.observation_words().cpu().numpy().view(np.uint64), twin2.get_state())
        assert np.array_equal(env.batch.get_n_steps(), twin2.get_n_steps())
        assert env.batch.counters() == twin2.counters()
        done_total += int((done != 0).sum().item())
    assert 0 < done_total
    env.close()
    twin.close()
    twin2.close()
