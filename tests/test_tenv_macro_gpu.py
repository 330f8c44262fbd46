"""The macro-action envs on the device: the fused macro step (k_tenv_macro, both modes) and the two env classes
on top of it. Every comparison is bit-exact, float64 rewards included.

Expected values come from the primitives the kernel fuses, on a twin batch of the same seed: ``t_max`` rounds of
``PBNBatch.flip(offset=1)`` + ``step(1)``, the state recorded after each, host ``StateSet.lookup`` per round. The
self-triggering stop draws are recomputed here from the documented counter (``bitmodel.draw``, stream 10) and the
discounted reward is accumulated in Python, in the reference's order (``self_triggering.py:77``).
"""

import functools
import json

import numpy as np
import pytest

import bitmodel
from conftest import GOLDEN
from shape_cases import SHAPES, edge_nodes, tt_net

pytestmark = pytest.mark.gpu

KAT = json.loads((GOLDEN / "mdp_kat.json").read_text())
SENTINEL = -77
INTERVAL, TRIGGER = 0, 1
T_MAX = 5
GAMMA = 0.99
SEED = 5
U0 = (1 << 32) - 2  # the rounds of one macro step run across the low counter word's end
STREAM_TENV_TRIGGER = 10
SHAPE_CASES = [("tt6", 257, 0), ("tt6", 2, 1), ("tt200", 257, 0), ("tt200", 2, 1)]


def _tt6_source():
    net = KAT["networks"]["tt6"]
    return [(np.array(d["mask"], dtype=bool), np.array(d["table"]).reshape((2,) * sum(d["mask"])), d["name"],
             d["control"]) for d in net["PBN_data"]]


@functools.lru_cache(maxsize=None)
def _net(name):
    from gym_pbn_amd.batch import Net
    from gym_pbn_amd.network import TruthTableNetwork, load_network

    if isinstance(name, int):
        return Net(tt_net(name))
    return Net(TruthTableNetwork.from_pbn_data(_tt6_source()) if name == "tt6" else load_network(name))


def _dev(a):
    import torch

    a = np.array(a)  # a copy: the shared case arrays are read-only
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to("cuda:0")


def _tables(t_max):
    from gym_pbn_amd.macro_env import gamma_powers, stop_thresholds

    return gamma_powers(GAMMA, t_max), stop_thresholds()


def _records(net, B, base, seed, s0, u0, acts, t_max):
    """The calls the kernel fuses, on a twin: [t_max][B][W] states after round 0, 1, ..."""
    from gym_pbn_amd.batch import PBNBatch

    twin = PBNBatch(net, B, env_id_base=base, seed=seed)
    twin.set_state(s0)
    twin.seek(update_count=u0)
    rec = []
    for _ in range(t_max):
        if acts.any():
            twin.flip(acts[:, None], offset=1, dedup=True)
        twin.step(1)
        rec.append(twin.get_state())
    assert twin.counters()["update_count"] == u0 + t_max
    twin.close()
    return np.stack(rec)


def _stop_rounds(seed, base, u0, probs, t_max, thr):
    """Rounds run per env in trigger mode and whether the env's own draw ended them."""
    n, by_draw = [], []
    for e, p in enumerate(probs):
        g = base + e
        for i in range(t_max):
            u = u0 + i
            w = bitmodel.draw(seed, u & 0xFFFFFFFF, u >> 32, g, STREAM_TENV_TRIGGER)
            k53 = ((w[0] >> 5) << 26) | (w[1] >> 6)
            drawn = k53 <= int(thr[p])
            if drawn or i + 1 == t_max:
                break
        n.append(i + 1)
        by_draw.append(drawn)
    return np.array(n), np.array(by_draw)


def _expect(rec, labels, acts, rounds, mode, gpow):
    """What the macro step returns for envs that run rounds[e] rounds over the recorded states."""
    B = rec.shape[1]
    out = dict(state=np.empty_like(rec[0]), label=np.empty(B, np.int32), flags=np.empty(B, np.uint8),
               first_hit=np.empty(B, np.int32), interval=rounds.astype(np.int32),
               reward=np.empty(B, np.int32 if mode == INTERVAL else np.float64))
    for e in range(B):
        k = int(rounds[e])
        total = 0  # as the reference starts it: an int, a float from the first discounted term on
        hit = -1
        for i in range(k):
            term = labels[i][e] >= 0
            r = 20 if term else -4 - int(acts[e] != 0)
            total = total + r if mode == INTERVAL else total + (GAMMA ** i) * r
            assert mode == INTERVAL or gpow[i] == GAMMA ** i
            if term and hit < 0:
                hit = i
        out["state"][e] = rec[k - 1][e]
        out["label"][e] = labels[k - 1][e]
        out["flags"][e] = labels[k - 1][e] >= 0
        out["first_hit"][e] = hit
        out["reward"][e] = total
    return out


class _Out:
    """Device output buffers of one macro step, prefilled so that an untouched row shows."""

    def __init__(self, B, W):
        import torch

        full = functools.partial(torch.full, device="cuda:0")
        self.obs = full((B, W), SENTINEL, dtype=torch.int64)
        self.reward_i32 = full((B,), SENTINEL, dtype=torch.int32)
        self.reward_f64 = full((B,), float(SENTINEL), dtype=torch.float64)
        self.flags = full((B,), 99, dtype=torch.uint8)
        self.label = full((B,), SENTINEL, dtype=torch.int32)
        self.interval = full((B,), SENTINEL, dtype=torch.int32)
        self.first_hit = full((B,), SENTINEL, dtype=torch.int32)
        torch.cuda.synchronize()

    def step(self, batch, target, mode, t_max, actions, limits, check=False):
        import torch

        a, lim = _dev(np.asarray(actions, dtype=np.int32)), _dev(np.asarray(limits, dtype=np.int32))
        gpow, thr = (_dev(t) for t in _tables(t_max))
        torch.cuda.synchronize()
        kw = dict(d_reward_i32=self.reward_i32.data_ptr()) if mode == INTERVAL else dict(
            d_reward_f64=self.reward_f64.data_ptr(), d_gpow=gpow.data_ptr(), d_stop_thr=thr.data_ptr())
        batch.tenv_macro_device(target, mode, t_max, a.data_ptr(), lim.data_ptr(), self.flags.data_ptr(),
                                d_obs=self.obs.data_ptr(), d_interval=self.interval.data_ptr(),
                                d_first_hit=self.first_hit.data_ptr(), d_labels=self.label.data_ptr(), check=check,
                                **kw)
        batch.sync()
        reward = self.reward_i32 if mode == INTERVAL else self.reward_f64
        return dict(obs=self.obs.cpu().numpy().view(np.uint64), reward=reward.cpu().numpy(),
                    flags=self.flags.cpu().numpy(), label=self.label.cpu().numpy(),
                    interval=self.interval.cpu().numpy(), first_hit=self.first_hit.cpu().numpy())


def _assert_equal(got, want, state, rows=slice(None)):
    assert np.array_equal(state[rows], want["state"][rows])
    assert np.array_equal(got["obs"][rows], want["state"][rows])
    assert np.array_equal(got["label"][rows], want["label"][rows])
    assert np.array_equal(got["flags"][rows], want["flags"][rows])
    assert np.array_equal(got["interval"][rows], want["interval"][rows])
    assert np.array_equal(got["first_hit"][rows], want["first_hit"][rows])
    assert got["reward"].dtype == want["reward"].dtype
    assert (got["reward"][rows] == want["reward"][rows]).all()  # == on float64 too: bit-exact up to the zero's sign


def _actions(rng, B, N):
    a = rng.integers(1, N + 1, size=B).astype(np.int32)  # a flips node a - 1: node 0 (a = 1) .. node N - 1 (a = N)
    a[rng.random(B) < 0.5] = 0
    if B >= 4:
        a[:4] = [1, N, 0, N // 2]
    return a


@functools.lru_cache(maxsize=None)
def _case(name, B, base):
    """One start state, one action row and the twin's records per shape, shared by both modes' tests; the target
    holds about half of the recorded states under labels 0..4, so both reward branches occur (_both_branches)."""
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.stateset import StateSet

    net = _net(name)
    rng = np.random.default_rng(B + base)
    acts = _actions(rng, B, net.n_nodes)
    b = PBNBatch(net, B, env_id_base=base, seed=SEED)
    b.randomize()
    s0 = b.get_state()
    b.close()
    rec = _records(net, B, base, SEED, s0, U0, acts, T_MAX)
    pool = np.unique(rec.reshape(-1, net.n_words), axis=0)
    keep = rng.random(len(pool)) < 0.5
    # whatever the draw: env 0's first state is a member, the last env's last state is not
    assert not np.array_equal(rec[0][0], rec[-1][-1])
    keep[(pool == rec[0][0]).all(axis=1)] = True
    keep[(pool == rec[-1][-1]).all(axis=1)] = False
    members = pool[keep]
    target = StateSet(members, net.n_nodes, labels=np.arange(len(members)) % 5, device=0)
    labels = np.stack([target.lookup(r) for r in rec])
    for a in (s0, rec, labels, acts):
        a.setflags(write=False)
    return net, s0, acts, rec, labels, target, rng.integers(0, 1 << 31)


def _both_branches(labels, rounds):
    ran = np.arange(labels.shape[0])[:, None] < np.asarray(rounds)[None, :]
    return bool((labels[ran] >= 0).any() and (labels[ran] < 0).any())


def _fresh(net, B, base, s0):
    from gym_pbn_amd.batch import PBNBatch

    f = PBNBatch(net, B, env_id_base=base, seed=SEED)
    f.set_state(s0)
    f.seek(update_count=U0)
    return f


def _then_one_plain_step(f, net, B, base, want_state):
    """The macro step left the counters where a twin seeked there continues identically."""
    f.step(1)
    twin = _fresh(net, B, base, want_state)
    twin.seek(update_count=U0 + T_MAX)
    twin.step(1)
    assert np.array_equal(f.get_state(), twin.get_state())
    assert f.counters()["update_count"] == U0 + T_MAX + 1
    twin.close()


@pytest.mark.parametrize("name,B,base", SHAPE_CASES)
def test_interval_mode_equals_rounds_of_flip_step_lookup(name, B, base):
    """B = 257: two workgroups and a ragged tail. env_id_base 1 with B = 2: envs 1 and 2 take their step words
    from two different Philox calls."""
    net, s0, acts, rec, labels, target, sub = _case(name, B, base)
    lims = np.random.default_rng(sub).integers(1, T_MAX + 1, size=B).astype(np.int32)
    lims[:2] = [1, T_MAX]
    assert (lims == 1).any() and (lims == T_MAX).any()
    lims[-1] = T_MAX
    assert _both_branches(labels, lims)
    want = _expect(rec, labels, acts, lims, INTERVAL, None)
    f = _fresh(net, B, base, s0)
    got = _Out(B, net.n_words).step(f, target, INTERVAL, T_MAX, acts, lims)
    _assert_equal(got, want, f.get_state())
    assert got["reward"].dtype == np.int32
    assert f.counters()["update_count"] == U0 + T_MAX  # t_max, whatever the intervals were
    _then_one_plain_step(f, net, B, base, want["state"])
    f.close()


@pytest.mark.parametrize("name,B,base", SHAPE_CASES)
def test_trigger_mode_equals_rounds_until_the_documented_draw(name, B, base):
    net, s0, acts, rec, labels, target, sub = _case(name, B, base)
    gpow, thr = _tables(T_MAX)
    probs = np.random.default_rng(sub + 1).integers(1, 11, size=B).astype(np.int32)
    probs[0], probs[-1] = 10, 1  # p = 10 always stops after round 0; p = 1 seldom stops
    rounds, by_draw = _stop_rounds(SEED, base, U0, probs, T_MAX, thr)
    assert rounds[0] == 1 and by_draw[0]
    assert (by_draw & (rounds < T_MAX)).any(), "no env stops by its draw"
    assert (~by_draw & (rounds == T_MAX)).any(), "no env runs into t_max"
    assert _both_branches(labels, rounds)
    want = _expect(rec, labels, acts, rounds, TRIGGER, gpow)
    f = _fresh(net, B, base, s0)
    got = _Out(B, net.n_words).step(f, target, TRIGGER, T_MAX, acts, probs)
    _assert_equal(got, want, f.get_state())
    assert got["reward"].dtype == np.float64
    assert f.counters()["update_count"] == U0 + T_MAX
    _then_one_plain_step(f, net, B, base, want["state"])
    f.close()


@pytest.mark.parametrize("mode", [INTERVAL, TRIGGER])
@pytest.mark.parametrize("name", ["tt6", "tt200"])
def test_an_invalid_env_is_skipped_whole_and_reported_once(name, mode):
    from gym_pbn_amd.stateset import StateSet

    net = _net(name)
    N, W, B, base = net.n_nodes, net.n_words, 70, 0
    rng = np.random.default_rng(3 + mode)
    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch(net, B, seed=SEED)
    b.randomize()
    s0 = b.get_state()
    b.close()
    gpow, thr = _tables(T_MAX)
    lim_max = T_MAX if mode == INTERVAL else 10
    acts = _actions(rng, B, N)
    lims = rng.integers(1, lim_max + 1, size=B).astype(np.int32)
    acts[3], acts[66], lims[5], lims[64] = N + 1, -1, 0, lim_max + 1
    bad = np.zeros(B, bool)
    bad[[3, 66, 5, 64]] = True
    ok_acts = np.where(bad, 0, acts).astype(np.int32)
    rec = _records(net, B, base, SEED, s0, U0, ok_acts, T_MAX)
    target = StateSet(np.unique(np.concatenate([s0, rec[0]]), axis=0), N, device=0)  # skipped rows would terminate
    labels = np.stack([target.lookup(r) for r in rec])
    ok_lims = np.where(bad, 1, lims)
    rounds = ok_lims if mode == INTERVAL else _stop_rounds(SEED, base, U0, ok_lims, T_MAX, thr)[0]
    want = _expect(rec, labels, ok_acts, rounds, mode, gpow)
    f = _fresh(net, B, base, s0)
    out = _Out(B, W)
    got = out.step(f, target, mode, T_MAX, acts, lims, check=False)  # asynchronous: no report yet
    state = f.get_state()
    assert np.array_equal(state[bad], s0[bad])
    _assert_equal(got, want, state, rows=~bad)
    assert (got["obs"][bad].view(np.int64) == SENTINEL).all() and (got["reward"][bad] == SENTINEL).all()
    assert (got["flags"][bad] == 99).all()
    for k in ("label", "interval", "first_hit"):
        assert (got[k][bad] == SENTINEL).all(), k
    assert f.counters()["update_count"] == U0 + T_MAX  # the launch happened
    zeros, ones = np.zeros(B, np.int32), np.ones(B, np.int32)
    with pytest.raises(ValueError, match="Invalid action"):
        out.step(f, target, mode, T_MAX, zeros, ones, check=True)  # the sticky flag, raised once ...
    assert f.counters()["update_count"] == U0 + 2 * T_MAX
    out.step(f, target, mode, T_MAX, zeros, ones, check=True)  # ... and cleared
    f.close()
    target.close()


@pytest.mark.parametrize("mode", [INTERVAL, TRIGGER])
@pytest.mark.parametrize("name", ["tt6", 65])
def test_one_workgroup_walks_every_env(name, mode, monkeypatch):
    """B = 600 with the grid capped at one workgroup (PBNSIM_ENVSET_GRID=1): every lane takes two or three envs in
    the grid-stride loop, and on the third trip only 88 lanes are live -- one full wave, one partly live, two that
    have left. The limits are ragged, so the lanes of a wave stop at different rounds on every trip. tt6: W = 1;
    ttk3_65: W = 2. Env 515 (third trip) holds an invalid limit: skipped whole and reported."""
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.stateset import StateSet

    net = _net(name)
    N, W, B, base, bad_env = net.n_nodes, net.n_words, 600, 2, 515
    rng = np.random.default_rng(N + mode)
    monkeypatch.setenv("PBNSIM_ENVSET_GRID", "1")
    b = PBNBatch(net, B, env_id_base=base, seed=SEED)
    b.randomize()
    s0 = b.get_state()
    b.close()
    gpow, thr = _tables(T_MAX)
    lim_max = T_MAX if mode == INTERVAL else 10
    acts = _actions(rng, B, N)
    acts[-1] = N  # node N - 1 on the last live lane of the third trip
    lims = rng.integers(1, lim_max + 1, size=B).astype(np.int32)
    lims[bad_env] = 0
    bad = np.arange(B) == bad_env
    ok_acts = np.where(bad, 0, acts).astype(np.int32)
    ok_lims = np.where(bad, 1, lims)
    rec = _records(net, B, base, SEED, s0, U0, ok_acts, T_MAX)
    pool = np.unique(rec.reshape(-1, W), axis=0)
    target = StateSet(pool[rng.random(len(pool)) < 0.5], N, device=0)
    labels = np.stack([target.lookup(r) for r in rec])
    rounds = ok_lims if mode == INTERVAL else _stop_rounds(SEED, base, U0, ok_lims, T_MAX, thr)[0]
    for trip in (slice(0, 256), slice(256, 512), slice(512, 600)):
        assert len(set(rounds[trip][:64].tolist())) > 1, "the first wave of a trip is not ragged"
        assert _both_branches(labels[:, trip], rounds[trip])
    want = _expect(rec, labels, ok_acts, rounds, mode, gpow)
    f = _fresh(net, B, base, s0)
    out = _Out(B, W)
    got = out.step(f, target, mode, T_MAX, acts, lims)
    state = f.get_state()
    assert np.array_equal(state[bad], s0[bad])
    _assert_equal(got, want, state, rows=~bad)
    assert (got["obs"][bad].view(np.int64) == SENTINEL).all() and (got["reward"][bad] == SENTINEL).all()
    assert (got["flags"][bad] == 99).all() and (got["interval"][bad] == SENTINEL).all()
    assert f.counters()["update_count"] == U0 + T_MAX
    with pytest.raises(ValueError, match="Invalid action"):
        out.step(f, target, mode, T_MAX, np.zeros(B, np.int32), np.ones(B, np.int32), check=True)
    f.close()
    target.close()


@pytest.mark.parametrize("N", SHAPES)
def test_every_state_width(N):
    """One interval-mode call per words-per-env instantiation, with flips on both sides of the word boundaries and
    on node N - 1."""
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.stateset import StateSet

    net = _net(N)
    B, base, t_max, W = 130, 0, 3, net.n_words
    rng = np.random.default_rng(N)
    acts = rng.integers(0, N + 1, size=B).astype(np.int32)
    edges = [n for n in edge_nodes(N) if n in (63, 64, N - 1)]
    assert N - 1 in edges and (N <= 64 or {63, 64} <= set(edges))
    acts[:len(edges)] = np.array(edges) + 1
    lims = rng.integers(1, t_max + 1, size=B).astype(np.int32)
    lims[:len(edges)] = [1, 3, 2][:len(edges)]
    b = PBNBatch(net, B, seed=SEED)
    b.randomize()
    s0 = b.get_state()
    b.close()
    rec = _records(net, B, base, SEED, s0, U0, acts, t_max)
    pool = np.unique(rec.reshape(-1, W), axis=0)
    target = StateSet(pool[rng.random(len(pool)) < 0.5], N, device=0)
    labels = np.stack([target.lookup(r) for r in rec])
    assert _both_branches(labels, lims)
    want = _expect(rec, labels, acts, lims, INTERVAL, None)
    f = _fresh(net, B, base, s0)
    got = _Out(B, W).step(f, target, INTERVAL, t_max, acts, lims)
    _assert_equal(got, want, f.get_state())
    assert f.counters()["update_count"] == U0 + t_max
    f.close()
    target.close()


def test_refusals_launch_nothing():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.stateset import StateSet

    net = _net("tt6")
    b = PBNBatch(net, 8, seed=1)
    b.randomize()
    s0 = b.get_state()
    out = _Out(8, 1)
    target = StateSet(np.array([[1]], np.uint64), 6, device=0)
    a = _dev(np.zeros(8, np.int32))
    lim = _dev(np.ones(8, np.int32))
    gpow, thr = (_dev(t) for t in _tables(T_MAX))
    import torch

    torch.cuda.synchronize()

    def call(batch=b, tgt=target, mode=INTERVAL, t_max=T_MAX, **kw):
        kw.setdefault("d_reward_i32", out.reward_i32.data_ptr())
        batch.tenv_macro_device(tgt, mode, t_max, a.data_ptr(), lim.data_ptr(), out.flags.data_ptr(), **kw)

    for t_max in (0, _lib.TENV_MACRO_MAX_T + 1):
        with pytest.raises(ValueError, match="t_max"):
            call(t_max=t_max)
    with pytest.raises(ValueError, match="mode"):
        call(mode=2)
    with pytest.raises(ValueError, match="d_reward_i32"):
        call(d_reward_i32=0)
    for missing in ("d_reward_f64", "d_gpow", "d_stop_thr"):
        kw = dict(d_reward_f64=out.reward_f64.data_ptr(), d_gpow=gpow.data_ptr(), d_stop_thr=thr.data_ptr())
        kw[missing] = 0
        with pytest.raises(ValueError, match=missing):
            call(mode=TRIGGER, **kw)
    with pytest.raises(ValueError, match="7 nodes"):
        call(tgt=StateSet(np.array([[1]], np.uint64), 7, device=0))
    mix = PBNBatch("bittner28", 8, seed=1)
    with pytest.raises(_lib.PbnError) as ei:
        call(batch=mix, tgt=StateSet(np.array([[1]], np.uint64), 28, device=0))
    assert ei.value.code == _lib.PBN_E_UNSUPPORTED
    b.sync()
    assert np.array_equal(b.get_state(), s0) and (out.reward_i32.cpu().numpy() == SENTINEL).all()
    assert b.counters()["update_count"] == 0
    b.close()
    mix.close()


# ---------------------------------------------------------------------------------------------- env classes
def _env_target():
    case = next(c for c in KAT["cases"] if c["network"] == "tt6" and c["kind"] == "PBNEnv")
    return {tuple(t) for t in case["target"]}


def _reset_picks(seed, base, reset_count, B, n):
    """mulhi(word 0 of the stream-9 call {0, reset_count, global env id}, n): pbn_tenv_reset_device's row."""
    picks = []
    for e in range(B):
        w = bitmodel.draw(seed, 0, reset_count, base + e, 9)
        picks.append((w[0] * n) >> 32)
    return np.array(picks)


@pytest.mark.parametrize("cls_name,mode", [("TorchVecPBNSampledDataEnv", INTERVAL),
                                           ("TorchVecPBNSelfTriggeringEnv", TRIGGER)])
def test_env_classes_equal_the_twin_and_auto_reset(cls_name, mode):
    import torch

    import gym_pbn_amd
    from gym_pbn_amd.macro_env import decode_discrete

    cls = getattr(gym_pbn_amd, cls_name)
    B, seed, T = 257, 3, T_MAX
    kw = dict(goal_config={"target_nodes": _env_target()}, n_envs=B, seed=seed, T=T, gamma=GAMMA)
    env = cls(_tt6_source(), **kw)
    net, N, W = env.net, env.N, env.W
    n_lim = T if mode == INTERVAL else 10
    assert env.T == T and env.primitive_action_space.n == N + 1 and env.discrete_action_space.n == (N + 1) * n_lim
    assert env.action_space.contains((N, n_lim)) and not env.action_space.contains((N + 1, 1))
    assert env.observation_space.shape == (N,)
    gpow, thr = _tables(T)
    env.batch.randomize()
    rng = np.random.default_rng(mode)
    terms = 0
    for t in range(3):
        prev = env.observation_words().cpu().numpy().view(np.uint64).copy()
        u0 = env.batch.counters()["update_count"]
        assert u0 == t * T
        if t % 2 == 0:  # discrete indices
            idx = rng.integers(0, (N + 1) * n_lim, size=B)
            acts, lims = (np.asarray(v, np.int32) for v in decode_discrete(idx, N + 1))
            obs, reward, term, trunc, info = env.step(torch.from_numpy(idx).to("cuda:0"))
        else:  # (action, limit) tensors
            acts = rng.integers(0, N + 1, size=B).astype(np.int32)
            lims = rng.integers(1, n_lim + 1, size=B).astype(np.int32)
            obs, reward, term, trunc, info = env.step(torch.from_numpy(acts).to("cuda:0"),
                                                      torch.from_numpy(lims).to("cuda:0"), check=True)
        rec = _records(net, B, 0, seed, prev, u0, acts, T)
        labels = np.stack([env.target.lookup(r) for r in rec])
        rounds = lims if mode == INTERVAL else _stop_rounds(seed, 0, u0, lims, T, thr)[0]
        want = _expect(rec, labels, acts, rounds, mode, gpow)
        assert obs.dtype == torch.uint8 and obs.shape == (B, N)
        assert reward.dtype == (torch.int32 if mode == INTERVAL else torch.float64) and reward.shape == (B,)
        assert term.dtype == torch.bool and trunc.dtype == torch.bool and not trunc.any().item()
        assert info["obs_words"].dtype == torch.int64 and info["obs_words"].shape == (B, W)
        for k in ("label", "interval", "first_hit"):
            assert info[k].dtype == torch.int32 and info[k].shape == (B,)
        got = dict(obs=info["obs_words"].cpu().numpy().view(np.uint64), reward=reward.cpu().numpy(),
                   flags=term.cpu().numpy().astype(np.uint8), label=info["label"].cpu().numpy(),
                   interval=info["interval"].cpu().numpy(), first_hit=info["first_hit"].cpu().numpy())
        _assert_equal(got, want, env.observation_words().cpu().numpy().view(np.uint64))
        bits = (want["state"][:, 0:1] >> np.arange(N, dtype=np.uint64)) & np.uint64(1)
        assert np.array_equal(obs.cpu().numpy(), bits.astype(np.uint8))
        terms += int(want["flags"].sum())
    assert 0 < terms < 3 * B
    with pytest.raises(ValueError, match="Invalid action"):
        env.step(torch.full((B,), (N + 1) * n_lim, dtype=torch.int64, device="cuda:0"), check=True)
    env.close()
    if mode == INTERVAL:
        with pytest.raises(ValueError, match="65536"):
            cls(_tt6_source(), goal_config={"target_nodes": _env_target()}, n_envs=B)

    # auto-reset: exactly the envs whose last round ended in the target hold the state the documented draw names
    env = cls(_tt6_source(), auto_reset=True, **kw)
    attracting = env._attracting.cpu().numpy().view(np.uint64)
    env.batch.randomize()
    ended = 0
    for t in range(3):
        rc = env.batch.counters()["reset_count"]
        idx = rng.integers(0, (N + 1) * n_lim, size=B)
        _, _, term, _, info = env.step(torch.from_numpy(idx).to("cuda:0"))
        term = term.cpu().numpy()
        after = env.observation_words().cpu().numpy().view(np.uint64)
        picks = _reset_picks(seed, 0, rc, B, len(attracting))
        final = info["obs_words"].cpu().numpy().view(np.uint64)
        assert np.array_equal(after, np.where(term[:, None], attracting[picks] & ~np.uint64(1), final)), t
        assert env.batch.counters()["reset_count"] == rc + 1
        ended += int(term.sum())
    assert 0 < ended < 3 * B
    env.close()
