"""The state census on the device (``pbn_census_*``, ``csrc/pbn_census.hip``) against a twin batch.

The expectation of every exact test is a twin: a second batch of the same network, seed, ``env_id_base`` and start
state that loops ``step(1)`` + ``get_state()`` on the host; the states at the sample points go through ``np.unique``.
Nothing expected comes from the census. The update counter starts just below 2^32, so the 33 updates of a run cross
the boundary between the Philox counter's two words.
"""

import functools

import numpy as np
import pytest

from shape_cases import pm_net, tt_net

pytestmark = pytest.mark.gpu

B = 300  # one full workgroup and a ragged one
T = 33  # odd: for predictor mix the last update uses half of a Philox call
BASE = 5  # odd: envs 2m / 2m + 1 of a Philox call sit in lanes 2k + 1 / 2k + 2
U0 = (1 << 32) - 7
SAMPLING = [(0, 1), (3, 4), (33, 1)]

NETS = {
    "tt8": lambda: "tt8",
    "bittner28": lambda: "bittner28",
    "pm65": lambda: pm_net(65),
    "tt65": lambda: tt_net(65),
    "pm257": lambda: pm_net(257),
    "tt257": lambda: tt_net(257),
    "pm512": lambda: pm_net(512),
    "tt512": lambda: tt_net(512),
}


def _batch(net, n_envs, seed, start=None, update_count=U0):
    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch(net, n_envs, seed=seed, env_id_base=BASE)
    if start is None:
        b.randomize()
    else:
        b.set_state(start)
    b.seek(update_count=update_count)
    return b


def _walk(b, n_updates):
    """The twin's trajectory [n_updates + 1][B][W]: the state after i updates, step by step through the host."""
    out = [b.get_state()]
    for _ in range(n_updates):
        b.step(1)
        out.append(b.get_state())
    return np.stack(out)


def _expected(traj, first, stride, mask=None):
    """{state words: visits} of the trajectory's sample points, and the number of sample points per env."""
    idx = list(range(first, traj.shape[0], stride))
    rows = traj[idx].reshape(-1, traj.shape[2])
    if mask is not None:
        rows = rows & np.asarray(mask, dtype=np.uint64)
    uniq, cnt = np.unique(rows, axis=0, return_counts=True)
    return {tuple(int(v) for v in r): int(c) for r, c in zip(uniq, cnt)}, len(idx)


def _got(result):
    d = {tuple(int(v) for v in r): int(c) for r, c in zip(result.states, result.counts)}
    assert len(d) == len(result)  # every state is held once
    return d


@functools.lru_cache(maxsize=None)
def _twin(name):
    """Per network, once: the start state, the twin's trajectory over T updates, its counters there, and its state
    after five more."""
    net = NETS[name]()
    t = _batch(net, B, seed=11)
    start = t.get_state()
    traj = _walk(t, T)
    counters = t.counters()
    t.step(5)
    after = t.get_state()
    t.close()
    for a in (start, traj, after):
        a.setflags(write=False)
    return start, traj, counters, after


@pytest.mark.parametrize("first,stride", SAMPLING)
@pytest.mark.parametrize("name", list(NETS))
def test_exact_counts_every_kind_and_word_edge(name, first, stride):
    from gym_pbn_amd.census import StateCensus

    start, traj, counters, after = _twin(name)
    want, samples = _expected(traj, first, stride)
    b = _batch(NETS[name](), B, seed=11)  # randomized as the twin was: the same counters, the same state
    assert np.array_equal(b.get_state(), start)
    c = StateCensus(b.net, max_states=1 << 15)
    c.run(b, T, first=first, stride=stride)
    r = c.result()
    assert _got(r) == want
    info = c.info()
    assert info["dropped"] == 0 and r.dropped == 0
    assert info["visits"] == B * samples == r.visits == sum(want.values())
    assert info["n_states"] == len(want)
    assert np.array_equal(b.get_state(), traj[T])
    assert b.counters() == counters and counters["update_count"] == U0 + T
    b.step(5)
    assert np.array_equal(b.get_state(), after)
    assert 0 < c.adds() <= info["visits"]
    c.close()
    b.close()


def test_one_workgroup_walks_the_whole_batch(monkeypatch):
    """PBNSIM_ENVSET_GRID=1: the grid-stride loop, a lane taking a second env with its run flushed in between."""
    from gym_pbn_amd.census import StateCensus

    start, traj, _, _ = _twin("bittner28")
    want, _ = _expected(traj, 0, 1)
    monkeypatch.setenv("PBNSIM_ENVSET_GRID", "1")
    b = _batch("bittner28", B, seed=11, start=start)
    c = StateCensus(b.net, max_states=1 << 15)
    c.run(b, T)
    assert _got(c.result()) == want and c.info()["dropped"] == 0
    assert np.array_equal(b.get_state(), traj[T])
    c.close()
    b.close()


def test_same_key_insert_race_across_workgroups():
    """4,096 envs in one state: 16 workgroups insert the same new key at once, then at most 128 keys take every add."""
    from gym_pbn_amd.census import StateCensus

    n_envs, n_updates = 4096, 16
    start = np.full((n_envs, 1), 0b10110100, dtype=np.uint64)  # node 0 clear, as PBN.reset leaves it
    t = _batch("tt8", n_envs, seed=3, start=start)
    want, samples = _expected(_walk(t, n_updates), 0, 1)
    assert 1 < len(want) <= 128 and want[(0b10110100,)] >= n_envs
    b = _batch("tt8", n_envs, seed=3, start=start)
    c = StateCensus(b.net, max_states=1 << 10)
    c.run(b, n_updates)
    r = c.result()
    assert _got(r) == want
    assert (r.dropped, r.visits) == (0, n_envs * samples)
    assert np.array_equal(b.get_state(), t.get_state())
    # a loser keeps the entry it took in vain through every later hit on a state already held, and inserts with it:
    # the key array gives out the states held plus at most one entry per lane (4,096 lanes here), not one per lost race
    assert len(want) < c.entries() <= len(want) + n_envs
    # a second launch inserts with what the first one's lanes left on the ring
    want2, samples2 = _expected(_walk(t, n_updates), 1, 1)
    for s, n in want2.items():
        want[s] = want.get(s, 0) + n
    c.run(b, n_updates, first=1)
    r = c.result()
    assert _got(r) == want and (r.dropped, r.visits) == (0, n_envs * (samples + samples2))
    assert c.entries() <= len(want) + n_envs
    for x in (c, b, t):
        x.close()


def test_half_a_million_lanes_race_for_one_state_and_drop_nothing():
    """2^20 envs in one state: every resident lane (up to 2^19, as many as the key array has entries past max_states)
    takes an entry for the same new key at the first sample point and all but one lose. The spares have to last: with
    128 reachable states and max_states = 256 nothing may be dropped. No twin at this size: the invariants alone."""
    from gym_pbn_amd.census import StateCensus

    n_envs, n_updates = 1 << 20, 8
    b = _batch("tt8", n_envs, seed=5, start=np.full((n_envs, 1), 0b10110100, dtype=np.uint64))
    c = StateCensus(b.net, max_states=256)
    c.run(b, n_updates)
    r = c.result()
    info = c.info()
    assert info["dropped"] == 0 and r.dropped == 0
    assert 1 < info["n_states"] == len(r) <= 128  # node 0 stays clear: 2^7 states
    assert int(r.counts.sum()) == info["visits"] == n_envs * (n_updates + 1)
    assert _got(r)[(0b10110100,)] >= n_envs  # every env was counted there once, before its first update
    assert np.isin(np.unique(b.get_state()), r.states).all()  # the last sample point is the state the batch is left in
    assert c.entries() <= info["n_states"] + (1 << 19)
    c.close()
    b.close()


def test_overflow_is_counted_never_silent():
    from gym_pbn_amd.census import StateCensus

    # 300 uniform draws over the 128 states with node 0 clear: about 116 distinct at the first sample point alone
    start, traj, _, _ = _twin("tt8")
    want, samples = _expected(traj, 0, 1)
    assert len(want) >= 32
    b = _batch("tt8", B, seed=11, start=start)
    c = StateCensus(b.net, max_states=16)
    c.run(b, T)
    r = c.result()
    got = _got(r)
    info = c.info()
    assert info["n_states"] == len(got) <= 16  # (a)
    assert info["visits"] == B * samples
    assert sum(got.values()) + info["dropped"] == info["visits"]  # (b)
    assert info["dropped"] > 0 and not r.exact
    for s, n in got.items():  # (d)
        assert s in want and 0 < n <= want[s], s
    assert np.array_equal(b.get_state(), traj[T])  # the walk does not depend on the table
    c.close()
    b.close()


def test_accumulate_and_clear():
    from gym_pbn_amd.census import StateCensus

    start, traj, _, _ = _twin("bittner28")
    b = _batch("bittner28", B, seed=11, start=start)
    c = StateCensus(b.net, max_states=1 << 15)
    c.run(b, 10)
    c.run(b, 7, first=1)  # the state after update 10 was the first call's last sample
    want, samples = _expected(traj[:18], 0, 1)
    assert _got(c.result()) == want
    assert c.info()["visits"] == B * samples and c.info()["dropped"] == 0
    c.clear()
    info = c.info()
    assert (info["n_states"], info["visits"], info["dropped"]) == (0, 0, 0) and len(c.result()) == 0 and c.adds() == 0
    c.run(b, 16)  # updates 17 .. 33 of the twin
    want, samples = _expected(traj[17:34], 0, 1)
    assert _got(c.result()) == want and c.info()["visits"] == B * samples
    assert np.array_equal(b.get_state(), traj[33])
    # no update: the current state is counted, nothing moves
    before = b.counters()
    c.clear()
    c.run(b, 0)
    want, _ = _expected(traj[33:34], 0, 1)
    assert _got(c.result()) == want and b.counters() == before
    c.close()
    b.close()


def test_projection_across_the_word_boundary():
    from gym_pbn_amd.census import StateCensus

    start, traj, _, _ = _twin("pm65")
    nodes = [5, 63, 64]
    mask = np.array([(1 << 5) | (1 << 63), 1], dtype=np.uint64)
    want, samples = _expected(traj, 0, 1, mask=mask)
    assert 2 <= len(want) <= 8
    b = _batch(pm_net(65), B, seed=11, start=start)
    c = StateCensus(b.net, max_states=64)
    assert np.array_equal(c.node_mask(nodes), mask)
    c.run(b, T, nodes=nodes)
    r = c.result()
    assert _got(r) == want and (r.dropped, r.visits) == (0, B * samples)
    assert np.array_equal(b.get_state(), traj[T])  # the state itself is not projected
    c.close()
    b.close()


def test_refusals_that_need_a_batch():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.census import StateCensus

    b = _batch("bittner28", 8, seed=1)
    before = b.counters()
    other = StateCensus(8)
    with pytest.raises(ValueError, match="28"):
        other.run(b, 4)
    c = StateCensus(b.net, max_states=64)
    with pytest.raises(ValueError, match="n_updates"):
        c.run(b, _lib.CENSUS_MAX_UPDATES + 1)
    with pytest.raises(ValueError, match="first"):
        c.run(b, 4, first=5)
    assert b.counters() == before and c.info()["visits"] == 0 and other.info()["visits"] == 0
    for x in (c, other, b):
        x.close()


def test_surface_statistical_attractors_state_set_and_occupancy():
    from gym_pbn_amd.attractors import find_attractors
    from gym_pbn_amd.batch import PBNBatch, unpack_bits
    from gym_pbn_amd.census import StateCensus, statistical_attractors

    resets, steps = 64, 50
    t = PBNBatch("tt8", resets, seed=0)
    t.randomize()
    traj = _walk(t, steps - 1)  # the state before each of the 50 steps
    t.close()
    want, _ = _expected(traj, 0, 1)
    # the documented tie rule: count descending, then the state as an integer ascending
    ranked = sorted(want, key=lambda s: (-want[s], s[::-1]))
    top4 = [tuple(int(v) for v in unpack_bits(np.array(s, dtype=np.uint64), 8)) for s in ranked[:4]]
    assert statistical_attractors("tt8", k=4, resets=resets, steps=steps) == top4

    b = PBNBatch("tt8", resets, seed=0)
    b.randomize()
    c = StateCensus("tt8")
    c.run(b, steps - 1)
    r = c.result()
    assert [tuple(int(v) for v in s) for s in r.states] == ranked
    s = r.state_set(k=4)
    assert s.lookup(np.array(ranked[:4], dtype=np.uint64)).tolist() == [0, 1, 2, 3]
    if len(ranked) > 4:
        assert s.lookup(np.array(ranked[4:5], dtype=np.uint64)).tolist() == [-1]
    assert b.classify_host(s).shape == (resets,)
    att = find_attractors("tt8", n_seeds=256, table_graph="step")
    per, outside = att.occupancy(r)
    assert len(per) == len(att.attractors) and int(per.sum()) + outside == r.visits == resets * steps
    assert np.isclose(r.frequencies().sum(), 1.0)
    for x in (s, c, b):
        x.close()
