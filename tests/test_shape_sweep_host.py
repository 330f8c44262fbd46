"""The oracle against the unpacked model (``bitmodel.py``) on every network of the shape table (CPU only).

``oracle/pbn_oracle.c`` is pinned to the reference by goldens at some widths (``test_oracle.py``); a
kernel-vs-oracle match elsewhere would only show that two word-packed implementations agree. Here the oracle's
four operations that every GPU test leans on are compared, bit for bit, with a model that has no words, masks
or shifts by node index, at every ``W = 1 .. 8``, every ``N % 64 == 0`` and both sides of 64 and 256. Each
trajectory also has to move node ``N - 1`` and the nodes next to every word boundary (asserted on the
oracle's result), so a comparison cannot pass on states that never touch an edge.
"""

import numpy as np
import pytest

from bitmodel import BitModel
from shape_cases import (KINDS, SHAPES, assert_edges_move, edge_actions, edge_attractors, edge_nodes, n_words,
                         shape_net)

B = 64
CASES = [(k, n) for k in KINDS for n in SHAPES]


@pytest.fixture(scope="module")
def both(oracle_mod):
    cache = {}

    def get(kind, N):
        if (kind, N) not in cache:
            net = shape_net(kind, N)
            cache[kind, N] = (oracle_mod.Oracle(net), BitModel(net))
        return cache[kind, N]

    return get


def _pack(oracle_mod, bits):
    return oracle_mod.pack_bits(np.array(bits, dtype=np.uint8))


def test_shape_table_reaches_every_width():
    assert sorted({n_words(n) for n in SHAPES}) == list(range(1, 9))
    assert [n for n in range(64, 513, 64)] == [n for n in SHAPES if n % 64 == 0]
    assert {63, 65, 256, 257} <= set(SHAPES) and max(SHAPES) == 512


@pytest.mark.parametrize("kind,N", CASES)
@pytest.mark.parametrize("base", [5, 4])
def test_init_and_step_match_the_unpacked_model(oracle_mod, both, kind, N, base):
    """``init_philox`` (reset counter 0 and 3), 48 Philox updates from update 7 and 16 forced updates, odd and
    even env base (the lane-pair draw sharing: env g takes words 2(g & 1), 2(g & 1) + 1 of call g >> 1)."""
    o, m = both(kind, N)
    seed, T = 17, 48
    init = o.init_philox(B, seed=seed, env_base=base)
    bits = m.init_philox(B, seed, base)
    assert np.array_equal(init, _pack(oracle_mod, bits))
    assert np.array_equal(o.init_philox(9, seed=2**40 + 3, env_base=base, reset_count=3),
                          _pack(oracle_mod, m.init_philox(9, 2**40 + 3, base, 3)))
    if N % 64 == 0:  # the unmasked top bit is a fair bit: both values occur
        top = (init[:, -1] >> np.uint64(63)) & np.uint64(1)
        assert 0 < int(top.sum()) < B
    last = o.step_philox(init, seed, base, 7, T)
    assert np.array_equal(last, _pack(oracle_mod, m.step_philox(bits, seed, base, 7, T)))
    rng = np.random.default_rng(N)
    ni = rng.integers(1 if kind == "tt" else 0, N, size=(16, B)).astype(np.uint32)
    edges = edge_nodes(N)
    for t in range(12):  # every edge node is forced in many envs: the compared states touch every edge
        ni[t] = [edges[(e + t) % len(edges)] for e in range(B)]
    forced = o.step_forced(init, ni, seed, base, 2**32 - 2)  # the update counter crosses 2^32
    assert_edges_move(init, forced, N, kind)
    assert np.array_equal(forced, _pack(oracle_mod, m.step_forced(bits, ni.tolist(), seed, base, 2**32 - 2)))


@pytest.mark.parametrize("kind,N", CASES)
def test_oracle_trajectories_reach_every_edge(oracle_mod, both, kind, N):
    """The coverage condition the sweeps rely on, for free-running trajectories (B = 512, 48 updates, seed 17,
    base 5): node ``N - 1`` and both sides of every word boundary change in some env."""
    o, _ = both(kind, N)
    init = o.init_philox(512, seed=17, env_base=5)
    assert_edges_move(init, o.step_philox(init, 17, 5, 0, 48), N, kind)


@pytest.mark.parametrize("kind,N", CASES)
@pytest.mark.parametrize("first", [False, True])
def test_env_reset_and_step_match_the_unpacked_model(oracle_mod, both, kind, N, first):
    """``env_reset_philox`` (masked: the other envs keep state and ``n_steps``) and three ``env_step_multi``
    calls: cubes caring about node ``N - 1`` and both sides of a word boundary, actions on nodes 0, 63, 64 and
    ``N - 1`` with duplicates, dedup on and off, offsets 1 and 0, a cap of 100 that some envs hit and others do
    not, horizon 2 (truncation at the second call)."""
    from gym_pbn_amd.batch import cube_arrays

    o, m = both(kind, N)
    rng = np.random.default_rng(1000 + N)
    attractors = edge_attractors(rng, N)
    care, val = cube_arrays([c for a in attractors for c in a], N)
    rc, rv = cube_arrays(attractors[0], N)
    tc, tv = cube_arrays([attractors[-1][0]], N)
    cfg = dict(care=care, value=val, target_care=tc[0], target_value=tv[0], horizon=2, first_tested=first)
    seed, base = 2**33 + 9, 6
    st0 = o.init_philox(B, seed=1, env_base=base)
    bits0 = m.init_philox(B, 1, base)
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    st, ns = o.env_reset_philox(st0, np.full(B, 5, np.int64), rc, rv, mask=mask, seed=seed, env_base=base,
                                reset_count=2)
    bits, mns = m.env_reset_philox(bits0, [5] * B, attractors[0], mask.tolist(), seed, base, 2)
    assert np.array_equal(st, _pack(oracle_mod, bits)) and ns.tolist() == mns
    assert np.array_equal(st[mask == 0], st0[mask == 0]) and (st[mask == 1] != st0[mask == 1]).any()
    ns[:] = 0
    mns = [0] * B
    seen, reset_state = set(), st
    for call, (dedup, offset) in enumerate([(True, 1), (False, 1), (True, 0)]):
        acts = edge_actions(rng, B, 3, N, offset)
        if offset == 1:
            acts[5, 2] = -N + 1  # Python list indexing: node 0 from the end
        r = o.env_step_multi(cfg, st, ns, acts, dedup=dedup, offset=offset, seed=seed, env_base=base,
                             call_idx=call, update_cap=100, n_threads=1)
        q = m.env_step_multi(attractors, 2, bits, mns, acts.tolist(), dedup, offset, seed, base, call, 100, first)
        assert np.array_equal(r["state"], _pack(oracle_mod, q["state"])), call
        assert np.array_equal(r["obs"], _pack(oracle_mod, q["obs"])), call
        for k in ("reward", "flags", "n_updates", "n_steps"):
            assert r[k].tolist() == q[k], (call, k)
        seen |= set(r["flags"].tolist())
        st, ns, bits, mns = r["state"], r["n_steps"], q["state"], q["n_steps"]
    assert any(f & 4 for f in seen) and any(not f & 4 for f in seen) and any(f & 2 for f in seen)
    assert_edges_move(reset_state, st, N, kind)
    with pytest.raises(ValueError):
        m.env_step_multi(attractors, 2, bits, mns, [[N + 1, 0, 0]] * B)
    with pytest.raises(ValueError):
        o.env_step_multi(cfg, st, ns, np.array([[N + 1, 0, 0]] * B, np.int32))
