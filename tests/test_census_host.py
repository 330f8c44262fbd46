"""The state census (``pbn_census_*``, ``csrc/pbn_census.hpp``) without a GPU: the refusals of the C entry points
through ctypes on a host-only handle (``device=-1``), ``CensusResult``'s ordering and helpers from hand-made arrays,
and the header's host part under ASan + UBSan (``make censuscheck``).
"""

import ctypes as C

import numpy as np
import pytest


def _create(n_nodes, max_states, device=-1):
    from gym_pbn_amd import _lib

    h = C.c_void_p()
    rc = _lib.lib.pbn_census_create(n_nodes, device, max_states, C.byref(h))
    return rc, h


def _run(h, n_updates, first, stride, mask=None, batch=None):
    from gym_pbn_amd import _lib

    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint64)
    return _lib.lib.pbn_census_run_device(batch, h, n_updates, first, stride, _lib.ptr(m, _lib._u64p))


def test_create_refusals_and_host_only_info():
    from gym_pbn_amd import _lib

    for n_nodes in (0, -3, 513):
        rc, h = _create(n_nodes, 16)
        assert rc == _lib.PBN_E_INVALID and "n_nodes" in _lib.last_error() and not h.value
    for max_states in (0, (1 << 24) + 1, 1 << 40):
        rc, h = _create(28, max_states)
        assert rc == _lib.PBN_E_INVALID and "max_states" in _lib.last_error() and not h.value
    assert _lib.lib.pbn_census_create(28, -1, 16, None) == _lib.PBN_E_INVALID
    assert C.sizeof(_lib.CensusInfo) == 56  # three int32 (+ padding), five uint64: the header's struct
    for n_nodes, max_states, words, slots in ((1, 1, 1, 64), (64, 32, 1, 64), (65, 33, 2, 128), (512, 1 << 24, 8, 1 << 25)):
        rc, h = _create(n_nodes, max_states)
        assert rc == 0 and h.value
        i = _lib.CensusInfo()
        assert _lib.lib.pbn_census_get_info(h, C.byref(i)) == 0
        assert (i.n_nodes, i.n_words, i.device, i.max_states, i.table_slots) == (n_nodes, words, -1, max_states, slots)
        assert (i.n_states, i.visits, i.dropped) == (0, 0, 0)
        # clear and read work on a host-only handle: it holds nothing
        assert _lib.lib.pbn_census_clear(h) == 0
        n = C.c_uint64(7)
        assert _lib.lib.pbn_census_read(h, None, None, 0, C.byref(n)) == 0 and n.value == 0
        _lib.lib.pbn_census_destroy(h)
    _lib.lib.pbn_census_destroy(None)


def test_run_refusals_come_before_anything_else():
    """Every PBN_E_INVALID case of pbn_census_run_device that the census alone decides, then PBN_E_STATE for the
    host-only handle -- with a NULL batch, which would otherwise be refused first."""
    from gym_pbn_amd import _lib

    rc, h = _create(65, 16)
    assert rc == 0
    assert _run(None, 1, 0, 1) == _lib.PBN_E_INVALID and _lib.last_error() == "census is NULL"
    assert _run(h, 5, 0, 0) == _lib.PBN_E_INVALID and "stride" in _lib.last_error()
    assert _run(h, 5, 6, 1) == _lib.PBN_E_INVALID and "first" in _lib.last_error()
    assert _run(h, 0, 1, 1) == _lib.PBN_E_INVALID and "first" in _lib.last_error()
    assert _run(h, 65537, 0, 1) == _lib.PBN_E_INVALID and "n_updates" in _lib.last_error()
    assert _run(h, 0xFFFFFFFF, 0, 1) == _lib.PBN_E_INVALID
    assert _run(h, 5, 0, 1, mask=[0, 2]) == _lib.PBN_E_INVALID and "past node 64" in _lib.last_error()
    assert _run(h, 5, 0, 1, mask=[0, 1 << 63]) == _lib.PBN_E_INVALID
    # valid arguments reach the device part: refused as a host-only handle
    for args in ((5, 0, 1), (5, 5, 1), (0, 0, 1), (65536, 0, 0xFFFFFFFF), (33, 3, 4)):
        assert _run(h, *args) == _lib.PBN_E_STATE, args
        assert "host-only" in _lib.last_error()
    assert _run(h, 5, 0, 1, mask=[~0 & ((1 << 64) - 1), 1]) == _lib.PBN_E_STATE  # nodes 0 .. 64: all in range
    i = _lib.CensusInfo()
    assert _lib.lib.pbn_census_get_info(h, C.byref(i)) == 0 and (i.visits, i.n_states, i.dropped) == (0, 0, 0)
    # NULL arguments
    assert _lib.lib.pbn_census_get_info(None, C.byref(i)) == _lib.PBN_E_INVALID
    assert _lib.lib.pbn_census_get_info(h, None) == _lib.PBN_E_INVALID
    assert _lib.lib.pbn_census_clear(None) == _lib.PBN_E_INVALID
    assert _lib.lib.pbn_census_read(h, None, None, 0, None) == _lib.PBN_E_INVALID
    assert _lib.lib.pbn_census_get_stats(h, None, None) == _lib.PBN_E_INVALID
    _lib.lib.pbn_census_destroy(h)
    # N a multiple of 64: no bit of the last word is stray
    rc, h = _create(128, 16)
    assert _run(h, 1, 0, 1, mask=[1, 1 << 63]) == _lib.PBN_E_STATE
    _lib.lib.pbn_census_destroy(h)


def test_state_census_host_only_handle():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.census import StateCensus
    from gym_pbn_amd.network import load_network

    c = StateCensus(load_network("bittner28"), max_states=100, device=None)
    assert c.info() == dict(n_nodes=28, n_words=1, device=-1, max_states=100, table_slots=256, n_states=0, visits=0,
                            dropped=0)
    assert c.node_mask([0, 27]).tolist() == [1 | 1 << 27]
    with pytest.raises(ValueError):
        c.node_mask([28])
    r = c.result()
    assert len(r) == 0 and r.states.shape == (0, 1) and r.visits == 0 and r.frequencies().shape == (0,)
    c.clear()
    c.close()
    with pytest.raises(ValueError):
        StateCensus(28, max_states=0, device=None)
    w = StateCensus(65, device=None)
    assert w.n_words == 2 and w.node_mask([63, 64]).tolist() == [1 << 63, 1]

    class FakeBatch:
        handle = None

    with pytest.raises(ValueError, match="stride"):
        w.run(FakeBatch(), 4, stride=0)
    with pytest.raises(_lib.PbnError) as ei:
        w.run(FakeBatch(), 4)
    assert ei.value.code == _lib.PBN_E_STATE
    import gym_pbn_amd

    assert gym_pbn_amd.StateCensus is StateCensus and callable(gym_pbn_amd.statistical_attractors)


def test_census_result_sorting_ties_and_helpers():
    from gym_pbn_amd.census import CensusResult

    # N = 65: two words. Counts 5, 9, 5, 9, 1; the ties are ordered by the state as an integer, word 1 first
    states = np.array([[7, 1], [3, 0], [9, 0], [2, 1], [0, 0]], dtype=np.uint64)
    counts = np.array([5, 9, 5, 9, 1], dtype=np.uint64)
    r = CensusResult(65, states, counts, visits=32, dropped=3)
    assert r.counts.tolist() == [9, 9, 5, 5, 1]
    assert r.states.tolist() == [[3, 0], [2, 1], [9, 0], [7, 1], [0, 0]]
    assert len(r) == 5 and not r.exact
    # the order does not depend on the input order
    perm = np.array([4, 2, 0, 3, 1])
    p = CensusResult(65, states[perm], counts[perm], visits=32, dropped=3)
    assert np.array_equal(p.states, r.states) and np.array_equal(p.counts, r.counts)
    t = r.top(3)
    assert t.states.tolist() == [[3, 0], [2, 1], [9, 0]] and t.counts.tolist() == [9, 9, 5]
    assert (t.visits, t.dropped) == (32, 3)
    assert len(r.top(0)) == 0 and len(r.top(99)) == 5
    assert np.array_equal(r.frequencies(), np.array([9, 9, 5, 5, 1]) / 29)
    assert CensusResult(65, states[:0], counts[:0]).frequencies().shape == (0,)
    lists = t.states_lists()
    assert all(isinstance(s, tuple) and len(s) == 65 for s in lists)
    assert lists[0] == (1, 1) + (0,) * 63  # state 3: nodes 0 and 1
    assert lists[1] == (0, 1) + (0,) * 62 + (1,)  # word 0 = 2: node 1; word 1 = 1: node 64
    # counts past 2^32 keep their order and their value
    big = CensusResult(8, [[1], [2]], [1 << 40, (1 << 40) + 1], visits=(1 << 41) + 1)
    assert big.states.tolist() == [[2], [1]] and int(big.counts[0]) == (1 << 40) + 1 and big.exact
    with pytest.raises(ValueError):
        CensusResult(8, [[1], [2]], [1])
    # the labelled set: rank = label
    s = r.state_set(k=4, device=None)
    assert len(s) == 4 and s.lookup(r.states).tolist() == [0, 1, 2, 3, -1]
    assert len(r.state_set(device=None)) == 5


def test_occupancy_splits_the_counts_by_attractor():
    from gym_pbn_amd.attractors import AttractorResult
    from gym_pbn_amd.census import CensusResult

    att = AttractorResult(8, attractors=[np.array([[1], [2]], np.uint64), np.array([[7]], np.uint64)], seed_counts=[1, 1])
    r = CensusResult(8, [[1], [2], [7], [9], [11]], [10, 20, 5, 3, 4], visits=42)
    per, outside = att.occupancy(r)
    assert per.tolist() == [30, 5] and outside == 7 and int(per.sum()) + outside == r.visits


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ is not installed")
def test_census_header_is_clean_under_asan_and_ubsan():
    """``make censuscheck``: tests/host/census_check.cpp on csrc/pbn_census.hpp alone (no HIP header, no library, no
    GPU) with ASan + UBSan: table sizing, the sample-point walk against a modulus, the sequential model of the slot /
    entry layout against a std::map for W = 1 .. 8 (exact counts, overflow accounting, dead entries reused by later
    launches, a full table) and the compaction."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(["make", "-C", str(root / "gym-pbn-stac_amd"), "censuscheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "census_check ok" in r.stdout
