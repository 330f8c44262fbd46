"""The exact transition graph (``pbn_stg_*``, ``csrc/pbn_mass_rule.hpp``) without a GPU: the host statement of the
edge mass (``pbn_net_edge_mass``) against a restatement in numpy, its support against ``pbn_net_unstable``, the
reference's ``getNextStates`` pinned through ``TransitionGraph.next_states``, the refusals of the C entry points on a
host-only handle, and the rule header under ASan + UBSan (``make massrulecheck``).

The numpy restatements live here (``np_edge_mass``, ``np_tt_edge_mass``): the GPU tests import them as the independent
statement the kernel is checked against.
"""

import ctypes as C
import functools
import json

import numpy as np
import pytest

from conftest import GOLDEN
from shape_cases import tt_net
from test_attractors_host import CASES, all_states, case_id, case_network, embed_network, lift_states

TWO53 = 1 << 53
GRAPHS = ("stg", "step")
EMBED_TOTALS = [64, 65, 128, 192, 256, 257, 384, 448, 512]  # every W; ending at bit 63, straddling 63 | 64, the last bit of W = 8


def case_by(n, max_preds, seed):
    return next(c for c in CASES if (c["n_nodes"], c["max_preds"], c["seed"]) == (n, max_preds, seed))


# ---------------------------------------------------------------- the restatements
def np_edge_mass(net, bits):
    """``[S][N]`` uint64: ``PredictorNetwork.update_probability``'s integer arithmetic (network.py), vectorised over
    states -- the summed widths of the predictors voting 1, kept for ``x_i = 0`` and taken from ``2**53`` for 1."""
    bits = np.asarray(bits, dtype=np.uint8)
    out = np.zeros(bits.shape, dtype=np.uint64)
    for i in range(net.n_nodes):
        o0, o1 = int(net.pred_offsets[i]), int(net.pred_offsets[i + 1])
        prev = 0
        xi = bits[:, i]
        mass1 = np.zeros(len(bits), dtype=np.uint64)
        for j in range(o0, o1):
            t = min(int(net.pred_thr[j]), TWO53) if j < o1 - 1 else TWO53
            w = max(t - prev, 0)
            prev = max(prev, t)
            a, b, c = (int(v) for v in net.pred_inputs[j])
            p = (bits[:, a] << 3) | (bits[:, b] << 2) | (bits[:, c] << 1) | xi
            table = np.array([(int(net.pred_tt[j]) >> k) & 1 for k in range(16)], dtype=np.uint8)
            mass1 += np.where(table[p] == 1, np.uint64(w), np.uint64(0))
        out[:, i] = np.where(xi == 1, np.uint64(TWO53) - mass1, mass1)
    return out


def np_tt_edge_mass(net, bits, graph):
    """``[S][N]`` uint64 from ``thr``: ``T`` from 0, ``2**53 - T`` from 1; node 0 frozen under ``"step"``."""
    bits = np.asarray(bits, dtype=np.uint8)
    out = np.zeros(bits.shape, dtype=np.uint64)
    for i in range(1 if graph == "step" else 0, net.n_nodes):
        k, io, to = int(net.node_k[i]), int(net.input_offsets[i]), int(net.thr_offsets[i])
        idx = np.zeros(len(bits), dtype=np.int64)
        for q in range(k):
            idx = (idx << 1) | bits[:, int(net.inputs[io + q])]
        T = np.minimum(net.thr[to + idx], np.uint64(TWO53))
        out[:, i] = np.where(bits[:, i] == 1, np.uint64(TWO53) - T, T)
    return out


def random_words(n_nodes, count, seed):
    from gym_pbn_amd.batch import pack_bits

    return pack_bits(np.random.default_rng(seed).integers(0, 2, size=(count, n_nodes), dtype=np.uint8))


def check_mass_and_support(net, words, graph=None):
    """The two identities every network of this file is held to; returns the host masses."""
    from gym_pbn_amd.attractors import host_unstable
    from gym_pbn_amd.batch import pack_bits, unpack_bits
    from gym_pbn_amd.transition import host_edge_mass

    bits = unpack_bits(words, net.n_nodes)
    got = host_edge_mass(net, words, graph)
    want = np_edge_mass(net, bits) if graph is None else np_tt_edge_mass(net, bits, graph)
    assert got.dtype == np.uint64 and got.shape == (len(words), net.n_nodes)
    assert np.array_equal(got, want)
    assert int(got.max()) <= TWO53
    assert np.array_equal(pack_bits((got > 0).astype(np.uint8)), host_unstable(net, words, graph))
    return got


# ---------------------------------------------------------------- the mass against its restatement
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_host_mass_on_every_state_of_the_golden_nets(c):
    net = case_network(c)
    m = check_mass_and_support(net, all_states(c["n_nodes"]))
    assert (m > 0).any() and (m == 0).any()


@pytest.mark.parametrize("name", ["bittner70", "bittner199"])
def test_host_mass_on_random_states_of_the_bittner_nets(name):
    from gym_pbn_amd.network import load_network

    net = load_network(name)
    m = check_mass_and_support(net, random_words(net.n_nodes, 257, 3))
    assert ((m > 0) & (m < TWO53)).any()  # cells that are neither certain nor impossible


@pytest.mark.parametrize("graph", GRAPHS)
def test_host_mass_truth_table(graph):
    net = tt_net(64)
    m = check_mass_and_support(net, random_words(64, 257, 4), graph)
    assert (m[:, 0] == 0).all() == (graph == "step")  # under "step" node 0 never moves
    assert ((m > 0) & (m < TWO53)).any()


def test_host_mass_rules_of_the_graph_argument():
    from gym_pbn_amd.transition import host_edge_mass

    with pytest.raises(ValueError, match="table_graph"):
        host_edge_mass(tt_net(64), random_words(64, 2, 0))
    c = case_by(10, 2, 0)
    net = case_network(c)
    s = all_states(10)[:5]
    assert np.array_equal(host_edge_mass(net, s), host_edge_mass(net, s, "step"))  # ignored for a predictor mix


@pytest.mark.parametrize("n_total", EMBED_TOTALS)
def test_host_mass_embedded_across_the_word_boundary(n_total):
    """The golden N = 10 net at the top of 64 / 65 / ... / 512 nodes (the layout of
    ``test_unstable_embedded_across_the_word_boundary``): frozen nodes have mass 0, and the masses are the small
    net's at the moved positions."""
    small = case_network(case_by(10, 2, 0))
    place = list(range(n_total - 10, n_total))
    big = embed_network(small, n_total, place)
    frozen = np.random.default_rng(5).integers(0, 2, size=n_total, dtype=np.uint8)
    states = lift_states(all_states(10), 10, n_total, place, frozen)
    got = check_mass_and_support(big, states)
    want = np.zeros((1024, n_total), dtype=np.uint64)
    want[:, place] = check_mass_and_support(small, all_states(10))
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- the reference pin
@functools.lru_cache(maxsize=None)
def stg_fixture():
    return json.loads((GOLDEN / "stg_small.json").read_text())["cases"]


def as_int(state):
    return sum(int(v) << i for i, v in enumerate(state))


def test_next_states_agrees_with_the_reference():
    """``TransitionGraph.next_states`` (host only) against ``Graph.getNextStates`` of every state of two golden nets:
    the same keys, and every probability within a bound derived here, in units of ``u = 2**-53``.

    Node ``i`` with cumulative CODs ``c_1 .. c_m`` (doubles; ``c_m == CODsum`` exactly, the same additions) has the
    real masses ``P = sum (c_q - c_{q-1}) / CODsum`` over the predictors voting one way.

    * Ours. ``T_q`` is the smallest ``k`` with ``fl(k * 2**-53 * CODsum) >= c_q``; one rounding of relative size ``u``
      puts it in ``[x - 1, x + 2 + eps]`` for ``x = 2**53 c_q / CODsum <= 2**53``. ``T_0 = 0`` and ``T_m = 2**53`` are
      exact, so a sum of widths carries at most ``pmax - 1`` interior thresholds: at most ``2 (pmax - 1)`` grid
      units (plus ``eps``, covered by the slack unit below). Then one correctly rounded division: ``u``.
    * The reference. ``currCOD = fl(c_q - c_{q-1})``, ``fl(currCOD / CODsum)``: ``2 u`` relative on terms that add
      up to at most 1; ``probs[Y] +=`` at most ``pmax - 1`` roundings of partial sums ``<= 1``; ``/ len(state)``: one.
      In all ``(pmax + 2) u`` on the node's probability, before the division by ``N``.

    So a flip entry differs by at most ``(3 pmax + 2) u / N``. The stay entry adds the ``N`` nodes' errors and the
    reference's ``N - 1`` rounded additions of partial sums ``<= 1``: ``(3 pmax + 2 + N) u``. Measured on these two
    nets: largest flip deviation 0.062 u at N = 8 and 0.125 u at N = 10 (bounds 1.0 u and 0.8 u),
    largest stay deviation 1.0 u on both (bounds 16 u and 18 u)."""
    from gym_pbn_amd.transition import TransitionGraph

    u = 2.0 ** -53
    assert len(stg_fixture()) == 2
    for fx in stg_fixture():
        n = fx["n_nodes"]
        net = case_network(case_by(n, fx["max_preds"], fx["seed"]))
        pmax = int(np.diff(net.pred_offsets).max())
        want = {}
        for s, t, p in fx["edges"]:
            want.setdefault(s, {})[t] = p
        assert sorted(want) == list(range(1 << n))
        g = TransitionGraph(net, all_states(n), device=None)
        worst_flip = worst_stay = 0.0
        for s in range(1 << n):
            got = {as_int(t): p for t, p in g.next_states(s).items()}
            assert sorted(got) == sorted(want[s]), f"state {s}: keys differ"
            assert abs(sum(got.values()) - 1.0) <= (n + 1) * u
            for t, p in got.items():
                dev = abs(p - want[s][t])
                if t == s:
                    worst_stay = max(worst_stay, dev)
                else:
                    worst_flip = max(worst_flip, dev)
        print(f"N={n} pmax={pmax}: largest flip deviation {worst_flip / u:.3f} u, stay {worst_stay / u:.3f} u")
        assert worst_flip <= (3 * pmax + 2) * u / n
        assert worst_stay <= (3 * pmax + 2 + n) * u
        g.close()


def test_next_states_merges_and_states_forms():
    """State tuples and packed rows are the same input; a frozen state maps to itself with probability 1."""
    from gym_pbn_amd.batch import unpack_bits
    from gym_pbn_amd.transition import TransitionGraph

    c = case_by(10, 2, 8)  # its attractor has 2 states
    net = case_network(c)
    words = all_states(10)
    tuples = [tuple(int(v) for v in row) for row in unpack_bits(words[:7], 10)]
    a = TransitionGraph(net, words[:7], device=None)
    b = TransitionGraph(net, tuples, device=None)
    assert np.array_equal(a.states, b.states) and len(a) == 7
    assert a.next_states(3) == b.next_states(3)
    assert all(isinstance(t, tuple) and len(t) == 10 for t in a.next_states(3))
    with pytest.raises(ValueError):
        a.next_states(7)
    with pytest.raises(ValueError):
        TransitionGraph(net, [(0, 1, 2) + (0,) * 7], device=None)  # not 0 / 1
    with pytest.raises(ValueError):
        TransitionGraph(net, [(0,) * 9], device=None)  # not N values
    with pytest.raises(ValueError, match="table_graph"):
        TransitionGraph(net, words[:7], table_graph="stg", device=None)
    with pytest.raises(ValueError, match="table_graph"):
        TransitionGraph(tt_net(64), random_words(64, 3, 0), device=None)
    t = TransitionGraph(tt_net(64), random_words(64, 3, 0), table_graph="step", device=None)
    assert (t.first_node, t.n_movable) == (1, 63)
    d = t.next_states(0)
    assert abs(sum(d.values()) - 1.0) <= 65 * 2.0 ** -53
    import gym_pbn_amd
    from gym_pbn_amd.transition import host_edge_mass

    assert gym_pbn_amd.TransitionGraph is TransitionGraph and gym_pbn_amd.host_edge_mass is host_edge_mass


# ---------------------------------------------------------------- refusals of the C entry points
def _stg_create(net, device, graph, states, n=None):
    from gym_pbn_amd import _lib

    h = C.c_void_p()
    w = None if states is None else np.ascontiguousarray(states, dtype=np.uint64)
    n = (0 if w is None else len(w)) if n is None else n
    rc = _lib.lib.pbn_stg_create(net, device, graph, _lib.ptr(w, _lib._u64p), n, C.byref(h))
    return rc, h


def test_refusals_of_every_new_entry_point():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import Net

    pm = Net(case_network(case_by(10, 2, 0)))
    tt = Net(tt_net(64))
    lib = _lib.lib
    s = all_states(10)[:5]
    out = np.zeros((5, 10), dtype=np.uint64)
    # pbn_net_edge_mass
    assert lib.pbn_net_edge_mass(None, 0, _lib.ptr(s, _lib._u64p), 5, _lib.ptr(out, _lib._u64p)) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "net is NULL"
    assert lib.pbn_net_edge_mass(pm.handle, 0, None, 5, _lib.ptr(out, _lib._u64p)) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "states is NULL"
    assert lib.pbn_net_edge_mass(pm.handle, 0, _lib.ptr(s, _lib._u64p), 5, None) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "mass is NULL"
    assert lib.pbn_net_edge_mass(pm.handle, 0, _lib.ptr(s, _lib._u64p), 0, _lib.ptr(out, _lib._u64p)) == _lib.PBN_E_INVALID
    assert "n_states" in _lib.last_error()
    w = random_words(64, 2, 0)
    o = np.zeros((2, 64), dtype=np.uint64)
    for bad in (0, 3, -1):
        assert lib.pbn_net_edge_mass(tt.handle, bad, _lib.ptr(w, _lib._u64p), 2, _lib.ptr(o, _lib._u64p)) == _lib.PBN_E_INVALID
        assert "PBN_TABLE_GRAPH" in _lib.last_error()
    # pbn_stg_create
    rc, h = _stg_create(None, -1, 0, s)
    assert rc == _lib.PBN_E_INVALID and _lib.last_error() == "net is NULL" and not h.value
    assert lib.pbn_stg_create(pm.handle, -1, 0, _lib.ptr(s, _lib._u64p), 5, None) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "out is NULL"
    rc, h = _stg_create(pm.handle, -1, 0, None, n=5)
    assert rc == _lib.PBN_E_INVALID and _lib.last_error() == "states is NULL" and not h.value
    for n in (0, (1 << 24) + 1):
        rc, h = _stg_create(pm.handle, -1, 0, s, n=n)
        assert rc == _lib.PBN_E_INVALID and "n_states" in _lib.last_error() and not h.value
    rc, h = _stg_create(pm.handle, -2, 0, s)
    assert rc == _lib.PBN_E_RANGE and "device" in _lib.last_error() and not h.value
    for bad in (0, 3):
        rc, h = _stg_create(tt.handle, -1, bad, w)
        assert rc == _lib.PBN_E_INVALID and "PBN_TABLE_GRAPH" in _lib.last_error() and not h.value
    rc, h = _stg_create(pm.handle, -1, 0, [[1], [2], [1]])
    assert rc == _lib.PBN_E_INVALID and "state 2 repeats" in _lib.last_error() and not h.value
    rc, h = _stg_create(pm.handle, -1, 0, [[1], [1 << 10]])
    assert rc == _lib.PBN_E_INVALID and "state 1 has bits set beyond node 9" in _lib.last_error() and not h.value
    # a host-only handle: get_info answers, device calls are refused
    assert C.sizeof(_lib.StgInfo) == 40  # six int32, two uint64: the header's struct
    rc, h = _stg_create(tt.handle, -1, _lib.TABLE_GRAPH_STEP, w)
    assert rc == 0 and h.value
    i = _lib.StgInfo()
    assert lib.pbn_stg_get_info(h, C.byref(i)) == 0
    assert (i.n_nodes, i.n_words, i.first_node, i.n_movable, i.device, i.table_graph, i.n_states, i.leaks) == \
        (64, 1, 1, 63, -1, _lib.TABLE_GRAPH_STEP, 2, 0)
    lib.pbn_stg_destroy(h)
    rc, h = _stg_create(pm.handle, -1, 77, s)  # the graph code is ignored for a predictor mix
    assert rc == 0
    assert lib.pbn_stg_get_info(h, C.byref(i)) == 0
    assert (i.n_nodes, i.first_node, i.n_movable, i.table_graph, i.n_states) == (10, 0, 10, 0, 5)
    assert lib.pbn_stg_get_info(None, C.byref(i)) == _lib.PBN_E_INVALID and _lib.last_error() == "stg is NULL"
    assert lib.pbn_stg_get_info(h, None) == _lib.PBN_E_INVALID and _lib.last_error() == "info is NULL"
    assert lib.pbn_stg_clear_leaks(None) == _lib.PBN_E_INVALID and _lib.last_error() == "stg is NULL"
    assert lib.pbn_stg_clear_leaks(h) == 0
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    assert lib.pbn_stg_rows_device(None, 0, 1, fake, fake) == _lib.PBN_E_INVALID and _lib.last_error() == "stg is NULL"
    for first, n in ((6, 0), (0, 6), (5, 1), (3, 3), (1 << 63, 1 << 63)):
        assert lib.pbn_stg_rows_device(h, first, n, fake, fake) == _lib.PBN_E_RANGE, (first, n)
        assert "reach past the 5 states" in _lib.last_error()
    assert lib.pbn_stg_rows_device(h, 0, 5, None, fake) == _lib.PBN_E_INVALID and _lib.last_error() == "d_mass is NULL"
    assert lib.pbn_stg_rows_device(h, 0, 5, fake, None) == _lib.PBN_E_INVALID and _lib.last_error() == "d_succ is NULL"
    for first, n in ((0, 5), (4, 1), (5, 0), (0, 0)):
        assert lib.pbn_stg_rows_device(h, first, n, fake, fake) == _lib.PBN_E_STATE, (first, n)
        assert "host-only" in _lib.last_error()
    lib.pbn_stg_destroy(h)
    lib.pbn_stg_destroy(None)


def test_transition_graph_host_only_handle():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.attractors import AttractorResult
    from gym_pbn_amd.transition import TransitionGraph

    c = case_by(10, 2, 0)
    net = case_network(c)
    g = TransitionGraph(net, all_states(10), device=None)
    assert g.info() == dict(n_nodes=10, n_words=1, first_node=0, n_movable=10, device=-1, table_graph=0,
                            n_states=1024, leaks=0)
    with pytest.raises(_lib.PbnError) as ei:
        g.rows(0, 4)
    assert ei.value.code == _lib.PBN_E_STATE
    with pytest.raises(ValueError):
        g.rows(5, 2000)
    g.close()
    att = [np.array([[3], [5]], np.uint64)]
    with pytest.raises(ValueError, match="network"):
        AttractorResult(10, attractors=att).transition_graph(0, device=None)
    t = AttractorResult(10, attractors=att).transition_graph(0, device=None, network=net)
    assert len(t) == 2 and t.device is None


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ is not installed")
def test_mass_rule_header_is_clean_under_asan_and_ubsan():
    """``make massrulecheck``: tests/host/mass_rule_check.cpp on csrc/pbn_mass_rule.hpp (no HIP header, no library, no
    GPU) with ASan + UBSan: a hand-written image of each kind with the masses by hand, and packer-built images of
    random networks against a restatement from the descriptor, the two values' masses adding up to 2**53, and
    ``mass > 0`` against the support rule."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(["make", "-C", str(root / "gym-pbn-stac_amd"), "massrulecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mass_rule_check ok" in r.stdout
