"""Attractor discovery for truth-table networks, host side: the edge rule restated in numpy, the host entry
point ``pbn_net_unstable`` pinned against it, the env switch.

The numpy restatement lives here (``np_tt_unstable``): node ``i`` can flip at ``x`` iff its table entry ``p``
at ``x`` (a double, looked up in ``probs``) has ``p > 0.0`` with ``x_i = 0`` or ``p < 1.0`` with ``x_i = 1``,
over nodes ``0..N-1`` (``"stg"``) or ``1..N-1`` (``"step"``). It never sees a threshold or the C++. The GPU
tests import it as the independent statement the kernels are checked against.

Golden ``"stg"`` attractors come from the reference's own ``PBN.print_STG`` + ``attracting_components``
(``tests/golden/attractors_tt_small.json``); the ``"step"`` graph has no reference function, so its expected
sets come from the restatement with column 0 masked (sizes recorded in the fixture).
"""

import functools
import json

import numpy as np
import pytest

from conftest import GOLDEN
from test_attractors_host import all_states, lift_states, np_unstable_words

GRAPHS = ("stg", "step")


# ---------------------------------------------------------------- fixtures and helpers
CASES = json.loads((GOLDEN / "attractors_tt_small.json").read_text())["cases"]


def case_id(c):
    return f"n{c['n_nodes']}-k{c['k']}-d{c['det']}-s{c['seed']}"


def case_by(n, k, det, seed):
    return next(c for c in CASES if (c["n_nodes"], c["k"], c["det"], c["seed"]) == (n, k, det, seed))


def case_pbn_data(c):
    out = []
    for i, (mask, table) in enumerate(zip(c["masks"], c["tables"])):
        m = np.asarray(mask, dtype=bool)
        out.append((m, np.asarray(table, dtype=np.float64).reshape((2,) * int(m.sum())), f"n{i}", False))
    return out


def case_network(c):
    from gym_pbn_amd.network import TruthTableNetwork

    return TruthTableNetwork.from_pbn_data(case_pbn_data(c), name=case_id(c))


def np_tt_unstable(net, bits, graph):
    """``[S][N]`` bool: node i can flip at state s (bits ``[S][N]`` 0/1) in the named graph."""
    bits = np.asarray(bits, dtype=np.int64)
    out = np.zeros(bits.shape, dtype=bool)
    for i in range({"stg": 0, "step": 1}[graph], net.n_nodes):
        ins = net.inputs[int(net.input_offsets[i]):int(net.input_offsets[i + 1])]
        code = np.zeros(len(bits), dtype=np.int64)
        for j in ins:  # ascending node order, the first input most significant
            code = 2 * code + bits[:, int(j)]
        p = net.probs[int(net.thr_offsets[i]):int(net.thr_offsets[i + 1])][code]
        out[:, i] = ((p > 0.0) & (bits[:, i] == 0)) | ((p < 1.0) & (bits[:, i] == 1))
    return out


def np_tt_unstable_words(net, words, graph):
    from gym_pbn_amd.batch import pack_bits, unpack_bits

    return pack_bits(np_tt_unstable(net, unpack_bits(words, net.n_nodes), graph).astype(np.uint8))


def np_tt_attractors(net, graph):
    """Terminal strongly connected components over all 2^N states (N small): sorted packed arrays ``[S][1]``,
    ordered by (size, smallest state) like ``find_attractors``."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    from gym_pbn_amd.batch import unpack_bits

    n = 1 << net.n_nodes
    src, node = np.nonzero(np_tt_unstable(net, unpack_bits(all_states(net.n_nodes), net.n_nodes), graph))
    dst = src ^ (1 << node)
    g = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n)).tocsr()
    n_comp, label = connected_components(g, directed=True, connection="strong")
    leaves = np.ones(n_comp, dtype=bool)
    leaves[label[src][label[src] != label[dst]]] = False
    out = [np.flatnonzero(label == k).astype(np.uint64).reshape(-1, 1) for k in np.flatnonzero(leaves)]
    return sorted(out, key=lambda a: (len(a), int(a[0, 0])))


def fixture_attractors(c):
    """The reference's ``"stg"`` attractors as sorted packed arrays, ordered by (size, smallest state)."""
    from gym_pbn_amd.attractors import sort_rows
    from gym_pbn_amd.batch import pack_bits

    out = [sort_rows(pack_bits(np.asarray(a, dtype=np.uint8))) for a in c["attractors"]]
    return sorted(out, key=lambda a: (len(a), int(a[0, 0])))


@functools.lru_cache(maxsize=None)
def _expected(index, graph):
    c = CASES[index]
    return fixture_attractors(c) if graph == "stg" else np_tt_attractors(case_network(c), "step")


def expected_attractors(c, graph):
    """Expected attractors of a fixture case: the reference's for ``"stg"``, the restatement's for ``"step"``.
    Computed once per case and shared; callers do not modify them."""
    return _expected(CASES.index(c), graph)


EPS0 = float(np.nextafter(0.0, 1.0))  # the smallest double above 0
EPS1 = float(np.nextafter(1.0, 0.0))  # the largest double below 1


def edge_value_network():
    """Nine nodes with k = 0, 0, 0, 1, ..., 6 inputs; the k = 0 tables are 0.0, 1.0 and 0.5, the others cycle
    through 0.0, 1.0, the two doubles next to them, and ordinary values."""
    from gym_pbn_amd.network import TruthTableNetwork

    n = 9
    ks = [0, 0, 0, 1, 2, 3, 4, 5, 6]
    consts = [0.0, 1.0, 0.5]
    cycle = [EPS0, 1.0, EPS1, 0.0, 0.25, 0.0, 1.0, EPS0, 0.75, EPS1]
    rng = np.random.default_rng(21)
    data, at = [], 0
    for i, k in enumerate(ks):
        mask = np.zeros(n, dtype=bool)
        if k:
            mask[rng.choice(n, size=k, replace=False)] = True  # a node may be its own input
            table = np.array([cycle[(at + e) % len(cycle)] for e in range(1 << k)]).reshape((2,) * k)
            at += 3
        else:
            table = np.array(consts[i])
        data.append((mask, table, f"n{i}", False))
    net = TruthTableNetwork.from_pbn_data(data, name="edge-values")
    assert list(net.node_k) == ks
    return net


def embed_tt_network(net, n_total, place, name="embedded"):
    """``net``'s nodes placed at positions ``place`` (ascending) of an ``n_total``-node network; every other node
    is frozen by the self-input table ``[0, 1]`` (it keeps its value with probability one)."""
    from gym_pbn_amd.network import TruthTableNetwork

    place = [int(p) for p in place]
    assert place == sorted(place)  # keeps every node's inputs in the same order
    at = {p: i for i, p in enumerate(place)}
    data = []
    for v in range(n_total):
        mask = np.zeros(n_total, dtype=bool)
        if v in at:
            i = at[v]
            k = int(net.node_k[i])
            ins = net.inputs[int(net.input_offsets[i]):int(net.input_offsets[i + 1])]
            mask[[place[int(j)] for j in ins]] = True
            table = net.probs[int(net.thr_offsets[i]):int(net.thr_offsets[i + 1])].reshape((2,) * k)
        else:
            mask[v] = True
            table = np.array([0.0, 1.0])
        data.append((mask, table, f"n{v}", False))
    return TruthTableNetwork.from_pbn_data(data, name=name)


def copies_pbn_data(c, copies):
    """``PBN_data`` of ``copies`` disjoint copies of a fixture network side by side (copy m at nodes
    ``m*n .. m*n + n - 1``, its inputs shifted with it): the support graphs are the products of the copies' graphs."""
    n = c["n_nodes"]
    data = []
    for m in range(copies):
        for mask, table, _, _ in case_pbn_data(c):
            big = np.zeros(n * copies, dtype=bool)
            big[m * n:(m + 1) * n] = mask
            data.append((big, table, f"n{len(data)}", False))
    return data


def copies_network(c, copies):
    from gym_pbn_amd.network import TruthTableNetwork

    return TruthTableNetwork.from_pbn_data(copies_pbn_data(c, copies), name=f"{case_id(c)}-x{copies}")


def product_states(parts, n):
    """Packed states of the side-by-side network: every combination of one ``n``-node state per copy.
    ``parts[m]``: packed ``[S_m][1]`` states of copy m. Rows ordered with the last copy varying fastest."""
    from gym_pbn_amd.batch import pack_bits, unpack_bits

    grids = np.meshgrid(*[np.arange(len(p)) for p in parts], indexing="ij")
    bits = np.concatenate([unpack_bits(p, n)[g.reshape(-1)] for p, g in zip(parts, grids)], axis=1)
    return pack_bits(bits)


# ---------------------------------------------------------------- the numpy rule against the reference
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_numpy_rule_reproduces_fixture_attractors(c):
    from gym_pbn_amd.batch import unpack_bits
    from gym_pbn_amd.stg import compute_attractors

    net = case_network(c)
    got = np_tt_attractors(net, "stg")
    want = expected_attractors(c, "stg")
    assert [len(a) for a in got] == [len(a) for a in want]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # the host route the envs take today gives the same sets
    stg = {frozenset(a) for a in compute_attractors(net)}
    assert stg == {frozenset(tuple(s) for s in a) for a in c["attractors"]}
    # the step graph: column 0 masked; sizes as recorded when the fixture was made, and another graph
    step = expected_attractors(c, "step")
    assert sorted(len(a) for a in step) == c["step_sizes"]
    assert [a.tolist() for a in step] != [a.tolist() for a in want]
    for a in step:  # closed under the step graph's moves
        src, node = np.nonzero(np_tt_unstable(net, unpack_bits(a, c["n_nodes"]), "step"))
        succ = a[src, 0] ^ (np.uint64(1) << node.astype(np.uint64))
        assert np.isin(succ, a[:, 0]).all()


# ---------------------------------------------------------------- pbn_net_unstable against the numpy rule
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_host_rule_on_every_state_of_the_fixture_nets(c, graph):
    from gym_pbn_amd.attractors import host_unstable

    net = case_network(c)
    states = all_states(c["n_nodes"])
    got = host_unstable(net, states, graph)
    assert got.shape == states.shape
    assert np.array_equal(got, np_tt_unstable_words(net, states, graph))
    if graph == "step":
        assert not (got[:, 0] & np.uint64(1)).any()  # node 0 never moves


@pytest.mark.parametrize("graph", GRAPHS)
def test_host_rule_at_the_edges_of_the_probability_range(graph):
    """``nextafter(0, 1)`` and ``nextafter(1, 0)`` are edges; 0.0 and 1.0 are not."""
    from gym_pbn_amd.attractors import host_unstable
    from gym_pbn_amd.batch import unpack_bits

    net = edge_value_network()
    assert {0.0, 1.0, EPS0, EPS1} <= set(net.probs.tolist())
    states = all_states(net.n_nodes)
    got = host_unstable(net, states, graph)
    assert np.array_equal(got, np_tt_unstable_words(net, states, graph))
    # stated once more without the comparisons of the restatement: on the entries themselves
    bits = unpack_bits(states, net.n_nodes).astype(np.int64)
    moves = unpack_bits(got, net.n_nodes)
    seen = set()
    for i in range(1 if graph == "step" else 0, net.n_nodes):
        ins = net.inputs[int(net.input_offsets[i]):int(net.input_offsets[i + 1])]
        code = np.zeros(len(bits), dtype=np.int64)
        for j in ins:
            code = 2 * code + bits[:, int(j)]
        p = net.probs[int(net.thr_offsets[i]):int(net.thr_offsets[i + 1])][code]
        for value, up, down in ((0.0, 0, 1), (1.0, 1, 0), (EPS0, 1, 1), (EPS1, 1, 1), (0.5, 1, 1)):
            sel = p == value
            if sel.any():
                seen.add(value)
                assert (moves[sel & (bits[:, i] == 0), i] == up).all()
                assert (moves[sel & (bits[:, i] == 1), i] == down).all()
    assert seen == {0.0, 1.0, EPS0, EPS1, 0.5}
    if graph == "step":
        assert not moves[:, 0].any()


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("n_total", [64, 65])
def test_host_rule_embedded_across_the_word_boundary(n_total, graph):
    """The edge-value network inside 64 / 65 nodes, its nodes ending at bit 63 / straddling bits 63 and 64."""
    from gym_pbn_amd.attractors import host_unstable

    small = edge_value_network()
    n = small.n_nodes
    place = list(range(n_total - n, n_total))
    big = embed_tt_network(small, n_total, place)
    frozen = np.random.default_rng(5).integers(0, 2, size=n_total, dtype=np.uint8)
    states = lift_states(all_states(n), n, n_total, place, frozen)
    got = host_unstable(big, states, graph)
    assert np.array_equal(got, np_tt_unstable_words(big, states, graph))
    # and it is the small network's "stg" answer moved to the new positions: frozen nodes never flip, and the
    # small network's node 0 is not the big one's, so it moves in both graphs
    want = lift_states(np_tt_unstable_words(small, all_states(n), "stg"), n, n_total, place, np.zeros(n_total, np.uint8))
    assert np.array_equal(got, want)


def test_host_rule_predictor_mix():
    """Predictor-mix networks have one graph: ``pbn_net_unstable`` gives the predictor rule, whatever the code."""
    import test_attractors_host as H
    from gym_pbn_amd import _lib as L
    from gym_pbn_amd.attractors import host_unstable
    from gym_pbn_amd.batch import Net

    c = H.CASES[3]
    net = H.case_network(c)
    states = all_states(c["n_nodes"])
    want = np_unstable_words(net, states)
    assert np.array_equal(host_unstable(net, states), want)
    assert np.array_equal(host_unstable(net, states, "step"), want)
    h = Net(net)
    out = np.empty_like(states)
    assert L.lib.pbn_net_unstable(h.handle, 77, L.ptr(states, L._u64p), len(states), L.ptr(out, L._u64p)) == 0
    assert np.array_equal(out, want)


def test_host_rule_refusals():
    from gym_pbn_amd import _lib as L
    from gym_pbn_amd.attractors import host_unstable
    from gym_pbn_amd.batch import Net

    c = CASES[0]
    net = Net(case_network(c))
    states = all_states(c["n_nodes"])
    out = np.empty_like(states)
    for bad in (0, 3, -1):  # a truth-table network has no default graph
        assert L.lib.pbn_net_unstable(net.handle, bad, L.ptr(states, L._u64p), len(states), L.ptr(out, L._u64p)) \
            == L.PBN_E_INVALID
        assert "PBN_TABLE_GRAPH" in L.last_error()
    assert L.lib.pbn_net_unstable(net.handle, L.TABLE_GRAPH_STG, None, 1, L.ptr(out, L._u64p)) == L.PBN_E_INVALID
    with pytest.raises(ValueError):
        host_unstable(net, states)
    with pytest.raises(ValueError):
        host_unstable(net, states, "sync")


def test_side_by_side_copies_have_product_graphs():
    """The 72-node network of the GPU tests, on the host: at a product of the copies' fixed points nothing moves
    under ``"stg"``; under ``"step"`` the same holds with copy 0 taken from its step graph."""
    from gym_pbn_amd.attractors import host_unstable

    c = case_by(12, 3, 0.47, 8)
    big = copies_network(c, 6)
    assert (big.n_nodes, big.n_words) == (72, 2)
    for graph in GRAPHS:  # only global node 0 is frozen by "step": copy 0 alone takes its step graph
        parts = [np.concatenate(expected_attractors(c, graph))] + [np.concatenate(expected_attractors(c, "stg"))] * 5
        fixed = product_states(parts, 12)
        assert len(fixed) == {"stg": 729, "step": 972}[graph] == len(np.unique(fixed, axis=0))
        assert not host_unstable(big, fixed, graph).any()
    # a step-graph fixed point of copy 0 that is none of the stg graph does move under "stg"
    only_step = [a for a in expected_attractors(c, "step")
                 if not any(np.array_equal(a, b) for b in expected_attractors(c, "stg"))]
    assert only_step
    s = product_states([only_step[0]] + [expected_attractors(c, "stg")[0]] * 5, 12)
    assert host_unstable(big, s, "stg").tolist() == [[1, 0]]  # node 0, and nothing else
    assert not host_unstable(big, s, "step").any()


# ---------------------------------------------------------------- the form the envs take
def test_states_lists_round_trip():
    from gym_pbn_amd.attractors import AttractorResult

    c = case_by(10, 3, 0.40, 7)
    res = AttractorResult(c["n_nodes"], attractors=expected_attractors(c, "stg"), seed_counts=[1])
    lists = res.states_lists()
    assert len(lists) == 1 and len(lists[0]) == 32
    assert all(isinstance(s, tuple) and len(s) == 10 and all(type(v) is int for v in s) for s in lists[0])
    assert {frozenset(a) for a in lists} == {frozenset(tuple(s) for s in a) for a in c["attractors"]}
    assert AttractorResult(10).states_lists() == []


# ---------------------------------------------------------------- the opt-in switch
class _Called(Exception):
    pass


GOAL = {"target_nodes": {(0,) * 8}, "all_attractors": None, "target": None}


def test_find_is_opt_in_for_the_truth_table_envs(monkeypatch):
    from gym_pbn_amd import attractors, envs

    calls = []

    def fake(network, **kw):
        calls.append(kw)
        raise _Called

    monkeypatch.setattr(attractors, "find_attractors", fake)
    data = case_pbn_data(case_by(8, 3, 0.47, 8))
    given = [[(0,) * 8], [(0, 1, 0, 1, 0, 1, 0, 1)]]
    for make in (lambda v: envs.PBNEnv(PBN_data=data, goal_config=GOAL, all_attractors=v),
                 lambda v: envs.VecPBNEnv(PBN_data=data, goal_config=GOAL, n_envs=4, all_attractors=v)):
        n = len(calls)
        with pytest.raises(_Called):
            make("find")
        assert len(calls) == n + 1 and calls[-1]["table_graph"] == "stg"
        for v in (None, given):  # the full STG, or the list as given: no discovery
            try:
                env = make(v)
            except attractors.L.PbnError as e:  # no device on this machine: the batch behind the env
                assert "HIP" in str(e)
                env = None
            assert len(calls) == n + 1
            if env is not None and v is given:
                assert env.all_attractors == [set(a) for a in given]


def test_find_switch_reports_what_was_not_enumerated(monkeypatch):
    """``RuntimeError`` when nothing was enumerated, a warning for incomplete closures, ``ValueError`` past
    2^16 states."""
    from gym_pbn_amd import attractors
    from gym_pbn_amd.attractors import AttractorResult, find_state_attractors

    c = case_by(10, 3, 0.40, 7)
    att = expected_attractors(c, "stg")
    entry = {"seed": att[0][0], "n_seen": 5, "hull": ("*",) * 10, "n_seeds": 3}
    results = iter([AttractorResult(10, incomplete=[entry]),
                    AttractorResult(10, attractors=att, seed_counts=[1], incomplete=[entry]),
                    AttractorResult(17, attractors=[np.arange((1 << 16) + 1, dtype=np.uint64).reshape(-1, 1)],
                                    seed_counts=[1])])
    monkeypatch.setattr(attractors, "find_attractors", lambda network, **kw: next(results))
    with pytest.raises(RuntimeError, match="no attractor"):
        find_state_attractors(None)
    with pytest.warns(UserWarning, match="3 seed"):
        got = find_state_attractors(None)
    assert {frozenset(a) for a in got} == {frozenset(tuple(s) for s in a) for a in c["attractors"]}
    with pytest.raises(ValueError, match="65537 states"):
        find_state_attractors(None)
