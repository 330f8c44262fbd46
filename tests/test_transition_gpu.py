"""The exact transition graph on the device (``k_stg_rows``, ``csrc/pbn_stg.hip``; ``gym_pbn_amd.transition``).

The integer arrays are checked bit for bit: ``mass`` against ``host_edge_mass`` (itself pinned against numpy and the
reference in ``test_transition_host.py``) and ``succ`` against a Python dict of the rows. The float64 methods are
checked against numpy on the same integer arrays within rounding bounds derived where they are used, and the
production stream's law against the exact masses.
"""

import math

import numpy as np
import pytest

from shape_cases import tt_net
from test_attractors_host import all_states, case_id, case_network, embed_network, lift_states
from test_transition_host import EMBED_TOTALS, GRAPHS, TWO53, case_by, random_words

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


# ---------------------------------------------------------------- helpers
def np_succ(states, mass):
    """``[S][N]`` int32 from a dict of the rows: the neighbour's row where ``mass > 0`` (-1: not a row), the row
    itself where ``mass == 0``. Only cells with mass are looked up."""
    states = np.ascontiguousarray(states, dtype=np.uint64)
    index = {row.tobytes(): r for r, row in enumerate(states)}
    assert len(index) == len(states)
    out = np.repeat(np.arange(len(states), dtype=np.int32)[:, None], mass.shape[1], axis=1)
    for s, i in zip(*np.nonzero(mass)):
        t = states[s].copy()
        t[i // 64] ^= np.uint64(1) << np.uint64(i % 64)
        out[s, i] = index.get(t.tobytes(), -1)
    return out


def check_rows(net, states, graph=None, device_graph=None):
    """``rows()`` of the whole set against the host statements; returns ``(graph, mass, succ)`` as numpy."""
    from gym_pbn_amd.transition import TransitionGraph, host_edge_mass

    g = device_graph if device_graph is not None else TransitionGraph(net, states, table_graph=graph)
    import torch

    mass, succ = g.rows()
    assert mass.dtype == torch.int64 and succ.dtype == torch.int32 and mass.is_cuda and succ.is_cuda
    assert tuple(mass.shape) == tuple(succ.shape) == (len(states), g.n_nodes)
    m, t = mass.cpu().numpy(), succ.cpu().numpy()
    want_m = host_edge_mass(g.net, states, graph)
    assert np.array_equal(m.astype(np.uint64), want_m)
    want_t = np_succ(states, want_m)
    assert np.array_equal(t, want_t)
    return g, want_m, want_t


def ball(seed_row, n_nodes, first):
    """The seed and every state one or two flips of nodes ``first .. N-1`` away, as packed rows, seed first."""
    W = (n_nodes + 63) // 64
    rows = [np.asarray(seed_row, np.uint64).reshape(W).copy()]
    bit = lambda i: (i // 64, np.uint64(1) << np.uint64(i % 64))  # noqa: E731
    for i in range(first, n_nodes):
        a = rows[0].copy()
        a[bit(i)[0]] ^= bit(i)[1]
        rows.append(a)
        for j in range(i + 1, n_nodes):
            b = a.copy()
            b[bit(j)[0]] ^= bit(j)[1]
            rows.append(b)
    return np.stack(rows)


_B28 = {}


def bittner28_attractor_120():
    """The 120-state attractor of Bittner-28 from ``find_attractors``, found once for the module."""
    if "res" not in _B28:
        from gym_pbn_amd.attractors import find_attractors

        _B28["res"] = find_attractors("bittner28", n_seeds=256, max_states=1 << 17, seed=1)
    res = _B28["res"]
    k = [len(a) for a in res.attractors].index(120)
    return res, k


# ---------------------------------------------------------------- rows() against the host statements
@pytest.mark.parametrize("c", [case_by(8, 2, 6), case_by(12, 3, 1)], ids=case_id)
def test_rows_full_space_of_a_golden_net(c):
    """All ``2**N`` states: closed, so no leak; N = 12 is 49,152 cells, 192 workgroups."""
    net = case_network(c)
    g, m, t = check_rows(net, all_states(c["n_nodes"]))
    assert g.leaks == 0 and g.closed and (t >= 0).all()
    assert (m == 0).any() and (m == TWO53).any() and ((m > 0) & (m < TWO53)).any()
    assert np.array_equal(g.mass.cpu().numpy().astype(np.uint64), m) and np.array_equal(g.succ.cpu().numpy(), t)


def test_rows_walk_the_grid_stride_loop(monkeypatch):
    """Three workgroups over 49,152 cells (PBNSIM_STG_GRID): every lane walks 64 cells."""
    monkeypatch.setenv("PBNSIM_STG_GRID", "3")
    c = case_by(12, 3, 1)
    g, _, _ = check_rows(case_network(c), all_states(12))
    assert g.leaks == 0


def test_rows_bittner28_attractor():
    res, k = bittner28_attractor_120()
    g, m, t = check_rows(res.network, res.attractors[k], device_graph=res.transition_graph(k))
    assert len(g) == 120 and g.closed and g.leaks == 0 and (t >= 0).all()
    # an attractor is strongly connected and has more than one state: every state has a way out
    assert ((m > 0).sum(axis=1) >= 1).all()


@pytest.mark.parametrize("graph", GRAPHS)
def test_rows_truth_table_ball(graph):
    """``tt_net(64)``: every table entry lies inside (0, 1), so the closure of any state is the whole space. The set
    here is the start of that closure -- a state and everything within two flips of it, 2,081 rows under "stg" and
    2,017 under "step" -- and the edges that leave it are leaks, counted against numpy."""
    net = tt_net(64)
    first = 1 if graph == "step" else 0
    states = ball(random_words(64, 1, 9)[0], 64, first)
    assert len(states) == 1 + (64 - first) + (64 - first) * (63 - first) // 2
    g, m, t = check_rows(net, states, graph)
    assert g.first_node == first and g.n_movable == 64 - first
    assert (m[:, 0] == 0).all() == (graph == "step")
    assert g.leaks == int((t < 0).sum()) > 0 and not g.closed
    assert (t[0] >= 0).all()  # the seed's neighbours are all rows


@pytest.mark.parametrize("graph", GRAPHS)
def test_rows_truth_table_closed_space(graph):
    """A truth-table fixture net's full space (tables with entries 0 and 1 among them): closed under both graphs."""
    import test_attractors_tt_host as T

    c = T.CASES[0]
    net = T.case_network(c)
    g, m, t = check_rows(net, all_states(c["n_nodes"]), graph)
    assert g.leaks == 0 and g.closed and (t >= 0).all()


@pytest.mark.parametrize("n_total", EMBED_TOTALS)
def test_rows_embedded_across_the_word_boundary(n_total):
    """The golden N = 10 net at the top of 64 / 65 / ... / 512 nodes, every W = 1 .. 8: the 1,024 lifted states are
    closed (frozen nodes never move), and the graph is the small net's at the moved positions."""
    small = case_network(case_by(10, 2, 0))
    place = list(range(n_total - 10, n_total))
    big = embed_network(small, n_total, place)
    frozen = np.random.default_rng(5).integers(0, 2, size=n_total, dtype=np.uint8)
    states = lift_states(all_states(10), 10, n_total, place, frozen)
    g, m, t = check_rows(big, states)
    assert g.n_words == (n_total + 63) // 64 and g.leaks == 0
    from gym_pbn_amd.transition import host_edge_mass

    sm = host_edge_mass(small, all_states(10))
    assert np.array_equal(m[:, place], sm) and int(m.sum(dtype=np.uint64)) == int(sm.sum(dtype=np.uint64))
    assert np.array_equal(t[:, place], np_succ(all_states(10), sm))


# ---------------------------------------------------------------- leaks and chunks
def test_leaks_of_a_set_with_one_state_removed():
    from gym_pbn_amd.transition import TransitionGraph

    c = case_by(10, 2, 0)
    net = case_network(c)
    states = np.delete(all_states(10), 517, axis=0)
    g, m, t = check_rows(net, states)
    n_leaks = int((t < 0).sum())
    assert n_leaks > 0 and g.leaks == n_leaks and not g.closed
    assert np.array_equal(np.argwhere(g.succ.cpu().numpy() < 0), np.argwhere(t < 0))
    # every leak points at the missing state
    for s, i in np.argwhere(t < 0):
        assert int(states[s, 0]) ^ (1 << int(i)) == 517
    v = np.arange(len(states), dtype=np.float64)
    for call in (lambda: g.pull(v), lambda: g.push(v), g.stationary):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert isinstance(g, TransitionGraph)


@pytest.mark.parametrize("S", [1, 65, 257])
def test_rows_in_chunks(S):
    """``rows(0, S)`` equals the chunks of 1, 63 and the rest put together, and each call adds its leaks."""
    import torch
    from gym_pbn_amd.transition import TransitionGraph

    net = case_network(case_by(10, 2, 0))
    states = all_states(10)[np.random.default_rng(S).permutation(1024)[:S]]
    g = TransitionGraph(net, states)
    mass, succ = g.rows(0, S)
    n_leaks = int((succ < 0).sum())
    assert g.info()["leaks"] == n_leaks
    cuts = [0, min(1, S), min(64, S), S]
    parts = [g.rows(a, b) for a, b in zip(cuts, cuts[1:])]
    assert [tuple(p[0].shape) for p in parts] == [(b - a, 10) for a, b in zip(cuts, cuts[1:])]
    assert torch.equal(torch.cat([p[0] for p in parts]), mass) and torch.equal(torch.cat([p[1] for p in parts]), succ)
    assert g.info()["leaks"] == 2 * n_leaks
    assert g.leaks == n_leaks  # the whole graph's own count does not see the earlier calls
    with pytest.raises(ValueError):
        g.rows(0, S + 1)


# ---------------------------------------------------------------- float64 on the integer arrays
def np_probabilities(m, n_movable):
    return m.astype(np.float64) / float(TWO53 * n_movable)


def np_pull(m, t, n_movable, v):
    p = np_probabilities(m, n_movable)
    return (p * v[t]).sum(axis=1) + (1.0 - p.sum(axis=1)) * v


def np_push(m, t, n_movable, d):
    p = np_probabilities(m, n_movable)
    out = (1.0 - p.sum(axis=1)) * d
    np.add.at(out, t.reshape(-1), (p * d[:, None]).reshape(-1))
    return out


def test_pull_and_push_against_numpy():
    """Both sides evaluate the same real number per element from the same doubles ``p`` (one IEEE division each, so
    equal) and ``v``: a sum of at most ``N + 1`` products whose weights ``p_i`` and ``stay`` add up to 1. Each
    side's error is at most ``(N + 3) u max|v|`` (``u = 2**-53``: one rounding per product, ``N`` additions in any
    order, the two roundings of ``stay = 1 - sum p``), so the two differ by at most ``(N + 3) * 2**-52 * max|v|``.
    For ``push`` an element collects at most ``N`` incoming flips (its ``N`` neighbours) and its own stay term, each
    at most ``max|d| / n_movable`` resp. ``max|d|``: the same count of operations and the same bound with ``max|d|``.
    The total mass: ``sum_t out[t]`` is ``sum_s d[s] (sum_i p[s][i] + stay[s])``, whose bracket is 1 within
    ``(N + 3) u``, and the element errors add up to at most ``(N + 3) u sum|d|`` more: ``|sum out - sum d| <=
    (N + 3) * 2**-52 * sum|d|``, both sums taken exactly (``math.fsum``)."""
    c = case_by(12, 3, 1)
    net = case_network(c)
    g, m, t = check_rows(net, all_states(12))
    N, S = 12, 4096
    rng = np.random.default_rng(0)
    p = g.probabilities().cpu().numpy()
    assert p.dtype == np.float64 and np.array_equal(p, np_probabilities(m, 12))
    v = rng.normal(size=S) * 1e3
    got = g.pull(v).cpu().numpy()
    assert got.dtype == np.float64
    dev = np.abs(got - np_pull(m, t, 12, v)).max()
    bound = (N + 3) * 2.0 ** -52 * np.abs(v).max()
    print(f"pull: largest deviation {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound
    assert np.array_equal(g.pull(np.ones(S)).cpu().numpy().round(12), np.ones(S))  # rows are distributions
    d = rng.random(S)
    d /= d.sum()
    out = g.push(d).cpu().numpy()
    dev = np.abs(out - np_push(m, t, 12, d)).max()
    bound = (N + 3) * 2.0 ** -52 * d.max()
    print(f"push: largest deviation {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound and (out >= 0).all()
    drift = abs(math.fsum(out) - math.fsum(d))
    print(f"push: total mass drift {drift:.3e}, bound {(N + 3) * 2.0 ** -52 * math.fsum(d):.3e}")
    assert drift <= (N + 3) * 2.0 ** -52 * math.fsum(np.abs(d))
    # pull and push are adjoint: <push(d), v> == <d, pull(v)> up to the same roundings
    lhs, rhs = math.fsum(out * v), math.fsum(d * got)
    assert abs(lhs - rhs) <= 4 * (N + 3) * 2.0 ** -52 * np.abs(v).max()


def test_stationary_inside_the_bittner28_attractor():
    """``pi > 0`` everywhere (an attractor is irreducible). Each push moves the total mass by at most ``(N + 3) *
    2**-52`` of it (above), the uniform start is 1 within ``S u``: ``|sum pi - 1| <= (iters (N + 3) 2 + S) u``.
    ``||push(pi) - pi||_1`` recomputed in numpy: a push is an L1 contraction, so it is at most the last change
    ``residual <= tol``, plus what numpy's push and torch's differ by, ``S (N + 3) 2**-52 max(pi)``."""
    res, k = bittner28_attractor_120()
    g = res.transition_graph(k)
    tol = 1e-12
    pi, residual, iters = g.stationary(tol=tol)
    print(f"stationary: {iters} pushes, residual {residual:.3e}")
    assert iters < 100000 and residual <= tol
    pi = pi.cpu().numpy()
    N, S = 28, 120
    assert pi.shape == (S,) and (pi > 0).all()
    assert abs(math.fsum(pi) - 1.0) <= (2 * iters * (N + 3) + S) * U
    m, t = g.mass.cpu().numpy().astype(np.uint64), g.succ.cpu().numpy()
    again = np.abs(np_push(m, t, 28, pi) - pi).sum()
    print(f"stationary: ||push(pi) - pi||_1 in numpy {again:.3e}")
    assert again <= tol + S * (N + 3) * 2.0 ** -52 * pi.max()
    # and it is not the uniform distribution it started from
    assert pi.max() / pi.min() > 1.5


# ---------------------------------------------------------------- the law of the production stream
def check_stream_law(net, states, nodes, graph, pmax, seed):
    """Every (state, node) cell in ``n = 4,096`` envs, one ``step_forced`` launch: the flip count of a cell with mass
    0 or ``2**53`` is exact; every other cell's lies within ``6 sqrt(n p (1 - p)) + 1 + n pmax 2**-32`` of ``n p``,
    ``p = mass / 2**53`` (the last term: the 32-bit grid of the Philox choice word, one grid step per threshold)."""
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.transition import host_edge_mass

    n = 4096
    S, K, W = len(states), len(nodes), net.n_words
    mass = host_edge_mass(net, states, graph)[:, nodes]
    before = np.repeat(states, K * n, axis=0)  # env (s, k, e) = (s * K + k) * n + e
    forced = np.tile(np.repeat(np.asarray(nodes, np.uint32), n), S)
    b = PBNBatch(net, S * K * n, seed=seed)
    b.set_state(before)
    b.step_forced(forced[None])
    after = b.get_state()
    b.close()
    diff = (before ^ after).reshape(S, K, n, W)
    nodes = np.asarray(nodes)
    own = (diff[:, np.arange(K), :, nodes // 64].transpose(1, 0, 2) >> (nodes % 64).astype(np.uint64)[None, :, None]) & np.uint64(1)
    counts = own.sum(axis=2).astype(np.int64)
    # nothing but the forced node moved
    own_bit = np.zeros((K, W), dtype=np.uint64)
    own_bit[np.arange(K), nodes // 64] = np.uint64(1) << (nodes % 64).astype(np.uint64)
    assert not (diff & ~own_bit[None, :, None, :]).any()
    p = mass.astype(np.float64) / TWO53
    exact0, exact1 = mass == 0, mass == TWO53
    assert (counts[exact0] == 0).all() and (counts[exact1] == n).all()
    band = 6.0 * np.sqrt(n * p * (1.0 - p)) + 1.0 + n * pmax * 2.0 ** -32
    dev = np.abs(counts - n * p)
    mid = ~(exact0 | exact1)
    print(f"stream law: {S * K} cells ({int(mid.sum())} inside (0, 1)), largest |count - n p| / band "
          f"{(dev[mid] / band[mid]).max():.3f}")
    assert mid.any() and (dev[mid] <= band[mid]).all()
    return counts


def test_stream_law_bittner199():
    """8 random states x 199 nodes x 4,096 envs = 6.5 M envs. At 1,592 cells the 6 sigma band leaves a false-alarm
    chance below 1e-5, and the fixed seed makes the run reproducible."""
    from gym_pbn_amd.network import load_network

    net = load_network("bittner199")
    pmax = int(np.diff(net.pred_offsets).max())
    check_stream_law(net, random_words(199, 8, 21), list(range(199)), None, pmax, seed=12345)


def test_stream_law_truth_table():
    """``tt_net(64)``, 2 states, the nodes ``PBN.step`` can update (1 .. 63; one threshold per entry: pmax 1)."""
    check_stream_law(tt_net(64), random_words(64, 2, 22), list(range(1, 64)), "step", 1, seed=54321)
