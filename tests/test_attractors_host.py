"""Attractor discovery, host side: the cube cover, the edge rule restated in numpy, the opt-in switch.

The numpy restatement of the support-graph edge rule lives here (``np_unstable``): node ``i`` can
flip at ``x`` iff a live predictor of node ``i`` outputs ``1 - x_i`` at ``x``, a predictor being live
iff its selection interval on the 53-bit grid is non-empty. The GPU tests import it as the
independent statement the kernels are checked against.
"""

import json

import numpy as np
import pytest

from conftest import GOLDEN

TWO53 = 1 << 53


# ---------------------------------------------------------------- fixtures and helpers
def golden_cases():
    return json.loads((GOLDEN / "attractors_small.json").read_text())["cases"]


def case_id(c):
    return f"N{c['n_nodes']}-p{c['max_preds']}-s{c['seed']}"


CASES = golden_cases()


def case_network(c):
    from gym_pbn_amd.network import PredictorNetwork

    sets = []
    for node in c["predictor_sets"]:
        ps = np.empty((3, len(node)), dtype=object)
        for q, (cod, A, ids) in enumerate(node):
            ps[0, q] = float(cod)
            ps[1, q] = np.asarray(A, dtype=np.float64).reshape(-1, 1)
            ps[2, q] = [int(v) for v in ids]
        sets.append(ps)
    return PredictorNetwork.from_predictor_sets(sets, list(range(c["n_nodes"])), name=case_id(c))


def case_attractors(c):
    """Golden attractors as sorted packed arrays ``[S][1]``, in the fixture's order."""
    from gym_pbn_amd.attractors import sort_rows
    from gym_pbn_amd.batch import pack_bits

    return [sort_rows(pack_bits(np.asarray(a, dtype=np.uint8))) for a in c["attractors"]]


def all_states(n):
    return np.arange(1 << n, dtype=np.uint64).reshape(-1, 1)


def np_unstable(net, bits):
    """``[S][N]`` bool: node i can flip at state s (bits ``[S][N]`` 0/1)."""
    bits = np.asarray(bits, dtype=np.uint8)
    out = np.zeros(bits.shape, dtype=bool)
    for i in range(net.n_nodes):
        o0, o1 = int(net.pred_offsets[i]), int(net.pred_offsets[i + 1])
        prev = 0
        xi = bits[:, i]
        for j in range(o0, o1):
            t = min(int(net.pred_thr[j]), TWO53) if j < o1 - 1 else TWO53
            live = t > prev
            prev = max(prev, t)
            if not live:
                continue
            a, b, c = (int(v) for v in net.pred_inputs[j])
            p = (bits[:, a] << 3) | (bits[:, b] << 2) | (bits[:, c] << 1) | xi
            table = np.array([(int(net.pred_tt[j]) >> k) & 1 for k in range(16)], dtype=np.uint8)
            out[:, i] |= table[p] != xi
    return out


def np_unstable_words(net, words):
    from gym_pbn_amd.batch import pack_bits, unpack_bits

    return pack_bits(np_unstable(net, unpack_bits(words, net.n_nodes)).astype(np.uint8))


def np_successors(net, words):
    """Edges of the support graph out of packed ``words``: (source row index, successor words)."""
    from gym_pbn_amd.batch import unpack_bits

    s_idx, i_idx = np.nonzero(np_unstable(net, unpack_bits(words, net.n_nodes)))
    succ = words[s_idx].copy()
    succ[np.arange(len(s_idx)), i_idx // 64] ^= np.uint64(1) << (i_idx % 64).astype(np.uint64)
    return s_idx, succ


def np_closure(net, seed_words):
    """Everything ``seed_words`` reach, breadth first, as sorted packed rows."""
    from gym_pbn_amd.attractors import rows_in, sort_rows

    seen = np.unique(np.asarray(seed_words, np.uint64).reshape(-1, net.n_words), axis=0)
    frontier = seen
    while len(frontier):
        _, succ = np_successors(net, frontier)
        succ = np.unique(succ, axis=0)
        frontier = succ[~rows_in(succ, seen)]
        seen = np.concatenate([seen, frontier])
    return sort_rows(seen)


def np_attractors(net):
    """Terminal strongly connected components over all 2^N states (N small), sorted packed arrays."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    from gym_pbn_amd.attractors import sort_rows

    n = 1 << net.n_nodes
    src, succ = np_successors(net, all_states(net.n_nodes))
    dst = succ[:, 0].astype(np.int64)
    g = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n)).tocsr()
    n_comp, label = connected_components(g, directed=True, connection="strong")
    leaves = np.ones(n_comp, dtype=bool)
    leaves[label[src][label[src] != label[dst]]] = False
    out = [sort_rows(np.flatnonzero(label == k).astype(np.uint64).reshape(-1, 1)) for k in np.flatnonzero(leaves)]
    return sorted(out, key=lambda a: (len(a), int(a[0, 0])))


def embed_network(net, n_total, place, name="embedded"):
    """``net``'s nodes placed at positions ``place`` of an ``n_total``-node network; every other node is
    frozen by a single self-copy predictor (truth table 0xAAAA: output = own value)."""
    from gym_pbn_amd.network import PredictorNetwork

    place = [int(p) for p in place]
    at = {p: i for i, p in enumerate(place)}
    offs, inputs, n_in, tts, thrs = [0], [], [], [], []
    for v in range(n_total):
        if v in at:
            i = at[v]
            for j in range(int(net.pred_offsets[i]), int(net.pred_offsets[i + 1])):
                inputs.append([place[int(x)] for x in net.pred_inputs[j]])
                n_in.append(int(net.pred_n_inputs[j]))
                tts.append(int(net.pred_tt[j]))
                thrs.append(int(net.pred_thr[j]))
        else:
            inputs.append([v, v, v])
            n_in.append(1)
            tts.append(0xAAAA)
            thrs.append(TWO53)
        offs.append(len(tts))
    P = len(tts)
    out = PredictorNetwork(
        node_ids=np.arange(n_total, dtype=np.int64), pred_offsets=np.asarray(offs, np.int32),
        pred_inputs=np.asarray(inputs, np.int32).reshape(-1, 3), pred_n_inputs=np.asarray(n_in, np.int32),
        pred_tt=np.asarray(tts, np.uint16), pred_thr=np.asarray(thrs, np.uint64), pred_cod=np.ones(P),
        pred_cumcod=np.ones(P), pred_A=np.zeros((P, 4)), node_codsum=np.ones(n_total), name=name)
    out.validate()
    return out


def lift_states(words, n_small, n_total, place, frozen_bits):
    """Packed states of the small network placed into the big layout (other nodes = ``frozen_bits``)."""
    from gym_pbn_amd.batch import pack_bits, unpack_bits

    small = unpack_bits(words, n_small)
    big = np.repeat(np.asarray(frozen_bits, np.uint8)[None], len(small), axis=0)
    big[:, np.asarray(place)] = small
    assert big.shape[1] == n_total
    return pack_bits(big)


# ---------------------------------------------------------------- the cube cover
def check_cover(states, n_nodes):
    from gym_pbn_amd.attractors import cube_cover, expand_cubes, sort_rows

    cubes = cube_cover(states, n_nodes)
    expanded = expand_cubes(cubes, n_nodes)
    assert len(expanded) == len(states), "cubes overlap or miss states"  # disjoint: no state twice
    assert len(np.unique(expanded, axis=0)) == len(expanded)
    assert np.array_equal(sort_rows(expanded), sort_rows(states))
    return cubes


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_cube_cover_of_golden_attractors(c):
    for a in case_attractors(c):
        cubes = check_cover(a, c["n_nodes"])
        if len(a) & (len(a) - 1):  # not a power of two: cannot be one cube
            assert len(cubes) > 1


def test_cube_cover_of_a_cube_minus_one_state():
    n = 70  # two words; the free nodes straddle the word boundary
    free = [3, 62, 63, 64, 65, 69]
    from gym_pbn_amd.attractors import cube_cover, expand_cubes

    full = expand_cubes([tuple("*" if i in free else (i % 2) for i in range(n))], n)
    assert len(full) == 64
    assert len(check_cover(full, n)) == 1
    states = np.delete(full, 37, axis=0)
    cubes = check_cover(states, n)
    assert len(cubes) == len(free)  # a 2^k cube minus a point splits into k cubes
    with pytest.raises(ValueError):
        cube_cover(states, n, max_cubes=len(free) - 1)


def test_all_attractors_form():
    from gym_pbn_amd.attractors import AttractorResult, expand_cubes, sort_rows

    c = CASES[0]
    res = AttractorResult(c["n_nodes"], attractors=case_attractors(c), seed_counts=[1, 1])
    out = res.all_attractors()
    assert len(out) == 2 and all(isinstance(cube, tuple) and len(cube) == c["n_nodes"] for a in out for cube in a)
    for cubes, a in zip(out, res.attractors):
        assert np.array_equal(sort_rows(expand_cubes(cubes, c["n_nodes"])), a)
    with pytest.raises(ValueError):
        res.all_attractors(max_cubes=0)


# ---------------------------------------------------------------- the edge rule
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_numpy_edge_rule_reproduces_golden_attractors(c):
    net = case_network(c)
    got = np_attractors(net)
    want = sorted(case_attractors(c), key=lambda a: (len(a), int(a[0, 0])))
    assert [len(a) for a in got] == [len(a) for a in want]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert (1 << c["n_nodes"]) - sum(len(a) for a in got) == c["n_transient"]
    # a closure from inside an attractor is that attractor
    assert np.array_equal(np_closure(net, want[-1][:1]), want[-1])


def test_dead_predictor_is_no_edge():
    """A predictor whose 53-bit interval is empty adds no edge, whatever it outputs."""
    net = case_network(CASES[0])
    i = next(k for k in range(net.n_nodes) if net.pred_offsets[k + 1] - net.pred_offsets[k] == 2)
    j = int(net.pred_offsets[i])
    bits = np.asarray(np.unravel_index(np.arange(1 << net.n_nodes), (2,) * net.n_nodes)).T
    before = np_unstable(net, bits)
    net.pred_thr[j] = 0  # predictor j is never selected: only predictor j + 1 counts
    net.pred_tt[j] = ~net.pred_tt[j]
    only_second = np_unstable(net, bits)
    xi = bits[:, i]
    a, b, c = (int(v) for v in net.pred_inputs[j + 1])
    p = (bits[:, a] << 3) | (bits[:, b] << 2) | (bits[:, c] << 1) | xi
    assert np.array_equal(only_second[:, i], ((int(net.pred_tt[j + 1]) >> p.astype(np.int64)) & 1) != xi)
    assert np.array_equal(np.delete(only_second, i, axis=1), np.delete(before, i, axis=1))


# ---------------------------------------------------------------- the opt-in switch
class _Called(Exception):
    pass


def test_find_is_opt_in(monkeypatch):
    from gym_pbn_amd import attractors, envs, registry

    calls = []

    def fake(network, **kw):
        calls.append(kw)
        raise _Called

    monkeypatch.setattr(attractors, "find_attractors", fake)
    for make in (lambda v: registry.make("gym-PBN/BittnerMulti-28-v0", all_attractors=v),
                 lambda v: registry.make("gym-PBN/Bittner-28-v0", all_attractors=v),
                 lambda v: registry.make("gym-PBN/BittnerMultiGeneral-v0", all_attractors=v),
                 lambda v: envs.PBNTargetMultiEnv("bittner28", all_attractors=v)):
        n = len(calls)
        with pytest.raises(_Called):
            make("find")
        assert len(calls) == n + 1
        with pytest.raises(ValueError, match="all_attractors is required"):
            make(None)
        assert len(calls) == n + 1
    assert attractors.resolve_all_attractors("bittner28", [[(0,) * 28]]) == [[(0,) * 28]]
