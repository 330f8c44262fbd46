"""Attractor discovery for predictor-mix (Bittner) and truth-table networks, on the device.

The reference gets ``all_attractors`` from the external ``cabean`` binary
(``get_attractors_from_cabean.py:39-54``); its own exhaustive route
(``Graph.genSTG`` + ``findAttractors``, ``base.py:199-242, 398-399``) enumerates all
``2**N`` states. Here attractors are found by reachability from simulated states:
settle a batch with the rollout kernel, then enumerate the attractor each state
landed in with the device state set of ``pbn_reach_*`` (``csrc/pbn_reach.hip``).

**Support graph.** State ``x`` has an edge to ``x ^ (1 << i)`` iff node ``i`` *can* flip
at ``x``: some *live* predictor of node ``i`` outputs ``1 - x_i`` there. A predictor is
live iff its selection interval on the **53-bit grid** is non-empty -- the widths
:meth:`PredictorNetwork.update_probability` computes, the last threshold taken as
``2**53``. This is the support of the reference's law (``getNextStates`` keeps an edge
when ``prob > 0``); it is deliberately *not* defined on the 32-bit grid of the Philox
choice word, so a predictor narrower than ``2**-32`` still counts.

**Truth-table networks** (``common/pbn.py`` ``PBN``) have two support graphs, and the caller
names one (``table_graph``). In both, node ``i`` can flip at ``x`` iff its table entry ``p`` at
``x`` lets it leave ``x_i``: ``p > 0`` from 0, ``p < 1`` from 1 -- evaluated on the 53-bit
threshold ``T = ceil(p * 2**53)`` as ``T > 0`` / ``T < 2**53``, which is the same test exactly
(a double ``p > 0`` has ``T >= 1``; a double ``p < 1`` has ``p * 2**53 <= 2**53 - 1``).

* ``"stg"``: every node may move. This is ``PBN._compute_next_states``' async branch
  (``pbn.py:186-199``), the graph behind ``PBNEnv.compute_attractors`` and
  :func:`gym_pbn_amd.stg.compute_attractors`: the drop-in ``all_attractors``, without the
  ``2**N`` enumeration (:mod:`gym_pbn_amd.stg` stops at 22 nodes).
* ``"step"``: nodes ``1..N-1`` only, the graph ``PBN.step`` walks (``randint(1, N-1)``; ``reset``
  clears node 0): where the simulation can end up.

The two differ on almost every network, so :class:`ReachSet` has no default between them.

**Attractor.** A terminal strongly connected component of the support graph, the same
object as ``nx.attracting_components`` on the reference's STG.

**What is exact and what is sampled.** Everything reported under ``attractors`` is
exactly an attractor: its closure was enumerated to the fixed point and every state of
it reaches every other. *Coverage* depends on the seeds: an attractor no seed reaches is
not reported. A closure that does not fit ``max_states`` is reported under
``incomplete`` with the hull cube of the states seen -- never guessed at.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib as L
from .batch import Net, PBNBatch, unpack_bits
from .network import KIND_PROB_TABLE

MAX_ENV_CUBES = 4096  # pbn_envcfg_create's limit on cubes
MAX_ENV_STATES = 1 << 16  # PBNEnv / VecPBNEnv keep their attractors as Python sets of state tuples
TABLE_GRAPHS = {"stg": L.TABLE_GRAPH_STG, "step": L.TABLE_GRAPH_STEP}


class ReachSet:
    """The device state set of one network (``pbn_reach_*``): closure, backward marks, read-back.

    ``table_graph``: the support graph of a truth-table network, ``"stg"`` or ``"step"`` (module
    docstring). ``None`` with a truth-table network is refused (``PBN_E_UNSUPPORTED``): neither
    graph is a default. A predictor-mix network has one graph and takes no ``table_graph``.
    """

    def __init__(self, net, max_states: int = 1 << 22, device: int = 0, table_graph: Optional[str] = None):
        if table_graph is not None and table_graph not in TABLE_GRAPHS:
            raise ValueError(f"table_graph={table_graph!r}: expected one of {sorted(TABLE_GRAPHS)} or None")
        self.net = net if isinstance(net, Net) else Net(net)
        self.n_nodes, self.n_words = self.net.n_nodes, self.net.n_words
        self.table_graph = table_graph
        h = C.c_void_p()
        if table_graph is None:
            L.check(L.lib.pbn_reach_create(self.net.handle, int(device), int(max_states), C.byref(h)))
        else:
            if self.net.kind != KIND_PROB_TABLE:
                raise ValueError("table_graph applies to truth-table networks; a predictor-mix network has one graph")
            L.check(L.lib.pbn_reach_create_table(self.net.handle, int(device), int(max_states),
                                                 TABLE_GRAPHS[table_graph], C.byref(h)))
        self._h = h

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(L, "lib", None) is not None:
            L.lib.pbn_reach_destroy(h)
            self._h = None

    __del__ = close

    def _words(self, states):
        w = np.ascontiguousarray(states, dtype=np.uint64)
        return w.reshape(-1, self.n_words)

    def info(self) -> dict:
        i = L.ReachInfo()
        L.check(L.lib.pbn_reach_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in L.ReachInfo._fields_}

    def unstable(self, states) -> np.ndarray:
        """Masks ``[S][W]`` of the nodes that can flip at each of ``states`` ``[S][W]``."""
        w = self._words(states)
        out = np.empty_like(w)
        L.check(L.lib.pbn_reach_unstable(self._h, L.ptr(w, L._u64p), w.shape[0], L.ptr(out, L._u64p)))
        return out

    def closure(self, seeds):
        """Clear the set, insert ``seeds`` and expand to the fixed point: ``(count, complete)``."""
        w = self._words(seeds)
        n, ok = C.c_uint64(0), C.c_int32(0)
        L.check(L.lib.pbn_reach_closure(self._h, L.ptr(w, L._u64p), w.shape[0], C.byref(n), C.byref(ok)))
        return int(n.value), bool(ok.value)

    def mark_backward(self, state) -> int:
        """Mark every state of the set that reaches ``state`` inside the set; returns how many."""
        w = self._words(state)
        if w.shape[0] != 1:
            raise ValueError("mark_backward takes one state")
        n = C.c_uint64(0)
        L.check(L.lib.pbn_reach_mark_backward(self._h, L.ptr(w, L._u64p), C.byref(n)))
        return int(n.value)

    def read(self):
        """``(states [n][W], marks [n])``, in an order that stays fixed until the next closure."""
        n = C.c_uint64(0)
        L.check(L.lib.pbn_reach_read(self._h, None, None, 0, C.byref(n)))
        cap = max(int(n.value), 1)
        s = np.empty((cap, self.n_words), dtype=np.uint64)
        m = np.empty(cap, dtype=np.uint32)
        L.check(L.lib.pbn_reach_read(self._h, L.ptr(s, L._u64p), L.ptr(m, L._u32p), cap, C.byref(n)))
        return s[: n.value], m[: n.value]

    def hull(self):
        """``(all, any)`` ``[W]``: AND / OR over the states of the set."""
        a = np.empty(self.n_words, dtype=np.uint64)
        o = np.empty(self.n_words, dtype=np.uint64)
        L.check(L.lib.pbn_reach_hull(self._h, L.ptr(a, L._u64p), L.ptr(o, L._u64p)))
        return a, o


def host_unstable(net, states, table_graph: Optional[str] = None) -> np.ndarray:
    """:meth:`ReachSet.unstable` without a device (``pbn_net_unstable``): the same rule definition the
    kernels evaluate, run over the host copy of the network image. ``table_graph`` is required for a
    truth-table network and ignored for a predictor-mix one."""
    net = net if isinstance(net, Net) else Net(net)
    graph = 0
    if net.kind == KIND_PROB_TABLE:
        if table_graph not in TABLE_GRAPHS:
            raise ValueError(f"table_graph={table_graph!r}: expected one of {sorted(TABLE_GRAPHS)}")
        graph = TABLE_GRAPHS[table_graph]
    w = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, net.n_words)
    out = np.empty_like(w)
    L.check(L.lib.pbn_net_unstable(net.handle, graph, L.ptr(w, L._u64p), w.shape[0], L.ptr(out, L._u64p)))
    return out


def host_edge_mass(net, states, table_graph: Optional[str] = None) -> np.ndarray:
    """The law behind :func:`host_unstable`'s support (``pbn_net_edge_mass``, ``csrc/pbn_mass_rule.hpp``; module
    :mod:`gym_pbn_amd.transition`): the edge masses ``[S][N]`` uint64 of packed ``states`` ``[S][W]``, each an integer
    in ``[0, 2**53]`` -- in units of ``2**-53`` the probability that node ``i`` flips given that it is the node updated.
    The same rule definition ``k_stg_rows`` evaluates, run over the host copy of the network image; ``mass > 0``
    exactly where :func:`host_unstable` sets the bit. ``table_graph`` is required for a truth-table network
    (``"step"``: node 0 has mass 0) and ignored for a predictor-mix one."""
    net = net if isinstance(net, Net) else Net(net)
    graph = 0
    if net.kind == KIND_PROB_TABLE:
        if table_graph not in TABLE_GRAPHS:
            raise ValueError(f"table_graph={table_graph!r}: expected one of {sorted(TABLE_GRAPHS)}")
        graph = TABLE_GRAPHS[table_graph]
    w = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, net.n_words)
    out = np.empty((w.shape[0], net.n_nodes), dtype=np.uint64)
    L.check(L.lib.pbn_net_edge_mass(net.handle, graph, L.ptr(w, L._u64p), w.shape[0], L.ptr(out, L._u64p)))
    return out


# ---------------------------------------------------------------- host helpers
def sort_rows(words: np.ndarray) -> np.ndarray:
    """Rows ``[S][W]`` sorted as integers (word ``W-1`` most significant)."""
    words = np.asarray(words, dtype=np.uint64)
    return words[np.lexsort(tuple(words[:, k] for k in range(words.shape[1])))]


def _row_keys(words: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return w.view([("", np.uint64)] * w.shape[1]).reshape(-1)


def rows_in(rows: np.ndarray, table: np.ndarray) -> np.ndarray:
    """Boolean ``[S]``: is ``rows[k]`` a row of ``table``."""
    if len(table) == 0 or len(rows) == 0:
        return np.zeros(len(rows), dtype=bool)
    return np.isin(_row_keys(rows), _row_keys(table))


def hull_cube(all_words, any_words, n_nodes: int) -> tuple:
    """The smallest cube holding a set, from its AND / OR words: ints where fixed, ``'*'`` elsewhere."""
    a = unpack_bits(np.asarray(all_words, np.uint64), n_nodes)
    o = unpack_bits(np.asarray(any_words, np.uint64), n_nodes)
    return tuple(int(x) if x == y else "*" for x, y in zip(a, o))


def cube_cover(states, n_nodes: int, max_cubes: Optional[int] = None) -> List[tuple]:
    """An exact, disjoint cover of packed ``states`` ``[S][W]`` (distinct rows) by hypercubes.

    Recursive split on a varying bit; a sub-set that fills its whole sub-cube becomes one
    cube with ``'*'`` on the varying nodes. Raises ``ValueError`` past ``max_cubes``.
    """
    words = np.ascontiguousarray(states, dtype=np.uint64).reshape(len(states), -1)
    if len(words) == 0:
        return []
    out: List[tuple] = []
    stack = [words]
    while stack:
        w = stack.pop()
        all_w = np.bitwise_and.reduce(w, axis=0)
        any_w = np.bitwise_or.reduce(w, axis=0)
        vary = unpack_bits(all_w ^ any_w, n_nodes)
        k = int(vary.sum())
        if k < 64 and len(w) == 1 << k:  # distinct rows inside a 2^k cube: they fill it
            out.append(hull_cube(all_w, any_w, n_nodes))
            if max_cubes is not None and len(out) > max_cubes:
                raise ValueError(f"the attractor needs more than {max_cubes} cubes")
            continue
        i = int(np.argmax(vary))  # the lowest varying node
        bit = (w[:, i // 64] >> np.uint64(i % 64)) & np.uint64(1)
        stack.append(w[bit == 1])
        stack.append(w[bit == 0])
    return out


def expand_cubes(cubes, n_nodes: int) -> np.ndarray:
    """Packed states ``[S][W]`` of a list of cubes (every ``'*'`` expanded), in cube order."""
    from .batch import pack_bits

    rows = []
    for c in cubes:
        free = [i for i, x in enumerate(c) if x == "*"]
        base = np.array([0 if x == "*" else int(x) for x in c], dtype=np.uint8)
        m = np.repeat(base[None], 1 << len(free), axis=0)
        idx = np.arange(1 << len(free))
        for j, i in enumerate(free):
            m[:, i] = (idx >> j) & 1
        rows.append(pack_bits(m))
    W = (n_nodes + 63) // 64
    return np.concatenate(rows) if rows else np.zeros((0, W), np.uint64)


@dataclass
class AttractorResult:
    """Result of :func:`find_attractors`.

    ``attractors``: packed ``[S_k][W]`` arrays, rows sorted as integers, ordered by (size, smallest
    state). ``seed_counts[k]``: seeds that ended in attractor k (a seed that reaches several is
    counted for one of them). ``incomplete``: closures that did not fit ``max_states``, as dicts
    ``{"seed", "n_seen", "hull", "n_seeds"}`` (``hull``: the cube of the states seen). ``network`` / ``table_graph``:
    what the attractors were found on (``None`` for a result built by hand), for :meth:`transition_graph`.
    """

    n_nodes: int
    attractors: List[np.ndarray] = field(default_factory=list)
    seed_counts: List[int] = field(default_factory=list)
    incomplete: List[dict] = field(default_factory=list)
    network: object = None  # the Net the attractors were found on, and its table graph (find_attractors sets both)
    table_graph: Optional[str] = None

    def all_attractors(self, max_cubes: int = MAX_ENV_CUBES) -> list:
        """The reference's ``all_attractors``: per attractor a list of cube tuples (ints / ``'*'``),
        an exact disjoint cover. Raises ``ValueError`` if one attractor needs more than ``max_cubes``
        cubes (``pbn_envcfg_create`` accepts 4,096)."""
        return [cube_cover(a, self.n_nodes, max_cubes) for a in self.attractors]

    def states_lists(self) -> list:
        """Per attractor the list of its states as tuples of ints, node 0 first, in the arrays' order:
        the form ``PBNEnv`` / ``VecPBNEnv`` take as ``all_attractors``."""
        return [[tuple(int(v) for v in row) for row in unpack_bits(a, self.n_nodes)] for a in self.attractors]

    def state_set(self, device: Optional[int] = 0):
        """One labelled :class:`gym_pbn_amd.stateset.StateSet` of every found attractor, label = the attractor's
        index: ``np.bincount(batch.classify_host(s) + 1)`` over a settled batch is the landing histogram
        (bin 0: envs in no found attractor). ``device=None``: the host copy only."""
        from .stateset import StateSet

        W = (self.n_nodes + 63) // 64
        rows = np.concatenate(self.attractors) if self.attractors else np.zeros((0, W), np.uint64)
        labels = np.concatenate([np.full(len(a), j, np.int32) for j, a in enumerate(self.attractors)]) \
            if self.attractors else np.zeros(0, np.int32)
        return StateSet(rows, self.n_nodes, labels=labels, device=device)

    def occupancy(self, census_result):
        """Where the mass of a :class:`gym_pbn_amd.census.CensusResult` goes: ``(per_attractor, outside)`` --
        ``per_attractor[k]`` the visits counted on states of attractor k, ``outside`` those on states of no found
        attractor (``dropped`` visits are in neither; ``per_attractor.sum() + outside + dropped == visits``). Host
        lookup of the census' states in :meth:`state_set`."""
        labels = self.state_set(device=None).lookup(census_result.states)
        counts = np.asarray(census_result.counts, dtype=np.uint64)
        per = np.zeros(len(self.attractors), dtype=np.uint64)
        np.add.at(per, labels[labels >= 0], counts[labels >= 0])
        return per, int(counts[labels < 0].sum())

    def transition_graph(self, k: int, device: Optional[int] = 0, network=None):
        """The exact weighted graph of attractor ``k`` (:class:`gym_pbn_amd.transition.TransitionGraph`): closed, so
        ``stationary()`` is the distribution inside it. The network is the one :func:`find_attractors` ran on, or
        ``network`` for a result built by hand."""
        from .transition import TransitionGraph

        net = self.network if network is None else network
        if net is None:
            raise ValueError("this AttractorResult carries no network: pass network=")
        return TransitionGraph(net, self.attractors[k], table_graph=self.table_graph, device=device)


def _known(found, s) -> int:
    """Index of the found attractor holding state ``s``, or -1. Attractors are disjoint, so one state decides."""
    s = np.asarray(s, np.uint64).reshape(1, -1)
    for j, f in enumerate(found):
        if (f == s).all(axis=1).any():  # one pass, no sort of a 2^21-row table
            return j
    return -1


def _descend(work: ReachSet, s: np.ndarray, found=()):
    """From seed ``s`` down to an attractor: ``(j, None)`` if the descent enters ``found[j]``,
    ``(states, None)`` for a new attractor, or ``(None, (n_seen, all, any))`` when a closure did
    not fit. Each round's closure is strictly inside the previous one."""
    while True:
        j = _known(found, s)
        if j >= 0:
            return j, None
        n, complete = work.closure(s)
        if not complete:
            return None, (n,) + work.hull()
        if work.mark_backward(s) == n:  # everything s reaches reaches s back: closed and strongly connected
            return sort_rows(work.read()[0]), None
        states, marks = work.read()
        s = states[np.flatnonzero(marks == 0)[0]]


def find_attractors(network, n_seeds: int = 4096, burn_in: Optional[int] = None, max_states: int = 1 << 22,
                    seed: int = 0, device: int = 0, states=None, table_graph: str = "stg") -> AttractorResult:
    """Attractors of a network reached from simulated (or given) states.

    ``table_graph`` names the support graph of a truth-table network (``"stg"``: the graph of
    ``PBNEnv.compute_attractors``; ``"step"``: the graph ``PBN.step`` walks, node 0 frozen); it is
    ignored for a predictor-mix network, which has one graph. The simulation of a truth-table network
    clears node 0 and never updates it, so sampled seeds all have ``x_0 = 0``: under ``"stg"`` an attractor
    that only states with ``x_0 = 1`` reach is found from ``states=`` alone.

    Seeds are ``PBNBatch.randomize()`` + ``rollout(burn_in)`` (default ``1024 * N`` updates) of
    ``n_seeds`` envs, or ``states`` (packed ``[S][W]``; no burn-in). Duplicate seeds and seeds
    inside a found attractor are dropped; from each remaining seed ``s``: ``F = closure(s)``; if it
    does not fit ``max_states`` it is recorded under ``incomplete``; else ``B = mark_backward(s)``;
    ``|B| == |F|`` makes ``F`` an attractor, otherwise an unmarked state is the next ``s``.
    A descent that enters an attractor already found ends there, so every attractor is listed once
    and its seeds are counted together.
    When the closure of all seeds together fits, one backward marking per attractor assigns
    every seed that reaches it at once (a second set holds that closure).

    Membership is exact, coverage is sampled: every array under ``attractors`` is exactly an
    attractor of the support graph (defined on the 53-bit selection thresholds, see the module
    docstring, or on the 53-bit table thresholds); attractors that no seed reaches are missing.
    """
    net = network if isinstance(network, Net) else Net(network)
    N, W = net.n_nodes, net.n_words
    graph = table_graph if net.kind == KIND_PROB_TABLE else None
    if net.kind == KIND_PROB_TABLE and graph not in TABLE_GRAPHS:
        raise ValueError(f"table_graph={table_graph!r}: expected one of {sorted(TABLE_GRAPHS)}")
    work = ReachSet(net, max_states, device, table_graph=graph)
    if states is None:
        b = PBNBatch(net, int(n_seeds), device=device, seed=seed)
        b.randomize()
        b.rollout(1024 * N if burn_in is None else int(burn_in))
        seeds = b.get_state()
        b.close()
    else:
        seeds = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, W)
    uniq, mult = np.unique(seeds, axis=0, return_counts=True)
    owner = np.full(len(uniq), -1, dtype=np.int64)  # attractor of each distinct seed; -2 = incomplete
    found: List[np.ndarray] = []
    res = AttractorResult(N, network=net, table_graph=graph)

    def note_incomplete(k, info):
        n_seen, all_w, any_w = info
        cube = hull_cube(all_w, any_w, N)
        owner[k] = -2
        for e in res.incomplete:
            if e["hull"] == cube:
                e["n_seeds"] += int(mult[k])
                e["n_seen"] = max(e["n_seen"], n_seen)
                return
        res.incomplete.append({"seed": uniq[k].copy(), "n_seen": n_seen, "hull": cube, "n_seeds": int(mult[k])})

    basin = None
    try:
        if len(uniq) > 1:
            basin = ReachSet(net, max_states, device, table_graph=graph)
            if not basin.closure(uniq)[1]:
                basin.close()
                basin = None
        if basin is not None:
            # every seed's closure lies inside the joint one, so every descent completes; a seed still without
            # an owner reaches none of the attractors found so far, so its descent ends in a new one
            pos = None
            while (owner == -1).any():
                k = int(np.flatnonzero(owner == -1)[0])
                att, info = _descend(work, uniq[k])
                if att is None:  # not expected inside a joint closure that fitted; reported all the same
                    note_incomplete(k, info)
                    continue
                found.append(att)
                basin.mark_backward(att[0])
                u_states, u_marks = basin.read()
                if pos is None:  # row of each seed in the joint closure (the read-back order is fixed)
                    order = np.argsort(_row_keys(u_states))
                    pos = order[np.searchsorted(_row_keys(u_states)[order], _row_keys(uniq))]
                owner[(owner == -1) & (u_marks[pos] != 0)] = len(found) - 1
        else:
            for k in range(len(uniq)):
                if owner[k] != -1:
                    continue
                att, info = _descend(work, uniq[k], found)  # may end in an attractor already found
                if att is None:
                    note_incomplete(k, info)
                elif isinstance(att, int):
                    owner[k] = att
                else:
                    found.append(att)
                    owner[k] = len(found) - 1
                    owner[(owner == -1) & rows_in(uniq, att)] = len(found) - 1
    finally:
        work.close()
        if basin is not None:
            basin.close()

    order = sorted(range(len(found)), key=lambda j: (len(found[j]), tuple(int(v) for v in found[j][0][::-1])))
    res.attractors = [found[j] for j in order]
    res.seed_counts = [int(mult[owner == j].sum()) for j in order]
    return res


def resolve_all_attractors(network, all_attractors, device: int = 0, seed: int = 0):
    """``all_attractors="find"`` -> the cube lists of :func:`find_attractors` (opt-in); anything
    else is returned as given."""
    if not (isinstance(all_attractors, str) and all_attractors == "find"):
        return all_attractors
    res = find_attractors(network, device=device, seed=seed)
    if not res.attractors:
        raise RuntimeError(
            f"no attractor fits the state set: {len(res.incomplete)} closure(s) ran past max_states "
            "(networks with N >= 149 are not enumerable this way)")
    if res.incomplete:
        import warnings

        warnings.warn(f"{sum(e['n_seeds'] for e in res.incomplete)} seed(s) ended in closures past max_states; "
                      "the env uses the attractors that were enumerated")
    return res.all_attractors()


def find_state_attractors(network, device: int = 0, seed: int = 0) -> list:
    """``all_attractors="find"`` of ``PBNEnv`` / ``VecPBNEnv``: the attractors of a truth-table network's
    ``"stg"`` graph (what :func:`gym_pbn_amd.stg.compute_attractors` enumerates ``2**N`` states for), found by
    :func:`find_attractors` and expanded to lists of state tuples. Raises ``RuntimeError`` if nothing was
    enumerated, ``ValueError`` past ``MAX_ENV_STATES`` states in all; warns when some closures were incomplete."""
    res = find_attractors(network, device=device, seed=seed, table_graph="stg")
    if not res.attractors:
        raise RuntimeError(f"no attractor fits the state set: {len(res.incomplete)} closure(s) ran past max_states")
    if res.incomplete:
        import warnings

        warnings.warn(f"{sum(e['n_seeds'] for e in res.incomplete)} seed(s) ended in closures past max_states; "
                      "the env uses the attractors that were enumerated")
    total = sum(len(a) for a in res.attractors)
    if total > MAX_ENV_STATES:
        raise ValueError(f"the attractors hold {total} states; the env keeps them as Python sets and takes at most "
                         f"{MAX_ENV_STATES}")
    return res.states_lists()


__all__ = ["ReachSet", "AttractorResult", "host_unstable", "host_edge_mass", "find_attractors", "cube_cover", "expand_cubes", "hull_cube", "rows_in",
           "sort_rows", "resolve_all_attractors", "find_state_attractors", "MAX_ENV_CUBES", "MAX_ENV_STATES",
           "TABLE_GRAPHS"]
