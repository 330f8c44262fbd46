"""State census: exact visit counts of full states, collected on the device (``pbn_census_*``, ``csrc/pbn_census.hip``).

The reference's ``statistical_attractors`` (``pbn_target.py:538-560``, ``pbn_target_multi.py:465-487``) runs 100 resets of
1,000 steps, increments a ``defaultdict(int)`` keyed by the full state tuple before every step, and keeps the
most-visited states. A :class:`StateCensus` is that dict as a device table: every env of a :class:`PBNBatch` walks
``n_updates`` updates in one launch and counts the state it is in at the sample points, one ``uint64`` count per
distinct packed state. :func:`compute_ssd_hist`-style histograms count a projection onto ~20 target genes; this counts
the whole state (or any node subset, ``nodes=``), for ``N`` up to 512.

Everything is integer work: with ``dropped == 0`` the counts are exactly what looping ``step(1)`` + ``get_state()`` and
``np.unique`` on the host gives.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterable, Optional

import numpy as np

from . import _lib as L
from .batch import Net, PBNBatch, unpack_bits


def _order(states: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """Row order: count descending, then the state as an integer ascending (word ``W-1`` most significant)."""
    keys = tuple(states[:, k] for k in range(states.shape[1])) + (-counts.astype(np.int64),)
    return np.lexsort(keys)


@dataclass
class CensusResult:
    """What a census holds: ``states`` ``[S][W]`` uint64 and ``counts`` ``[S]`` uint64, sorted by count descending,
    then by state ascending (as integers, word ``W-1`` most significant), so ties have one order. ``visits``: sample
    points counted in all; ``dropped``: those whose state was absent and could not be inserted. ``sum(counts) + dropped
    == visits``; with ``dropped == 0`` every count is exact, otherwise every count is a lower bound."""

    n_nodes: int
    states: np.ndarray
    counts: np.ndarray
    visits: int = 0
    dropped: int = 0

    def __post_init__(self):
        W = (int(self.n_nodes) + 63) // 64
        s = np.ascontiguousarray(self.states, dtype=np.uint64).reshape(-1, W)
        c = np.ascontiguousarray(self.counts, dtype=np.uint64).reshape(-1)
        if len(s) != len(c):
            raise ValueError(f"{len(c)} counts for {len(s)} states")
        o = _order(s, c)
        self.states, self.counts = s[o], c[o]

    def __len__(self) -> int:
        return len(self.counts)

    @property
    def exact(self) -> bool:
        return self.dropped == 0

    def top(self, k: int) -> "CensusResult":
        """The ``k`` most visited states (all of them if fewer are held); ``visits`` and ``dropped`` are kept."""
        k = max(int(k), 0)
        return CensusResult(self.n_nodes, self.states[:k], self.counts[:k], self.visits, self.dropped)

    def frequencies(self) -> np.ndarray:
        """``counts / (visits - dropped)``: the share of the counted visits. With ``dropped > 0`` this is an
        estimate (the dropped visits belong to states that may or may not be held); see :attr:`exact`."""
        n = self.visits - self.dropped
        return self.counts.astype(np.float64) / n if n > 0 else np.zeros(len(self.counts))

    def states_lists(self) -> list:
        """The states as tuples of ints, node 0 first, in rank order: the form ``PBNEnv`` keeps states in."""
        return [tuple(int(v) for v in row) for row in unpack_bits(self.states, self.n_nodes)]

    def state_set(self, k: Optional[int] = None, device: Optional[int] = 0):
        """A :class:`gym_pbn_amd.stateset.StateSet` of the ``k`` most visited states (``None``: all), each labelled
        by its rank: what ``TorchVecPBNTargetMultiSetEnv(attractors=...)`` and ``PBNBatch.classify_host`` take."""
        from .stateset import StateSet

        rows = self.states if k is None else self.states[: max(int(k), 0)]
        return StateSet(rows, self.n_nodes, labels=np.arange(len(rows), dtype=np.int32), device=device)


class StateCensus:
    """``StateCensus(network_or_n_nodes, max_states=1 << 22, device=0)``: a device table of visit counts.

    ``max_states``: distinct states the table can hold (up to ``2**24``). A visit of a state that is absent when the
    table is full is counted in ``dropped``, never silently lost. ``device=None``: a host-only handle (argument checks
    only; :meth:`run` is refused with ``PBN_E_STATE``). One census is fed by one batch at a time.
    """

    def __init__(self, network_or_n_nodes, max_states: int = 1 << 22, device: Optional[int] = 0):
        if isinstance(network_or_n_nodes, (int, np.integer)):
            self.n_nodes = int(network_or_n_nodes)
        elif isinstance(network_or_n_nodes, Net):
            self.n_nodes = network_or_n_nodes.n_nodes
        elif isinstance(network_or_n_nodes, (str, bytes)) or hasattr(network_or_n_nodes, "__fspath__"):
            from .network import load_network

            self.n_nodes = load_network(network_or_n_nodes).n_nodes
        else:
            self.n_nodes = int(network_or_n_nodes.n_nodes)
        self.n_words = (self.n_nodes + 63) // 64
        self.device = None if device is None else int(device)
        h = C.c_void_p()
        L.check(L.lib.pbn_census_create(self.n_nodes, -1 if device is None else int(device), int(max_states),
                                        C.byref(h)))
        self._h = h

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(L, "lib", None) is not None:
            L.lib.pbn_census_destroy(h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def node_mask(self, nodes: Iterable[int]) -> np.ndarray:
        """The projection mask ``[W]`` of an iterable of node indices."""
        m = np.zeros(self.n_words, dtype=np.uint64)
        for i in nodes:
            i = int(i)
            if not 0 <= i < self.n_nodes:
                raise ValueError(f"node {i} outside [0, {self.n_nodes - 1}]")
            m[i // 64] |= np.uint64(1) << np.uint64(i % 64)
        return m

    def run(self, batch: PBNBatch, n_updates: int, first: int = 0, stride: int = 1, nodes=None):
        """Every env of ``batch`` makes ``n_updates`` updates (the draws ``batch.step`` would make: afterwards the
        batch is where ``step(n_updates)`` leaves it) and counts "the state after ``i`` updates" for ``i = first,
        first + stride, ... <= n_updates``; ``first=0`` counts the state before the call. ``nodes``: count the
        projection onto these nodes only. One launch, asynchronous; at most 65,536 updates per call."""
        for name, v in (("n_updates", n_updates), ("first", first), ("stride", stride)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError(f"{name}={v} outside [0, 2^32)")
        mask = None if nodes is None else self.node_mask(nodes)
        L.check(L.lib.pbn_census_run_device(batch.handle, self._h, int(n_updates), int(first), int(stride),
                                            L.ptr(mask, L._u64p)))

    def clear(self):
        L.check(L.lib.pbn_census_clear(self._h))

    def info(self) -> dict:
        i = L.CensusInfo()
        L.check(L.lib.pbn_census_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in L.CensusInfo._fields_}

    def adds(self) -> int:
        """Count adds issued since the last clear (measurement): ``adds / visits`` is the share of sample points that
        touched memory; the rest extended a lane's run of equal consecutive keys in registers."""
        n = C.c_uint64(0)
        L.check(L.lib.pbn_census_get_stats(self._h, C.byref(n), None))
        return int(n.value)

    def entries(self) -> int:
        """Entries taken from the end of the key array since the last clear (measurement): the states held plus the
        entries lanes took in vain when they lost a publish race -- at most one per lane of a launch, and handed out
        again by later launches."""
        n = C.c_uint64(0)
        L.check(L.lib.pbn_census_get_stats(self._h, None, C.byref(n)))
        return int(n.value)

    def result(self) -> CensusResult:
        n = C.c_uint64(0)
        L.check(L.lib.pbn_census_read(self._h, None, None, 0, C.byref(n)))
        cap = max(int(n.value), 1)
        s = np.empty((cap, self.n_words), dtype=np.uint64)
        c = np.empty(cap, dtype=np.uint64)
        L.check(L.lib.pbn_census_read(self._h, L.ptr(s, L._u64p), L.ptr(c, L._u64p), cap, C.byref(n)))
        i = self.info()
        return CensusResult(self.n_nodes, s[: n.value], c[: n.value], int(i["visits"]), int(i["dropped"]))


def statistical_attractors(network, k: int = 4, resets: int = 100, steps: int = 1000, seed: int = 0,
                           device: int = 0) -> list:
    """The reference's ``statistical_attractors`` (``pbn_target.py:538-560``, ``pbn_target_multi.py:465-487``) in
    one launch: ``resets`` envs, the state counted before each of ``steps`` steps, the ``k`` most visited states
    returned as tuples of ints (node 0 first), most visited first.

    Two deviations from the reference:

    * Its ``reset()`` draws from ``all_attractors`` -- the very thing this function is meant to find, which is why the
      reference never calls it. The start here is the uniform random state of ``genRandState`` / ``PBN.reset(None)``
      (``PBNBatch.randomize``).
    * Ties in the visit count are broken by state order (the state as an integer, ascending), not by the insertion
      order of a Python dict.
    """
    net = network if isinstance(network, Net) else Net(network)
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be at least 1")
    b = PBNBatch(net, int(resets), device=device, seed=seed)
    c = StateCensus(net, max_states=min(L.CENSUS_MAX_STATES, max(int(resets) * steps, 1)), device=device)
    try:
        b.randomize()
        done, first = 0, 0  # states 0 .. steps - 1 are counted: the start, then the state after each update but the last
        while True:
            n = min(steps - 1 - done, L.CENSUS_MAX_UPDATES)
            c.run(b, n, first=first)
            done += n
            first = 1  # a later call's "state as loaded" was the earlier call's last sample
            if done >= steps - 1:
                break
        return c.result().top(k).states_lists()
    finally:
        c.close()
        b.close()


__all__ = ["StateCensus", "CensusResult", "statistical_attractors"]
