"""The exact transition graph of an enumerated state set, on the device (``pbn_stg_*``, ``csrc/pbn_stg.hip``).

The reference states the law of the asynchronous update in three places: ``Graph.getNextStates``
(``bittner/base.py:221-242``: ``{next_state: prob}`` of one state; ``genSTG`` builds the weighted graph from it),
``PBN._compute_next_states`` (``common/pbn.py:186-199``) and ``PBCN._async_compute_next_states``
(``common/pbcn.py:72-93``) for truth tables. All three loop over ``2**N`` states in Python. A :class:`TransitionGraph`
is that object for a set somebody already enumerated -- an attractor of :func:`gym_pbn_amd.attractors.find_attractors`,
a closure, the states of a census -- as two dense device arrays filled in one launch per row chunk:

* ``mass[s][i]``: the **edge mass**, an integer in ``[0, 2**53]``: in units of ``2**-53`` the probability that node
  ``i`` takes the value ``1 - x_i`` at state ``s`` given that node ``i`` is the one updated. Predictor mix: the summed
  widths of the selection intervals, on the 53-bit grid, of the live predictors that output ``1 - x_i`` (the
  arithmetic of :meth:`PredictorNetwork.update_probability`). Truth tables: with ``T = ceil(p * 2**53)`` the entry's
  threshold, ``T`` from 0 and ``2**53 - T`` from 1. One definition for host and device, ``csrc/pbn_mass_rule.hpp``.
* ``succ[s][i]``: the row of ``x_s ^ (1 << i)`` where ``mass > 0`` and that state is in the set; ``-1`` where
  ``mass > 0`` and it is not (a *leak*: the set is not closed); ``s`` itself where ``mass == 0``.

**Exact**: ``mass``, ``succ``, ``leaks``, ``closed`` -- integers, equal bit for bit to :func:`host_edge_mass` and a
host lookup. **Float64**: :meth:`TransitionGraph.probabilities`, :meth:`~TransitionGraph.pull`,
:meth:`~TransitionGraph.push`, :meth:`~TransitionGraph.stationary`, :meth:`~TransitionGraph.next_states` -- torch /
Python arithmetic on the integer arrays -- and :meth:`~TransitionGraph.expect`, ``pull`` as one fused kernel
(``csrc/pbn_control.hip``; what :mod:`gym_pbn_amd.control` iterates). :meth:`~TransitionGraph.row_of` names the row of
device state words.

**Node choice.** The probability of an edge is ``mass / (2**53 * n_movable)``: the updated node is drawn uniformly
from the movable nodes -- all ``N`` for a predictor-mix network (``Graph.step``'s ``randint(0, N-1)``,
``getNextStates``' ``1 / len(state)``), nodes ``1..N-1`` for ``table_graph="step"`` (``PBN.step``'s
``randint(1, N-1)``), all ``N`` for ``table_graph="stg"``. For ``"stg"`` that uniform choice is this library's: the
reference's async STG carries ``prob_true`` unnormalised.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from .attractors import TABLE_GRAPHS, host_edge_mass
from .batch import Net, pack_bits, unpack_bits
from .network import KIND_PROB_TABLE, TWO53


def _graph_code(net: Net, table_graph: Optional[str]) -> int:
    """``ReachSet``'s rules: a truth-table network names its graph, a predictor-mix network has one."""
    if net.kind == KIND_PROB_TABLE:
        if table_graph not in TABLE_GRAPHS:
            raise ValueError(f"table_graph={table_graph!r}: expected one of {sorted(TABLE_GRAPHS)}")
        return TABLE_GRAPHS[table_graph]
    if table_graph is not None:
        raise ValueError("table_graph applies to truth-table networks; a predictor-mix network has one graph")
    return 0


def _as_rows(states, n_nodes: int) -> np.ndarray:
    """Packed rows ``[S][W]`` uint64 from packed rows (a uint64 array) or from state tuples / bit rows ``[S][N]``."""
    W = (n_nodes + 63) // 64
    if isinstance(states, np.ndarray) and states.dtype == np.uint64:
        return np.ascontiguousarray(states).reshape(-1, W)
    bits = np.asarray(states)
    if bits.ndim != 2 or bits.shape[1] != n_nodes:
        raise ValueError(f"states: packed uint64 rows [S][{W}] or state tuples of {n_nodes} values")
    if bits.size and ((bits != 0) & (bits != 1)).any():
        raise ValueError("state tuples hold 0 / 1 values")
    return np.ascontiguousarray(pack_bits(bits.astype(np.uint8))).reshape(-1, W)


class TransitionGraph:
    """``TransitionGraph(network, states, table_graph=None, device=0)``: the weighted graph of ``states``.

    ``states``: packed rows ``[S][W]`` uint64 (e.g. one attractor of an ``AttractorResult``), or a list of state
    tuples (node 0 first); ``1 <= S <= 2**24``, rows distinct. Row ``s`` of every array is ``states[s]``.
    ``table_graph`` follows :class:`gym_pbn_amd.attractors.ReachSet`: ``"stg"`` or ``"step"`` for a truth-table
    network, nothing for a predictor-mix one. ``device=None``: a host-only handle -- :meth:`next_states` and
    :meth:`info` work, device calls are refused (``PBN_E_STATE``).
    """

    def __init__(self, network, states, table_graph: Optional[str] = None, device: Optional[int] = 0):
        self.net = network if isinstance(network, Net) else Net(network)
        self.n_nodes, self.n_words = self.net.n_nodes, self.net.n_words
        self.table_graph = table_graph
        self._graph = _graph_code(self.net, table_graph)
        self.states = _as_rows(states, self.n_nodes)
        self.n_states = int(self.states.shape[0])
        self.device = None if device is None else int(device)
        h = C.c_void_p()
        L.check(L.lib.pbn_stg_create(self.net.handle, -1 if device is None else int(device), self._graph,
                                     L.ptr(self.states if self.states.size else None, L._u64p), self.n_states,
                                     C.byref(h)))
        self._h = h
        i = self.info()
        self.first_node, self.n_movable = int(i["first_node"]), int(i["n_movable"])
        self._whole = None  # (mass, succ, leaks) of the whole graph, once asked for

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(L, "lib", None) is not None:
            L.lib.pbn_stg_destroy(h)
            self._h = None

    __del__ = close

    def __len__(self) -> int:
        return self.n_states

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        i = L.StgInfo()
        L.check(L.lib.pbn_stg_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in L.StgInfo._fields_}

    # ------------------------------------------------------------ the integer arrays
    def _fill(self, lo: int, hi: int, mass, succ):
        """Rows ``[lo, hi)`` into ``mass`` / ``succ`` (their rows 0 ..), at most ``2**31`` cells per launch."""
        import torch

        step = max(L.STG_MAX_CELLS // self.n_nodes, 1)
        # the library launches on the device's default stream: order it against torch's current one
        cur, dflt = torch.cuda.current_stream(mass.device), torch.cuda.default_stream(mass.device)
        if cur != dflt:
            dflt.wait_stream(cur)
        for a in range(lo, hi, step):
            n = min(step, hi - a)
            L.check(L.lib.pbn_stg_rows_device(self._h, a, n, C.c_void_p(mass[a - lo:].data_ptr()),
                                              C.c_void_p(succ[a - lo:].data_ptr())))
        if cur != dflt:
            cur.wait_stream(dflt)

    def rows(self, lo: int = 0, hi: Optional[int] = None):
        """``(mass, succ)`` of rows ``[lo, hi)``: device tensors int64 ``[n][N]`` and int32 ``[n][N]``. Every ``-1``
        written adds to the handle's leak counter (``info()["leaks"]``)."""
        import torch

        hi = self.n_states if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo <= hi <= self.n_states:
            raise ValueError(f"rows [{lo}, {hi}) outside [0, {self.n_states}]")
        if self.device is None:
            raise L.PbnError(L.PBN_E_STATE, "the transition graph is a host-only handle (device=None)")
        dev = torch.device("cuda", self.device)
        mass = torch.empty((hi - lo, self.n_nodes), dtype=torch.int64, device=dev)
        succ = torch.empty((hi - lo, self.n_nodes), dtype=torch.int32, device=dev)
        if hi > lo:
            self._fill(lo, hi, mass, succ)
        return mass, succ

    def _graph_arrays(self):
        if self._whole is None:
            L.check(L.lib.pbn_stg_clear_leaks(self._h))
            mass, succ = self.rows()
            self._whole = (mass, succ, int(self.info()["leaks"]))
        return self._whole

    @property
    def mass(self):
        """The whole graph's masses, int64 ``[S][N]`` on the device, computed once in row chunks."""
        return self._graph_arrays()[0]

    @property
    def succ(self):
        """The whole graph's successor rows, int32 ``[S][N]`` on the device (``-1``: a leak)."""
        return self._graph_arrays()[1]

    @property
    def leaks(self) -> int:
        """Edges of the whole graph that leave the set (the ``-1`` entries of :attr:`succ`)."""
        return self._graph_arrays()[2]

    @property
    def closed(self) -> bool:
        return self.leaks == 0

    # ------------------------------------------------------------ float64 on the integer arrays
    def probabilities(self):
        """float64 ``[S][N]`` on the device: ``mass / (2**53 * n_movable)``, the probability that the next update
        flips node ``i`` at row ``s``. The node choice is uniform over the movable nodes (``Graph.step`` /
        ``getNextStates``' ``1 / len(state)``; ``PBN.step``'s ``randint(1, N-1)``). For ``table_graph="stg"`` this
        uniform choice is ours: the reference's async STG carries ``prob_true`` unnormalised. One rounding per
        entry: the mass is an exact double (``<= 2**53``), the scaling by ``2**-53`` is exact, and the division by
        ``n_movable`` is an IEEE division -- by a device tensor, since torch turns a division by a Python scalar into
        a multiplication by its rounded reciprocal."""
        import torch

        m = self.mass
        n = torch.tensor(float(self.n_movable), dtype=torch.float64, device=m.device)
        return (m.to(torch.float64) * (1.0 / TWO53)) / n

    def _need_closed(self, what: str):
        if not self.closed:
            raise ValueError(f"{what} needs a closed set: {self.leaks} edge(s) leave it (succ == -1)")

    def pull(self, v):
        """``E[v(next) | s]`` for every row (the gather form; policy evaluation, the backup of value iteration):
        ``sum_i p[s][i] * v[succ[s][i]] + (1 - sum_i p[s][i]) * v[s]``. ``v``: ``[S]``, taken as float64 on the
        device. Raises ``ValueError`` unless the set is closed."""
        import torch

        self._need_closed("pull")
        p = self.probabilities()
        v = torch.as_tensor(v, dtype=torch.float64, device=p.device).reshape(self.n_states)
        return (p * v[self.succ.long()]).sum(dim=1) + (1.0 - p.sum(dim=1)) * v

    # ------------------------------------------------------------ fused kernels on the integer arrays (csrc/pbn_control.hip)
    def _on_default_stream(self, dev):
        """A context that orders the library's default-stream launches against torch's current stream, as
        :meth:`_fill` does, and makes the default stream torch's current one inside, so that torch ops between two
        launches (a sweep's ``h``) run in order with them."""
        import contextlib

        import torch

        @contextlib.contextmanager
        def ordered():
            cur, dflt = torch.cuda.current_stream(dev), torch.cuda.default_stream(dev)
            if cur == dflt:
                yield
                return
            dflt.wait_stream(cur)
            try:
                with torch.cuda.stream(dflt):
                    yield
            finally:
                cur.wait_stream(dflt)

        return ordered()

    def _expect_into(self, v, out, pen=None, cost: float = 0.0, out_pen=None):
        """``k_stg_expect`` on contiguous float64 device tensors ``[S]``; no checks, no ordering: the caller's."""
        mass, succ = self.mass, self.succ
        L.check(L.lib.pbn_stg_expect_device(self._h, mass.data_ptr(), succ.data_ptr(), v.data_ptr(), out.data_ptr(),
                                            None if pen is None else pen.data_ptr(), float(cost),
                                            None if out_pen is None else out_pen.data_ptr()))

    def expect(self, v, pen=None, cost: float = 0.0):
        """:meth:`pull` in one fused launch (``k_stg_expect``): ``v[s] + (sum_i mass[s][i] * (v[succ[s][i]] - v[s])) *
        2**-53 / n_movable``, read from the integer arrays in one pass with no ``[S][N]`` temporary. The same real
        number as :meth:`pull`, rounded differently (within ``(2 N + 8) * 2**-53 * max|v|`` of it); a constant comes
        back exactly; the result is bit-identical from call to call and under any grid. With ``pen`` ``[S]`` it
        returns ``(out, out - cost * pen)``, both written in the same pass. Raises ``ValueError`` unless the set is
        closed."""
        import torch

        self._need_closed("expect")
        dev = self.mass.device
        v = torch.as_tensor(v, dtype=torch.float64, device=dev).reshape(self.n_states).contiguous()
        out = torch.empty_like(v)
        out_pen = None
        if pen is not None:
            pen = torch.as_tensor(pen, dtype=torch.float64, device=dev).reshape(self.n_states).contiguous()
            out_pen = torch.empty_like(v)
        with self._on_default_stream(dev):
            self._expect_into(v, out, pen, cost, out_pen)
        return out if pen is None else (out, out_pen)

    def row_of(self, words):
        """The row of each state of ``words`` (device int64 ``[n][W]``, e.g. ``observation_words()`` of a device env):
        device int32 ``[n]``, ``-1`` for a state that is no row. One launch of the state set's lookup kernel over the
        graph's own table."""
        import torch

        if self.device is None:
            raise L.PbnError(L.PBN_E_STATE, "the transition graph is a host-only handle (device=None)")
        dev = torch.device("cuda", self.device)
        w = torch.as_tensor(words, device=dev)
        if w.dtype != torch.int64:
            raise ValueError(f"words: int64 [n][{self.n_words}] on the device, not {w.dtype}")
        w = w.reshape(-1, self.n_words).contiguous()
        out = torch.empty(w.shape[0], dtype=torch.int32, device=dev)
        if w.shape[0]:
            with self._on_default_stream(dev):
                L.check(L.lib.pbn_stg_lookup_device(self._h, w.data_ptr(), w.shape[0], out.data_ptr()))
        return out

    def push(self, d):
        """One step of a distribution ``d`` ``[S]`` (the scatter form, ``index_add_``): ``out[succ[s][i]] +=
        d[s] * p[s][i]``, ``out[s] += d[s] * (1 - sum_i p[s][i])``. Raises ``ValueError`` unless the set is closed."""
        import torch

        self._need_closed("push")
        p = self.probabilities()
        d = torch.as_tensor(d, dtype=torch.float64, device=p.device).reshape(self.n_states)
        out = (1.0 - p.sum(dim=1)) * d
        out.index_add_(0, self.succ.long().reshape(-1), (p * d[:, None]).reshape(-1))
        return out

    def stationary(self, tol: float = 1e-12, max_iters: int = 100000):
        """``(pi, residual, iters)``: repeated :meth:`push` from the uniform distribution until the L1 change of one
        step is at most ``tol`` or ``max_iters`` steps were made. ``residual`` is the last L1 change: reported,
        never promised. Inside an attractor (irreducible; the stay mass makes it aperiodic) ``pi`` is the exact
        stationary distribution's float64 approximation, which a census only estimates."""
        import torch

        self._need_closed("stationary")
        pi = torch.full((self.n_states,), 1.0 / self.n_states, dtype=torch.float64,
                        device=torch.device("cuda", self.device))
        residual, iters = float("inf"), 0
        while iters < int(max_iters):
            nxt = self.push(pi)
            residual = float((nxt - pi).abs().sum())
            pi = nxt
            iters += 1
            if residual <= tol:
                break
        return pi, residual, iters

    # ------------------------------------------------------------ one state, no device
    def next_states(self, row: int) -> dict:
        """``{state_tuple: prob}`` of row ``row``: ``Graph.getNextStates``' dict for a predictor-mix network. Equal
        targets are merged, and the mass of staying (the updated node keeps its value) is on the state itself when it
        is positive. Built from :func:`host_edge_mass`: no device. Each probability is one correctly rounded
        division of exact integers."""
        row = int(row)
        if not 0 <= row < self.n_states:
            raise ValueError(f"row {row} outside [0, {self.n_states - 1}]")
        mass = host_edge_mass(self.net, self.states[row], self.table_graph)[0]
        bits = unpack_bits(self.states[row], self.n_nodes)
        here = tuple(int(b) for b in bits)
        denom = TWO53 * self.n_movable
        out = {}
        moved = 0
        for i in range(self.n_nodes):
            m = int(mass[i])
            if m:
                out[here[:i] + (1 - here[i],) + here[i + 1:]] = m / denom
                moved += m
        if denom - moved > 0:
            out[here] = (denom - moved) / denom
        return out


__all__ = ["TransitionGraph", "host_edge_mass"]
