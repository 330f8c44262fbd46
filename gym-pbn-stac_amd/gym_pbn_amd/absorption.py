"""Absorption over a transition graph: where states end up, and when (``csrc/pbn_absorb.hip``).

The reference's until-attractor envs (``PBNTargetMultiEnv.step``, ``pbn_target_multi.py:133-146``) flip nodes and then
update "until the state is in an attractor, at most ``update_cap`` times"; which attractor that is, whether the cap
cut the loop and how many updates it took can only be sampled there. Over a dynamics-closed
:class:`~gym_pbn_amd.transition.TransitionGraph` the law of one update is exact (integer ``mass`` / ``succ``), so
these are sums that one kernel sweep advances for every row at once.

**The recursion.** ``label[s]`` is ``-1`` for a transient row and ``k`` in ``[0, K)`` for a row of class ``k``. The
classes are *first-hit* classes: every labelled row is held, whether or not its class is closed under the dynamics
(``K = 1`` with any target set gives "the probability of reaching the target within ``n`` updates"). For a column ``x``
with source constant ``b``, one sweep is::

    out[s] = x[s]                                                                    if label[s] >= 0  (the same bits)
    out[s] = (x[s] + (sum_i mass[s][i] * (x[succ[s][i]] - x[s])) * 2**-53 / n_movable) + b     otherwise

With ``H`` the first ``n >= 0`` at which the chain started at ``s`` is in a labelled row, ``n`` sweeps give exactly

* from ``1{label == k}``, ``b = 0``: ``P(H <= n, class k)`` -- ``prob[:, k]``;
* from ``1{label < 0}``, ``b = 0``: ``u_n = P(H > n)`` -- ``unabsorbed``;
* from ``0``, ``b = 1``: ``T_n = E[min(H, n)]`` -- ``time``.

The update is the plain (lazy) one, a row's stay mass included: sweep ``n`` is the law of exactly ``n`` updates, and
``u_n[s]`` bounds how far ``P(H <= n, k)`` is below its limit. All ``K + 2`` columns obey the same recursion over the
same arrays, so one launch of ``k_stg_absorb`` advances up to eight of them, reading ``mass`` / ``succ`` once.

**Exact**: the graph, the labels and which rows are held. **Float64**: every column; one sweep is within
``(2 N + 8) * 2**-53 * max|x| + 2**-53 * (max|x| + |b|)`` of the exact rational value per entry, and the exact operator
does not expand the sup norm, so ``n`` sweeps are within the sum of those. The result is bit-identical from call to
call, under any grid, and however the columns are chunked into launches. Memory: two ``[S][K + 2]`` float64 buffers
(``16 S (K + 2)`` bytes) beside the graph's ``12 S N``. The iteration count is the lazy chain's: no jump-chain or
Gauss-Seidel acceleration.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .network import TWO53
from .transition import TransitionGraph, _as_rows

MAX_COLS = L.STG_ABSORB_MAX_COLS  # columns of one launch


# ---------------------------------------------------------------- the arithmetic, stated in numpy (no device)
def host_absorb_sweep(mass, succ, label, n_movable: int, x, src=None) -> np.ndarray:
    """One sweep of the module docstring's recursion in numpy float64, the device's formula with the device's roundings
    per term (the order of a row's sum is numpy's). ``mass`` ``[S][N]`` integers in ``[0, 2**53]``, ``succ`` ``[S][N]``
    rows, ``label`` ``[S]`` (``>= 0``: held), ``x`` ``[S][C]`` or ``[S]``, ``src`` ``[C]`` (``None``: zeros). Returns an
    array of ``x``'s shape."""
    m = np.asarray(mass).astype(np.float64)
    S = m.shape[0]
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape
    x2 = x.reshape(S, -1)
    b = np.zeros(x2.shape[1]) if src is None else np.asarray(src, dtype=np.float64).reshape(x2.shape[1])
    t = np.asarray(succ).astype(np.int64)
    own = np.arange(S, dtype=np.int64)[:, None]
    t = np.where((t >= 0) & (t < S), t, own)  # an entry that is no row reads as "stays"
    held = np.asarray(label).reshape(S) >= 0
    out = np.empty_like(x2)
    for c in range(x2.shape[1]):
        v = x2[:, c]
        acc = (m * (v[t] - v[:, None])).sum(axis=1)
        out[:, c] = np.where(held, v, (v + (acc * (1.0 / TWO53)) / float(n_movable)) + b[c])
    return out.reshape(shape)


def host_absorb_within(mass, succ, label, n_movable: int, n_updates=None, tol: float = 1e-12,
                       max_updates: int = 1 << 20) -> dict:
    """:meth:`Absorption.within` (``n_updates`` given) or :meth:`Absorption.solve` with ``check_every = 1`` (``n_updates``
    ``None``: until ``max unabsorbed <= tol``) by :func:`host_absorb_sweep`: ``dict(prob [S][K], unabsorbed [S], time
    [S], n_updates, residual, unabsorbed_1)``."""
    lab = np.asarray(label).reshape(-1).astype(np.int64)
    S, K = lab.shape[0], int(lab.max()) + 1
    x = np.zeros((S, K + 2))
    x[lab >= 0, lab[lab >= 0]] = 1.0
    x[:, K] = lab < 0
    src = np.zeros(K + 2)
    src[K + 1] = 1.0
    n, u1 = 0, None
    stop = int(max_updates) if n_updates is None else int(n_updates)
    while n < stop and (n_updates is not None or x[:, K].max() > tol):
        x = host_absorb_sweep(mass, succ, lab, n_movable, x, src)
        n += 1
        if n == 1:
            u1 = x[:, K].copy()
    return dict(prob=x[:, :K].copy(), unabsorbed=x[:, K].copy(), time=x[:, K + 1].copy(), n_updates=n,
                residual=float(x[:, K].max()), unabsorbed_1=u1)


def step_law(prob, unabsorbed, time, transient, unabsorbed_1):
    """:meth:`AbsorptionResult.env_step_law`'s bookkeeping on rows already selected (numpy arrays or torch tensors):
    ``(label_prob, capped_prob, mean_updates)`` with ``mean_updates = time + 1{H = 0} + P(H = 1)``, ``1{H = 0} = 1 -
    transient`` and ``P(H = 1) = transient - unabsorbed_1``."""
    return prob, unabsorbed, time + (1.0 - transient) + (transient - unabsorbed_1)


def _check_labels(labels, n_states: int) -> np.ndarray:
    if hasattr(labels, "detach"):  # a torch tensor
        labels = labels.detach().cpu().numpy()
    lab = np.asarray(labels)
    if lab.shape != (n_states,) or lab.dtype.kind not in "iu":
        raise ValueError(f"labels: an int array [{n_states}], not {lab.dtype} {lab.shape}")
    lab = lab.astype(np.int64)
    if lab.size and lab.min() < -1:
        raise ValueError(f"labels hold {int(lab.min())}: -1 marks a transient row, k >= 0 a row of class k")
    if not (lab >= 0).any():
        raise ValueError("no labelled row: nothing absorbs")
    if lab.max() > 0x7FFFFFFF:
        raise ValueError("labels must lie in [-1, 2^31)")
    return lab.astype(np.int32)


class AbsorptionResult:
    """What :meth:`Absorption.within` and :meth:`Absorption.solve` return, at horizon ``n_updates``: ``prob`` ``[S][K]``
    (``P(H <= n, class k)``), ``unabsorbed`` ``[S]`` (``P(H > n)``) and ``time`` ``[S]`` (``E[min(H, n)]``), float64 on the
    device; ``residual`` = ``max(unabsorbed)``, reported, never promised; ``unabsorbed_1`` = ``P(H > 1)`` (``None`` at
    ``n_updates == 0``), which :meth:`env_step_law` needs."""

    def __init__(self, absorption: "Absorption", prob, unabsorbed, time, n_updates: int, residual: float, unabsorbed_1):
        self.absorption = absorption
        self.prob, self.unabsorbed, self.time = prob, unabsorbed, time
        self.n_updates, self.residual = int(n_updates), float(residual)
        self.unabsorbed_1 = unabsorbed_1

    def basin_weights(self, weights=None):
        """Device float64 ``[K]``: the mean of ``prob`` over the rows, or with ``weights`` ``[S]`` the weighted sum
        ``weights @ prob``. Over all ``2**N`` states the mean is the exact basin weight of each class at this horizon:
        the share of the state space that has drained into it."""
        import torch

        if weights is None:
            return self.prob.mean(dim=0)
        w = torch.as_tensor(weights, dtype=torch.float64, device=self.prob.device).reshape(self.prob.shape[0])
        return w @ self.prob

    def _rows(self, words):
        rows = self.absorption.graph.row_of(words)
        missing = int((rows < 0).sum())
        if missing:
            raise ValueError(f"{missing} state(s) are no row of the graph")
        return rows.long()

    def at(self, words):
        """``(prob [n][K], unabsorbed [n], time [n])`` of the device state words ``words`` (int64 ``[n][W]``), through the
        graph's own table. A state that is no row of the graph is a ``ValueError``."""
        r = self._rows(words)
        return self.prob[r], self.unabsorbed[r], self.time[r]

    def env_step_law(self, words):
        """``(label_prob [n][K], capped_prob [n], mean_updates [n])``: the exact law of one
        ``TorchVecPBNTargetMultiSetEnv.step`` whose state after the flips is ``words[e]``, at ``update_cap =
        n_updates``, for attractor classes (closed under the dynamics).

        From the step loop (``pbn_target_multi.py:133-146``; ``orc_env_step_multi`` in the oracle): the env always
        makes update 1; after update 1 it tests the snapshot taken *before* that update; from update 2 on it tests
        the state itself. So with ``H`` the first ``n >= 0`` at which the chain from ``words[e]`` is in an attractor:
        ``H = 0`` ends the loop after 1 update; ``H = 1`` is not seen after update 1 (the snapshot is older) and ends it
        after update 2, where the state is still inside the closed attractor; ``2 <= H <= cap`` ends it after ``H``
        updates; otherwise the cap ends it, unlabelled. Hence the env is labelled ``k`` iff ``H <= cap`` in class ``k``
        and ``n_updates`` is 1, 2, ``H``, ``cap`` in the four cases::

            label_prob   = prob              capped_prob = unabsorbed
            mean_updates = E[min(H, cap)] + 1{H = 0} + P(H = 1) = time + 1{label >= 0} + (u_0 - u_1)

        with ``u_0 = 1{label < 0}`` and ``u_1`` = :attr:`unabsorbed_1`. The case split needs ``cap >= 2``: a smaller
        ``n_updates`` is refused."""
        if self.n_updates < 2:
            raise ValueError(f"env_step_law needs n_updates >= 2 (the env tests the state from update 2 on), not "
                             f"{self.n_updates}")
        r = self._rows(words)
        return step_law(self.prob[r], self.unabsorbed[r], self.time[r], self.absorption.transient[r], self.unabsorbed_1[r])


class Absorption:
    """``Absorption(graph, labels)``: the first-hit recursion of the module docstring over a closed
    :class:`TransitionGraph`. ``labels``: an int array ``[S]`` over the graph's rows, ``-1`` a transient row, ``k >= 0`` a
    row of class ``k`` (``K`` = the largest label + 1). Raises ``ValueError`` for a label below ``-1``, for no labelled
    row, and unless ``graph.closed``. Keeps the labels on the device, two ``[S][K + 2]`` float64 buffers and one ``[S]``."""

    def __init__(self, graph: TransitionGraph, labels):
        import torch

        lab = _check_labels(labels, graph.n_states)
        if graph.device is None:
            raise L.PbnError(L.PBN_E_STATE, "the transition graph is a host-only handle (device=None)")
        graph._need_closed("Absorption")
        self.graph = graph
        self.labels_host = lab
        self.n_classes = K = int(lab.max()) + 1
        self.device = dev = torch.device("cuda", graph.device)
        self.labels = torch.from_numpy(lab).to(dev)
        self.transient = (self.labels < 0).to(torch.float64)  # u_0
        S = graph.n_states
        self._a = torch.empty((S, K + 2), dtype=torch.float64, device=dev)
        self._b = torch.empty((S, K + 2), dtype=torch.float64, device=dev)
        self._u1 = torch.empty(S, dtype=torch.float64, device=dev)  # u_1, kept by every run for env_step_law
        self._src = np.zeros(K + 2, dtype=np.float64)
        self._src[K + 1] = 1.0

    @classmethod
    def from_attractors(cls, graph: TransitionGraph, attractors) -> "Absorption":
        """``attractors``: a list of attractors (each packed rows ``[S_k][W]`` uint64 or a list of state tuples), an
        :class:`~gym_pbn_amd.attractors.AttractorResult`, or a labelled :class:`~gym_pbn_amd.stateset.StateSet`; class
        ``k`` is attractor ``k`` resp. label ``k``. The members' rows come from the graph's own table
        (:meth:`TransitionGraph.row_of`), a ``StateSet``'s from its host lookup of the graph's states. A member state
        that is no row of the graph is a ``ValueError``."""
        import torch

        from .attractors import AttractorResult
        from .stateset import StateSet

        S = graph.n_states
        if isinstance(attractors, StateSet):
            if attractors.n_nodes != graph.n_nodes:
                raise ValueError(f"a state set of {attractors.n_nodes} nodes for a graph of {graph.n_nodes}")
            lab = attractors.lookup(graph.states).astype(np.int32)
            if int((lab >= 0).sum()) != len(attractors):
                raise ValueError(f"{len(attractors) - int((lab >= 0).sum())} member state(s) are no row of the graph")
            return cls(graph, lab)
        if isinstance(attractors, AttractorResult):
            attractors = attractors.attractors
        if graph.device is None:
            raise L.PbnError(L.PBN_E_STATE, "the transition graph is a host-only handle (device=None)")
        lab = np.full(S, -1, dtype=np.int32)
        for k, a in enumerate(attractors):
            rows = _as_rows(a if isinstance(a, np.ndarray) else np.asarray(a), graph.n_nodes)
            words = torch.from_numpy(rows.view(np.int64)).to(torch.device("cuda", graph.device))
            r = graph.row_of(words).cpu().numpy()
            if (r < 0).any():
                raise ValueError(f"{int((r < 0).sum())} state(s) of attractor {k} are no row of the graph")
            if (lab[r] >= 0).any():
                raise ValueError(f"attractor {k} shares a state with an earlier one")
            lab[r] = k
        return cls(graph, lab)

    # ------------------------------------------------------------ one sweep
    def _launch(self, x, out, src):
        """``k_stg_absorb`` on float64 device tensors ``[S][C]`` (any ``C``, row-major), in launches of at most eight
        columns: each launch takes its columns in place (``ld = C``), so the chunking copies nothing and -- the sum
        order being the column's own -- cannot be observed. No checks, no ordering: the caller's."""
        g = self.graph
        mass, succ = g.mass, g.succ
        cols = x.shape[1]
        for lo in range(0, cols, MAX_COLS):
            n = min(MAX_COLS, cols - lo)
            b = (C.c_double * n)(*[float(v) for v in src[lo:lo + n]])
            L.check(L.lib.pbn_stg_absorb_device(g.handle, mass.data_ptr(), succ.data_ptr(), self.labels.data_ptr(),
                                                x.data_ptr() + 8 * lo, out.data_ptr() + 8 * lo, n, cols, b))

    def sweep(self, x, src=None):
        """One sweep of ``x`` (``[S][C]`` or ``[S]``, any ``C``, taken as float64 on the device) with source constants
        ``src`` (``[C]``, ``None``: zeros): a fresh tensor of ``x``'s shape."""
        import torch

        S = self.graph.n_states
        x = torch.as_tensor(x, dtype=torch.float64, device=self.device)
        shape = x.shape
        x2 = x.reshape(S, -1).contiguous()
        cols = x2.shape[1]
        b = np.zeros(cols) if src is None else np.asarray(src, dtype=np.float64).reshape(cols)
        out = torch.empty_like(x2)
        if cols:
            with self.graph._on_default_stream(self.device):
                self._launch(x2, out, b)
        return out.reshape(shape)

    # ------------------------------------------------------------ the standard columns
    def _start(self):
        K = self.n_classes
        a = self._a
        a.zero_()
        a[:, :K].scatter_(1, self.labels.clamp(min=0).long()[:, None], (1.0 - self.transient)[:, None])
        a[:, K] = self.transient
        return a, self._b

    def within(self, n_updates: int) -> AbsorptionResult:
        """The law at horizon ``n_updates >= 0``: that many sweeps from the standard start, one wait after the last (for
        ``residual``)."""
        n_updates = int(n_updates)
        if n_updates < 0:
            raise ValueError(f"n_updates={n_updates} is negative")
        return self._run(n_updates, None, max(n_updates, 1))

    def solve(self, tol: float = 1e-12, max_updates: int = 1 << 20, check_every: int = 16) -> AbsorptionResult:
        """Sweeps until ``max_s unabsorbed[s] <= tol`` -- looked at every ``check_every`` sweeps and after the last, each
        look a device-to-host wait and the only ones -- or ``max_updates`` sweeps were made. With attractor classes and
        every state draining into one, ``prob`` is then within ``tol`` (plus the rounding band) of the absorption
        probabilities and ``time`` of the expected hitting time's partial sum."""
        return self._run(int(max_updates), float(tol), max(int(check_every), 1))

    def _run(self, max_updates, tol, check_every):
        K = self.n_classes
        # before the first sweep the survival column is the indicator of the transient rows: known on the host
        residual = 1.0 if bool((self.labels_host < 0).any()) else 0.0
        n = 0
        with self.graph._on_default_stream(self.device):
            a, b = self._start()
            while n < max_updates and (tol is None or residual > tol):
                self._launch(a, b, self._src)
                a, b = b, a
                n += 1
                if n == 1:
                    self._u1.copy_(a[:, K])
                if n % check_every == 0 or n == max_updates:
                    residual = float(a[:, K].max())
        # outside the context: the result's tensors belong to the caller's stream, which the context's exit has
        # ordered behind the sweeps
        return AbsorptionResult(self, a[:, :K].clone(), a[:, K].clone(), a[:, K + 1].clone(), n, residual,
                                self._u1.clone() if n >= 1 else None)


__all__ = ["Absorption", "AbsorptionResult", "host_absorb_sweep", "host_absorb_within", "step_law", "MAX_COLS"]
