"""The multi-flip until-attractor MDP, solved exactly on the device (``csrc/pbn_flipset.hip``).

The reference's main environment (``PBNTargetMultiEnv.step``, ``pbn_target_multi.py:105-146``; here
:class:`~gym_pbn_amd.torch_env.TorchVecPBNTargetMultiSetEnv`) flips up to ``A`` nodes in one step and then updates
until the state is in an attractor, at most ``update_cap`` times. The reference trains agents against this MDP and never
solves it. Over a dynamics-closed :class:`~gym_pbn_amd.transition.TransitionGraph` with attractor labels the law of that
macro step is exact (:mod:`gym_pbn_amd.absorption`), so ``V*`` and an optimal policy can be computed and an agent
compared with them.

**The MDP.** State: a row ``s`` of the graph (the env's live state). Action: a set ``F`` of ``1 <= |F| <= A`` distinct
allowed nodes, at cost ``k |F|`` (``k = action_cost``, the env's ``dedup=True``); ``noop_cost=c`` adds the empty set at
cost ``c``. One step from ``t = s ^ F`` follows §18's step law: a labelled ``t`` makes one update and ends with its
label; a transient ``t`` makes updates 1 and 2 and then tests the state itself after update 2, 3, ..., ``n`` (``n`` =
the cap), stopping at the first labelled state. The reward is ``R 1{label == target} - k |F|`` (``R = reward_success``),
the episode ends iff ``label == target``, the return is discounted by ``gamma`` per env step. With ``E`` =
:meth:`TransitionGraph.expect` and ``sweep`` = :meth:`Absorption.sweep` with source 0 (labelled rows are held)::

    g[x]  = label[x] == target ? R : gamma * V[x]   # worth of ending at x: labelled -> by the test; transient -> by the cap
    Z     = sweep^(n-2)(g)
    M     = where(label >= 0, E(g), E(E(Z)))        # the worth of arriving at t by the flips, before their cost
    V'[s] = max over F of M[s ^ F] - k * |F|        (and M[s] - noop_cost, if given)

``V -> V'`` is a sup-norm contraction of modulus ``gamma``. The max is the top-two recursion of
``csrc/pbn_flipset_rule.hpp``: ``A`` launches of ``k_stg_flipset`` and one of ``k_stg_flipset_select``, ``N * A`` gathers
per row where enumeration makes ``sum_{j <= A} C(N, j)`` probes. The order among equal actions: larger value, then fewer
flips, then the lower end row; the empty set wins a tie.

**Exact**: the graph, the labels, ``nbr``, which sets are actions, the order. **Float64**: every value. ``M`` is within
the summed bound of its ``n - 2`` sweeps and three expectations of the exact value; the max adds one rounded multiply
and one rounded subtract. ``n_updates=None`` uses ``n = min(update_cap, n_tol)``, ``n_tol`` the sweep count at which
``Absorption.solve(tol=inner_tol)`` stops; ``inner_residual`` is then the largest unabsorbed probability ``max u_n``, and
the law at any larger cap differs from the one used by at most ``u_n * max|g|`` per entry: reported, never promised.
"""

from __future__ import annotations

import ctypes as C
import itertools
import math

import numpy as np

from . import _lib as L
from .absorption import Absorption, host_absorb_sweep
from .control import host_expect
from .transition import TransitionGraph

MAX_FLIPS = L.STG_FLIPSET_MAX_FLIPS
FOR_ENV_MAX_NODES = 24  # for_env enumerates 2**N states: the graph's cap of 2**24 rows


# ---------------------------------------------------------------- the statements, in numpy (no device)
def _host_nbr(states_or_nbr, nodes):
    """``nbr`` ``[S][N]`` int64 from packed states ``[S][W]`` uint64 (a dict of the rows; ``-1``: no row, or a node that is
    not allowed) or from an int array that is ``nbr`` already (columns outside ``nodes`` are not read)."""
    a = np.asarray(states_or_nbr)
    if a.dtype != np.uint64:
        return a.astype(np.int64)
    a = np.ascontiguousarray(a)
    index = {row.tobytes(): r for r, row in enumerate(a)}
    n_nodes = max(nodes) + 1 if nodes else 0
    out = np.full((a.shape[0], max(n_nodes, 1)), -1, dtype=np.int64)
    for i in nodes:
        t = a.copy()
        t[:, i // 64] ^= np.uint64(1) << np.uint64(i % 64)
        out[:, i] = [index.get(row.tobytes(), -1) for row in t]
    return out


def host_multiflip_max(m, states_or_nbr, nodes, max_flips: int, cost: float, noop_cost=None):
    """``(v, policy_end, policy_flips)`` by plain enumeration: for every row ``s`` every set ``F`` of ``1 .. max_flips``
    distinct nodes of ``nodes`` (``itertools.combinations``), worth ``m[row of s ^ F] - cost * len(F)``; the best under
    the order larger value, then fewer flips, then lower end row; with ``noop_cost`` the empty set at ``m[s] -
    noop_cost``, which wins a tie. ``states_or_nbr``: packed states ``[S][W]`` uint64 or ``nbr`` ``[S][N]``. A set that
    leaves the state set is a ``ValueError``. Rows with no action: ``-inf, -1, 0``."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    S = m.shape[0]
    nodes = sorted({int(i) for i in nodes})
    nbr = _host_nbr(states_or_nbr, nodes)
    own = np.arange(S, dtype=np.int64)
    v = np.full(S, -np.inf)
    end = np.full(S, -1, dtype=np.int64)
    flips = np.zeros(S, dtype=np.int64)
    for d in range(1, min(int(max_flips), len(nodes)) + 1):
        c = float(cost) * float(d)
        for F in itertools.combinations(nodes, d):
            y = own
            for i in F:
                y = nbr[y, i]
                if (y < 0).any():
                    raise ValueError(f"the flip of node {i} leaves the state set")
            q = m[y] - c
            # sets of d flips come after every smaller set: "fewer flips" is the loop's order
            better = (q > v) | ((q == v) & (flips == d) & (y < end))
            v, end, flips = np.where(better, q, v), np.where(better, y, end), np.where(better, d, flips)
    if noop_cost is not None:
        stay = m - float(noop_cost)
        take = stay >= v
        v, end, flips = np.where(take, stay, v), np.where(take, own, end), np.where(take, 0, flips)
    return v, end.astype(np.int32), flips.astype(np.int32)


def host_multiflip_arrival(mass, succ, label, n_movable: int, target: int, v, n_updates: int, reward_success=1000,
                           gamma: float = 0.99) -> np.ndarray:
    """``M`` of the module docstring in numpy float64, built on :func:`~gym_pbn_amd.control.host_expect` and
    :func:`~gym_pbn_amd.absorption.host_absorb_sweep`: the worth of arriving at each row by the flips, at cap
    ``n_updates >= 2``."""
    if int(n_updates) < 2:
        raise ValueError(f"n_updates={n_updates}: the step law needs a cap of at least 2")
    lab = np.asarray(label).reshape(-1)
    v = np.asarray(v, dtype=np.float64).reshape(lab.shape[0])
    g = np.where(lab == int(target), float(reward_success), float(gamma) * v)
    z = g
    for _ in range(int(n_updates) - 2):
        z = host_absorb_sweep(mass, succ, lab, n_movable, z)
    e = lambda x: host_expect(mass, succ, n_movable, x)  # noqa: E731
    return np.where(lab >= 0, e(g), e(e(z)))


# ---------------------------------------------------------------- the device side
def _check_params(n_classes, target, max_flips, n_updates, update_cap, gamma, action_cost, noop_cost, reward_success):
    if not 0 <= int(target) < int(n_classes):
        raise ValueError(f"target={target} outside the classes [0, {n_classes})")
    if not 1 <= int(max_flips) <= MAX_FLIPS:
        raise ValueError(f"max_flips={max_flips} outside [1, {MAX_FLIPS}]")
    if n_updates is not None and int(n_updates) < 2:
        raise ValueError(f"n_updates={n_updates}: the step law needs a cap of at least 2")
    if int(update_cap) < 2:
        raise ValueError(f"update_cap={update_cap}: the step law needs a cap of at least 2")
    if not 0.0 <= float(gamma) < 1.0:
        raise ValueError(f"gamma={gamma} outside [0, 1)")
    for name, c in (("action_cost", action_cost), ("noop_cost", noop_cost)):
        if c is not None and not (0.0 <= float(c) < math.inf):
            raise ValueError(f"{name}={c} is not a finite cost >= 0")
    if not math.isfinite(float(reward_success)):
        raise ValueError(f"reward_success={reward_success} is not finite")


class MultiFlipSolution:
    """What :meth:`MultiFlipProblem.solve` returns: ``v`` (float64 ``[S]``), ``policy_end`` (int32 ``[S]``: the row the
    chosen flips lead to; the row itself for the empty set) and ``policy_flips`` (int32 ``[S]``: ``|F|``) on the device;
    ``residual`` (the last sup-norm change of a backup: reported, never promised), ``iters`` (backups made),
    ``n_updates`` (the cap ``n`` the law was taken at) and ``inner_residual`` (``max u_n``: see the module docstring)."""

    def __init__(self, problem: "MultiFlipProblem", v, policy_end, policy_flips, residual: float, iters: int):
        self.problem, self.v, self.policy_end, self.policy_flips = problem, v, policy_end, policy_flips
        self.residual, self.iters = float(residual), int(iters)
        self.n_updates, self.inner_residual = problem.n_updates, problem.inner_residual

    def flip_words(self):
        """Device int64 ``[S][W]``: ``F`` of every row as state words, ``states[s] ^ states[policy_end[s]]``."""
        p = self.problem
        return p.states ^ p.states[self.policy_end.long()]

    def act(self, words, width=None, check: bool = False):
        """Env action rows int32 ``[n][width]`` (``width`` = ``max_flips`` by default) for the device state words
        ``words`` (int64 ``[n][W]``, e.g. ``env.observation_words()``): the ``node + 1`` values of ``F`` ascending, the
        first repeated into the unused slots; the empty set is all zeros. A state that is no row of the graph gets an
        all-zero row; ``check=True`` waits and raises ``ValueError`` then."""
        import torch

        p = self.problem
        A = p.max_flips if width is None else int(width)
        if A < p.max_flips:
            raise ValueError(f"width={A} below max_flips={p.max_flips}")
        rows = p.graph.row_of(words)
        if check and bool((rows < 0).any()):
            raise ValueError(f"{int((rows < 0).sum())} state(s) are no row of the graph")
        ok = rows >= 0
        r = rows.clamp(min=0).long()
        F = p.states[r] ^ p.states[self.policy_end[r].long()]  # [n][W]
        nodes = p._nodes_t  # [n_allowed] int64, ascending
        bit = ((F[:, nodes // 64] >> (nodes % 64)) & 1).bool() & ok[:, None]
        big = p.graph.n_nodes + 1
        key = torch.where(bit, (nodes + 1)[None, :], torch.full_like(nodes, big)[None, :])
        if key.shape[1] < A:
            key = torch.cat([key, key.new_full((key.shape[0], A - key.shape[1]), big)], dim=1)
        key = key.sort(dim=1).values[:, :A]
        first = torch.where(key[:, :1] == big, torch.zeros_like(key[:, :1]), key[:, :1])
        return torch.where(key == big, first, key).to(torch.int32)


class MultiFlipProblem:
    """``MultiFlipProblem(absorption, target, *, max_flips, n_updates=None, update_cap=1 << 20, inner_tol=1e-12,
    reward_success=1000, action_cost=1, noop_cost=None, gamma=0.99, nodes=None)``: the MDP of the module docstring over
    the graph and the labels of an :class:`~gym_pbn_amd.absorption.Absorption`.

    ``target``: a class index. ``nodes``: the nodes an action may flip (default: every node, as the env's actions).
    Raises ``ValueError`` for classes that are not closed under the dynamics (a labelled row with ``mass > 0`` into a
    row of another label), an allowed flip that leaves the state set, ``max_flips`` outside ``[1, 15]``, ``n_updates <
    2``, no allowed node and no ``noop_cost``, ``gamma`` outside ``[0, 1)``, a negative cost."""

    def __init__(self, absorption: Absorption, target: int, *, max_flips: int, n_updates=None, update_cap: int = 1 << 20,
                 inner_tol: float = 1e-12, reward_success=1000, action_cost=1, noop_cost=None, gamma: float = 0.99,
                 nodes=None):
        import torch

        graph: TransitionGraph = absorption.graph
        _check_params(absorption.n_classes, target, max_flips, n_updates, update_cap, gamma, action_cost, noop_cost,
                      reward_success)
        N, S, W = graph.n_nodes, graph.n_states, graph.n_words
        self.nodes = sorted({int(i) for i in (range(N) if nodes is None else nodes)})
        if self.nodes and not 0 <= self.nodes[0] <= self.nodes[-1] < N:
            raise ValueError(f"nodes outside [0, {N - 1}]")
        if not self.nodes and noop_cost is None:
            raise ValueError("no allowed node and no noop_cost: the MDP has no action")
        if graph.device is None:
            raise L.PbnError(L.PBN_E_STATE, "the transition graph is a host-only handle (device=None)")
        self.absorption, self.graph = absorption, graph
        self.target, self.max_flips = int(target), int(max_flips)
        self.reward_success, self.action_cost, self.gamma = float(reward_success), float(action_cost), float(gamma)
        self.noop_cost = None if noop_cost is None else float(noop_cost)
        self.device = dev = absorption.device
        lab = absorption.labels
        mass, succ = graph.mass, graph.succ
        crossing = (lab[:, None] >= 0) & (mass > 0) & (lab[succ.long().clamp(min=0)] != lab[:, None])
        if bool(crossing.any()):
            raise ValueError(f"the classes are not closed under the dynamics: {int(crossing.sum())} edge(s) lead from a "
                             f"labelled row into a row of another label")
        mask = np.zeros(W, dtype=np.uint64)
        for i in self.nodes:
            mask[i // 64] |= np.uint64(1) << np.uint64(i % 64)
        self.action_mask = mask
        self.nbr = torch.empty((S, N), dtype=torch.int32, device=dev)
        with graph._on_default_stream(dev):
            L.check(L.lib.pbn_stg_flip_rows_device(graph.handle, 0, S, L.ptr(mask, L._u64p), self.nbr.data_ptr()))
        self._nodes_t = torch.tensor(self.nodes, dtype=torch.int64, device=dev)
        if self.nodes:
            gone = int((self.nbr[:, self._nodes_t] < 0).sum())
            if gone:
                raise ValueError(f"{gone} allowed flip(s) leave the state set: it is not closed under the flips")
        self.states = torch.from_numpy(graph.states.view(np.int64)).to(dev)
        # the cap n and what it leaves out
        if n_updates is None:
            r = absorption.solve(tol=float(inner_tol), max_updates=int(update_cap))
            self.n_updates = max(r.n_updates, 2)
            self.inner_residual = r.residual if r.n_updates >= 2 else absorption.within(2).residual
        else:
            self.n_updates = int(n_updates)
            self.inner_residual = absorption.within(self.n_updates).residual
        f64 = dict(dtype=torch.float64, device=dev)
        self._is_target = lab == self.target
        self._labelled = lab >= 0
        self._r = torch.tensor(self.reward_success, **f64)
        self._g, self._e1, self._e2, self._m = (torch.empty(S, **f64) for _ in range(4))
        self._za, self._zb = (torch.empty((S, 1), **f64) for _ in range(2))
        self._base = [torch.empty((S, 2), **f64) for _ in range(2)]
        self._tag = [torch.empty((S, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        self._noop = None if self.noop_cost is None else C.c_double(self.noop_cost)

    # ------------------------------------------------------------ the pieces of a backup (no checks, no ordering)
    def _arrival_into(self, v, m):
        """``M`` of ``v`` into ``m``: ``n - 2`` launches of ``k_stg_absorb`` and three of ``k_stg_expect``."""
        import torch

        g = self._g
        torch.mul(v, self.gamma, out=g)
        torch.where(self._is_target, self._r, g, out=g)
        a, b = self._za, self._zb
        a.copy_(g[:, None])
        for _ in range(self.n_updates - 2):
            self.absorption._launch(a, b, (0.0,))
            a, b = b, a
        gr = self.graph
        gr._expect_into(g, self._e1)
        gr._expect_into(a.reshape(-1), self._e2)
        gr._expect_into(self._e2, m)
        torch.where(self._labelled, self._e1, m, out=m)

    def _max_into(self, m, v_new, policy_end, policy_flips):
        """The max over the flip sets of ``m``: ``max_flips`` launches of ``k_stg_flipset`` and the select."""
        h, k = self.graph.handle, self.action_cost
        src = None
        for lev in range(self.max_flips):
            base, tag = self._base[lev & 1], self._tag[lev & 1]
            L.check(L.lib.pbn_stg_flipset_level_device(h, self.nbr.data_ptr(), m.data_ptr(), k,
                                                       None if src is None else src[0].data_ptr(),
                                                       None if src is None else src[1].data_ptr(), base.data_ptr(),
                                                       tag.data_ptr()))
            src = (base, tag)
        L.check(L.lib.pbn_stg_flipset_select_device(h, src[0].data_ptr(), src[1].data_ptr(), m.data_ptr(), k,
                                                    None if self._noop is None else C.byref(self._noop),
                                                    v_new.data_ptr(), policy_end.data_ptr(), policy_flips.data_ptr()))

    def _backup_into(self, v, v_new, policy_end, policy_flips):
        self._arrival_into(v, self._m)
        self._max_into(self._m, v_new, policy_end, policy_flips)

    def _as_v(self, v):
        import torch

        return torch.as_tensor(v, dtype=torch.float64, device=self.device).reshape(self.graph.n_states).contiguous()

    def _policy_buffers(self):
        import torch

        S = self.graph.n_states
        return (torch.empty(S, dtype=torch.int32, device=self.device), torch.empty(S, dtype=torch.int32, device=self.device))

    # ------------------------------------------------------------ public
    def arrival(self, v):
        """``M``: the worth of arriving at each row by the flips, before their cost. A fresh float64 ``[S]``."""
        v = self._as_v(v)
        with self.graph._on_default_stream(self.device):
            self._arrival_into(v, self._m)
        return self._m.clone()

    def flipset_max(self, m):
        """``(v, policy_end, policy_flips)``: the max over the flip sets of any arrival worth ``m`` ``[S]``, fresh
        tensors."""
        import torch

        m = self._as_v(m)
        v_new = torch.empty_like(m)
        end, flips = self._policy_buffers()
        with self.graph._on_default_stream(self.device):
            self._max_into(m, v_new, end, flips)
        return v_new, end, flips

    def backup(self, v):
        """One Bellman backup: ``(v_new, policy_end, policy_flips)``, fresh device tensors."""
        import torch

        v = self._as_v(v)
        v_new = torch.empty_like(v)
        end, flips = self._policy_buffers()
        with self.graph._on_default_stream(self.device):
            self._backup_into(v, v_new, end, flips)
        return v_new, end, flips

    def _iterate(self, sweep, v0, tol, max_iters, check_every):
        import torch

        v = torch.zeros(self.graph.n_states, dtype=torch.float64, device=self.device) if v0 is None else self._as_v(v0).clone()
        nxt = torch.empty_like(v)
        residual, iters = float("inf"), 0
        check_every = max(int(check_every), 1)
        with self.graph._on_default_stream(self.device):
            while iters < int(max_iters):
                sweep(v, nxt)
                iters += 1
                look = iters % check_every == 0 or iters == int(max_iters)
                if look:
                    residual = float((nxt - v).abs().max())  # the only wait of a backup
                v, nxt = nxt, v
                if look and residual <= tol:
                    break
        return v, residual, iters

    def solve(self, tol: float = 1e-9, max_iters: int = 100000, check_every: int = 4, v0=None) -> MultiFlipSolution:
        """Value iteration from ``v0`` (zeros) until a backup's sup-norm change is at most ``tol`` -- looked at every
        ``check_every`` backups, each look a device-to-host wait -- or ``max_iters`` backups were made. ``v`` is then
        within ``tol * gamma / (1 - gamma)`` (plus the rounding band) of ``V*``; the policy is the last backup's."""
        end, flips = self._policy_buffers()
        end.fill_(-1)
        flips.zero_()
        v, residual, iters = self._iterate(lambda a, b: self._backup_into(a, b, end, flips), v0, tol, max_iters, check_every)
        return MultiFlipSolution(self, v.clone(), end, flips, residual, iters)

    def evaluate(self, policy_end, tol: float = 1e-9, max_iters: int = 100000, check_every: int = 4, v0=None):
        """``(v, residual, iters)``: the value of the fixed policy ``policy_end`` (int ``[S]``: the row each row's flips
        lead to; the row itself: the empty set), by iterating ``V'[s] = M[policy_end[s]] - k |F|``. ``ValueError`` for
        an entry that is no row, a set of more than ``max_flips`` nodes or with a node that is not allowed, and the
        empty set without ``noop_cost``."""
        import torch

        S = self.graph.n_states
        p = torch.as_tensor(policy_end, device=self.device).reshape(S).long()
        if bool(((p < 0) | (p >= S)).any()):
            raise ValueError(f"policy_end entries outside [0, {S - 1}]")
        F = self.states ^ self.states[p]
        allowed = torch.from_numpy(self.action_mask.view(np.int64)).to(self.device)
        if bool((F & ~allowed[None, :]).any()):
            raise ValueError("a row is given a flip of a node that is not allowed")
        d = torch.zeros(S, dtype=torch.int64, device=self.device)
        for i in self.nodes:
            d += (F[:, i // 64] >> (i % 64)) & 1
        if bool((d > self.max_flips).any()):
            raise ValueError(f"a row is given more than max_flips={self.max_flips} flips")
        stay = d == 0
        if self.noop_cost is None and bool(stay.any()):
            raise ValueError(f"{int(stay.sum())} row(s) are given the empty set, which is no action without noop_cost")
        cost = self.action_cost * d.to(torch.float64)  # the kernel's product: one rounding
        if self.noop_cost is not None:
            cost = torch.where(stay, torch.full_like(cost, self.noop_cost), cost)

        def sweep(v, nxt):
            self._arrival_into(v, self._m)
            torch.sub(self._m[p], cost, out=nxt)

        v, residual, iters = self._iterate(sweep, v0, tol, max_iters, check_every)
        return v.clone(), residual, iters

    # ------------------------------------------------------------ the env's MDP
    @classmethod
    def for_env(cls, env, gamma: float = 0.99, max_flips: int = 1, target=None, **kw) -> "MultiFlipProblem":
        """The MDP a :class:`~gym_pbn_amd.torch_env.TorchVecPBNTargetMultiSetEnv` simulates: all ``2**N`` states (refused
        for ``N > 24``), ``table_graph`` ``None`` for a predictor-mix network and ``"step"`` for truth tables, the labels
        of ``env.set``, the env's reward constants and ``update_cap``, every node allowed; ``target`` defaults to the
        env's ``K - 1``."""
        from .network import KIND_PROB_TABLE

        N = int(env.N)
        if N > FOR_ENV_MAX_NODES:
            raise ValueError(f"{N} nodes: for_env enumerates 2**N states and stops at 2**{FOR_ENV_MAX_NODES}")
        states = np.arange(1 << N, dtype=np.uint64).reshape(-1, 1)
        graph = TransitionGraph(env.net, states, table_graph="step" if env.net.kind == KIND_PROB_TABLE else None,
                                device=env.device.index)
        labels = env.set.lookup(states).astype(np.int32)
        kw.setdefault("reward_success", env.reward_success)
        kw.setdefault("action_cost", env.action_cost)
        kw.setdefault("update_cap", env.update_cap)
        return cls(Absorption(graph, labels), env.n_attractors - 1 if target is None else int(target),
                   max_flips=max_flips, gamma=gamma, **kw)


__all__ = ["MultiFlipProblem", "MultiFlipSolution", "host_multiflip_max", "host_multiflip_arrival", "MAX_FLIPS",
           "FOR_ENV_MAX_NODES"]
