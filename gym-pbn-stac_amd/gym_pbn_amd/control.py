"""Exact optimal control over a transition graph: value iteration on the device (``csrc/pbn_control.hip``).

The reference trains agents to steer a PBN into a target (``PBNEnv.step`` + ``_get_reward``, ``pbn_env.py:125-188``) and
never solves the MDP it defines. Over a dynamics-closed :class:`~gym_pbn_amd.transition.TransitionGraph` the law is
exact (integer ``mass`` / ``succ``), so the optimal value and policy of the **single-flip MDP** can be computed and an
agent trained on :class:`~gym_pbn_amd.torch_env.TorchVecPBNEnv` compared with them.

**The MDP.** ``T[s]`` marks the target set, ``R`` = ``reward_target``, ``c`` = ``step_cost``, ``k`` = ``action_cost``
(defaults 20 / 4 / 1: the literals of ``pbn_env.py:156-188``), ``gamma`` the discount. An action is the no-op or the
flip of one allowed node ``i``: ``t = s`` resp. ``t = s ^ bit(i)``, then one asynchronous update from ``t`` under the
graph's law. If the next state is in the target the reward is ``R`` and the episode ends; otherwise it is ``-c``, minus
``k`` when the action was a flip. With ``E`` the graph's one-step expectation (:meth:`TransitionGraph.expect`)::

    h[s'] = T[s'] ? R : (-c + gamma * V[s'])
    U     = E[h]                    # per sweep
    nT    = E[1 - T]                # once per problem
    Ua    = U - k * nT              # the value of arriving at t by a flip
    V'[s] = max(U[s], max over allowed i with nbr[s][i] >= 0 of Ua[nbr[s][i]])
    pi[s] = the arg max: -1 the no-op, else the node; ties: the no-op first, then the lowest node

``nbr[s][i]`` is the row of ``s ^ bit(i)`` whatever the mass of that flip, ``-1`` outside the set: a flip that leaves
the set is not an action at that state.

**Exact**: ``nbr`` and the action restriction the policy obeys (integers). **Float64**: every value and expectation.
Memory: ``16 S N`` bytes for ``mass``, ``succ`` and ``nbr``. The until-attractor multi-flip MDP is
:mod:`gym_pbn_amd.multiflip`'s.
"""

from __future__ import annotations

import numpy as np

from . import _lib as L
from .attractors import rows_in
from .network import TWO53
from .transition import TransitionGraph, _as_rows

FOR_ENV_MAX_FREE_NODES = 24  # for_env enumerates 2**(N - 1) states: the graph's cap of 2**24 rows


# ---------------------------------------------------------------- the arithmetic, stated in numpy (no device)
def host_expect(mass, succ, n_movable: int, v) -> np.ndarray:
    """``E[v(next) | s]`` in numpy float64: ``v[s] + (sum_i mass[s][i] * (v[succ[s][i]] - v[s])) * 2**-53 /
    n_movable``. ``mass`` ``[S][N]`` integers in ``[0, 2**53]`` (exact doubles), ``succ`` ``[S][N]`` rows."""
    m = np.asarray(mass).astype(np.float64)
    v = np.asarray(v, dtype=np.float64).reshape(m.shape[0])
    t = np.asarray(succ).astype(np.int64)
    acc = (m * (v[t] - v[:, None])).sum(axis=1)
    return v + (acc * (1.0 / TWO53)) / float(n_movable)


def host_backup(mass, succ, nbr, n_movable: int, target, v, *, reward_target=20, step_cost=4, action_cost=1,
                gamma: float = 0.99, n_t=None, full: bool = False):
    """One Bellman backup of the module docstring's formula in numpy float64: ``(v_new, policy)``, or with ``full``
    ``(v_new, policy, u, ua)``. ``nbr`` ``[S][N]`` int, ``-1`` where the flip is no action (outside the set, or a node
    that is not allowed); ``target`` bool ``[S]``; ``n_t`` = ``E[1 - T]`` if the caller has it already."""
    T = np.asarray(target, dtype=bool)
    v = np.asarray(v, dtype=np.float64).reshape(T.shape[0])
    nbr = np.asarray(nbr).astype(np.int64)
    if n_t is None:
        n_t = host_expect(mass, succ, n_movable, (~T).astype(np.float64))
    h = np.where(T, float(reward_target), gamma * v - float(step_cost))
    u = host_expect(mass, succ, n_movable, h)
    ua = u - float(action_cost) * n_t
    q = np.where(nbr >= 0, ua[np.maximum(nbr, 0)], -np.inf)
    node = q.argmax(axis=1)  # the first of equal maxima: the lowest node
    best = q[np.arange(len(q)), node] if q.shape[1] else np.full(len(q), -np.inf)
    flip = best > u  # a tie keeps the no-op
    v_new = np.where(flip, best, u)
    policy = np.where(flip, node, -1).astype(np.int32)
    return (v_new, policy, u, ua) if full else (v_new, policy)


def _target_mask(graph: TransitionGraph, target) -> np.ndarray:
    """``target`` in any accepted form -> bool ``[S]`` over the graph's rows."""
    from .stateset import StateSet

    S = graph.n_states
    if isinstance(target, StateSet):
        if target.n_nodes != graph.n_nodes:
            raise ValueError(f"target set of {target.n_nodes} nodes for a graph of {graph.n_nodes}")
        return target.lookup(graph.states) >= 0
    if hasattr(target, "detach"):  # a torch tensor
        target = target.detach().cpu().numpy()
    a = np.asarray(target)
    if a.dtype == np.bool_:
        if a.shape != (S,):
            raise ValueError(f"target: a bool array [{S}], not {a.shape}")
        return a.copy()
    return rows_in(graph.states, _as_rows(a, graph.n_nodes))


class ControlSolution:
    """What :meth:`ControlProblem.solve` returns: ``v`` (float64 ``[S]``) and ``policy`` (int32 ``[S]``: ``-1`` the
    no-op, else the node to flip) on the device, ``residual`` (the last sup-norm change of a sweep: reported, never
    promised) and ``iters`` (sweeps made)."""

    def __init__(self, problem: "ControlProblem", v, policy, residual: float, iters: int):
        self.problem, self.v, self.policy = problem, v, policy
        self.residual, self.iters = float(residual), int(iters)

    def act(self, obs_words, offset: int = 0, check: bool = False):
        """Device int64 actions ``[n]`` for the states ``obs_words`` (device int64 ``[n][W]``): 0 for the no-op,
        otherwise ``node + offset`` (``PBN-v0``: offset 0, action ``a`` flips node ``a``). A state that is no row of
        the graph gets the no-op; ``check=True`` waits and raises ``ValueError`` then."""
        import torch

        rows = self.problem.graph.row_of(obs_words)
        if check and bool((rows < 0).any()):
            raise ValueError(f"{int((rows < 0).sum())} state(s) are no row of the graph")
        node = torch.where(rows >= 0, self.policy[rows.clamp(min=0).long()], torch.full_like(rows, -1))
        return torch.where(node < 0, torch.zeros_like(node), node + int(offset)).long()


class ControlProblem:
    """``ControlProblem(graph, target, *, reward_target=20, step_cost=4, action_cost=1, gamma=0.99, nodes=None,
    strict=False)``: the single-flip MDP of the module docstring over a closed :class:`TransitionGraph`.

    ``target``: a bool array ``[S]`` over the graph's rows, packed rows ``[K][W]`` uint64, state tuples, or a
    :class:`~gym_pbn_amd.stateset.StateSet` (states outside the graph are ignored). ``nodes``: the nodes an action
    may flip; the default is the graph's movable nodes, so node 0 is left out under ``table_graph="step"`` as in
    ``PBN-v0``. ``strict=True`` raises when an allowed flip leaves the set (otherwise that flip is no action at that
    state). Raises ``ValueError`` unless ``graph.closed``.
    """

    def __init__(self, graph: TransitionGraph, target, *, reward_target=20, step_cost=4, action_cost=1,
                 gamma: float = 0.99, nodes=None, strict: bool = False):
        import torch

        if graph.device is None:
            raise L.PbnError(L.PBN_E_STATE, "the transition graph is a host-only handle (device=None)")
        graph._need_closed("ControlProblem")
        if not 0.0 <= float(gamma) < 1.0:
            raise ValueError(f"gamma={gamma} outside [0, 1)")
        self.graph = graph
        self.reward_target, self.step_cost, self.action_cost = float(reward_target), float(step_cost), float(action_cost)
        self.gamma = float(gamma)
        N, S, W = graph.n_nodes, graph.n_states, graph.n_words
        if nodes is None:
            nodes = range(graph.first_node, N)
        self.nodes = sorted({int(i) for i in nodes})
        if self.nodes and not 0 <= self.nodes[0] <= self.nodes[-1] < N:
            raise ValueError(f"nodes outside [0, {N - 1}]")
        mask = np.zeros(W, dtype=np.uint64)
        for i in self.nodes:
            mask[i // 64] |= np.uint64(1) << np.uint64(i % 64)
        self.action_mask = mask
        self.target_mask = _target_mask(graph, target)
        self.device = dev = torch.device("cuda", graph.device)
        self.target = torch.from_numpy(self.target_mask).to(dev)
        self.nbr = torch.empty((S, N), dtype=torch.int32, device=dev)
        with graph._on_default_stream(dev):
            L.check(L.lib.pbn_stg_flip_rows_device(graph.handle, 0, S, L.ptr(mask, L._u64p), self.nbr.data_ptr()))
        if strict and self.nodes:
            gone = int((self.nbr[:, self.nodes] < 0).sum())
            if gone:
                raise ValueError(f"{gone} allowed flip(s) leave the state set (strict=True)")
        # nT = E[1 - T]: the probability that one update from a row does not end the episode
        self.n_t = graph.expect((~self.target).to(torch.float64))
        f64 = dict(dtype=torch.float64, device=dev)
        self._h, self._u, self._ua = (torch.empty(S, **f64) for _ in range(3))
        self._r = torch.tensor(self.reward_target, **f64)

    # ------------------------------------------------------------ one sweep
    def _values(self, v):
        """``(U, Ua)`` of ``v`` into the problem's own buffers (overwritten by the next call)."""
        import torch

        h = self._h
        torch.mul(v, self.gamma, out=h)
        h.sub_(self.step_cost)
        torch.where(self.target, self._r, h, out=h)
        self.graph._expect_into(h, self._u, self.n_t, self.action_cost, self._ua)
        return self._u, self._ua

    def _backup_into(self, v, v_new, policy):
        u, ua = self._values(v)
        L.check(L.lib.pbn_stg_backup_device(self.graph.handle, self.nbr.data_ptr(), u.data_ptr(), ua.data_ptr(),
                                            v_new.data_ptr(), policy.data_ptr()))

    def _as_v(self, v):
        import torch

        return torch.as_tensor(v, dtype=torch.float64, device=self.device).reshape(self.graph.n_states).contiguous()

    def backup(self, v):
        """One Bellman backup: ``(v_new, policy)``, fresh device tensors float64 ``[S]`` and int32 ``[S]``."""
        import torch

        v = self._as_v(v)
        v_new = torch.empty_like(v)
        policy = torch.empty(self.graph.n_states, dtype=torch.int32, device=self.device)
        with self.graph._on_default_stream(self.device):
            self._backup_into(v, v_new, policy)
        return v_new, policy

    def q_values(self, v):
        """``(U, Ua)`` of ``v`` as fresh tensors: the no-op's value at each row and the value of arriving at each row
        by a flip; ``Q(s, flip i) = Ua[nbr[s][i]]``."""
        with self.graph._on_default_stream(self.device):
            u, ua = self._values(self._as_v(v))
            return u.clone(), ua.clone()

    # ------------------------------------------------------------ fixed points
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
                if iters % check_every == 0 or iters == int(max_iters):
                    residual = float((nxt - v).abs().max())  # the only wait of a sweep
                    v, nxt = nxt, v
                    if residual <= tol:
                        break
                else:
                    v, nxt = nxt, v
        return v, residual, iters

    def solve(self, tol: float = 1e-9, max_iters: int = 100000, check_every: int = 16, v0=None) -> ControlSolution:
        """Value iteration from ``v0`` (zeros) until a sweep's sup-norm change is at most ``tol`` -- looked at every
        ``check_every`` sweeps, each look a device-to-host wait -- or ``max_iters`` sweeps were made. The policy is
        the last sweep's arg max."""
        import torch

        policy = torch.full((self.graph.n_states,), -1, dtype=torch.int32, device=self.device)
        v, residual, iters = self._iterate(lambda a, b: self._backup_into(a, b, policy), v0, tol, max_iters, check_every)
        return ControlSolution(self, v, policy, residual, iters)

    def evaluate(self, policy, tol: float = 1e-9, max_iters: int = 100000, check_every: int = 16, v0=None):
        """``(v, residual, iters)``: the value of following ``policy`` (int ``[S]``: ``-1`` the no-op, else a node),
        by iterating the backup with the action fixed. A flip the problem does not allow at its state is a
        ``ValueError``."""
        import torch

        S = self.graph.n_states
        p = torch.as_tensor(policy, device=self.device).reshape(S).long()
        if bool(((p < -1) | (p >= self.graph.n_nodes)).any()):
            raise ValueError(f"policy entries outside [-1, {self.graph.n_nodes - 1}]")
        flip = p >= 0
        to = self.nbr.gather(1, p.clamp(min=0)[:, None]).reshape(S).long()
        if bool((flip & (to < 0)).any()):
            raise ValueError(f"{int((flip & (to < 0)).sum())} state(s) are given a flip that is no action there")
        to = to.clamp(min=0)

        def sweep(v, nxt):
            u, ua = self._values(v)
            torch.where(flip, ua[to], u, out=nxt)

        return self._iterate(sweep, v0, tol, max_iters, check_every)

    # ------------------------------------------------------------ PBN-v0
    @classmethod
    def for_env(cls, env, gamma: float = 0.99, **kw) -> "ControlProblem":
        """The MDP a :class:`~gym_pbn_amd.torch_env.TorchVecPBNEnv` simulates: every state with node 0 clear (its
        resets clear node 0 and ``PBN.step`` never moves it), ``table_graph="step"``, the env's expanded target set
        and its three reward constants; actions flip nodes ``1 .. N-1``. Refuses ``N - 1 > 24``."""
        N = int(env.N)
        if N - 1 > FOR_ENV_MAX_FREE_NODES:
            raise ValueError(f"{N - 1} free nodes: for_env enumerates 2**(N - 1) states and stops at "
                             f"2**{FOR_ENV_MAX_FREE_NODES}")
        if N < 2:
            raise ValueError("PBN.step updates a node in [1, N-1]: the network needs two nodes")
        states = (np.arange(1 << (N - 1), dtype=np.uint64) << np.uint64(1)).reshape(-1, 1)
        graph = TransitionGraph(env.net, states, table_graph="step", device=env.device.index)
        kw.setdefault("reward_target", env.REWARD_TARGET)
        kw.setdefault("step_cost", env.STEP_COST)
        kw.setdefault("action_cost", env.ACTION_COST)
        return cls(graph, np.ascontiguousarray(env.target_words, dtype=np.uint64), gamma=gamma, **kw)


__all__ = ["ControlProblem", "ControlSolution", "host_backup", "host_expect", "FOR_ENV_MAX_FREE_NODES"]
