"""Device-resident vectorised multi-flip env for agents on the GPU (torch tensors in and out).

``PBNTargetMultiEnv.step`` (``pbn_target_multi.py:119-154``) takes a torch action tensor and
de-duplicates it with ``actions.unique()`` (``:120-121``): the reference is written for a
torch agent (BDQ branches). Here the B envs, the agent's action tensor and every output stay
on the GPU: the batch runs on torch's current stream (``pbn_batch_set_stream``), so the R6
kernel orders with the policy's kernels without a host sync, and nothing crosses PCIe per
step. Observations are unpacked from the packed state words by a small kernel (one byte per
node, ``pbn_unpack_bits_device``).

Same transition, reward, termination and truncation as :class:`gym_pbn_amd.envs.VecPBNTargetMultiEnv`
(one R6 launch per call; Philox draws keyed by the global env id); ``auto_reset`` resets the
envs that ended, on the device, after their outputs were written (SB3 VecEnv convention; the
reference env never resets itself).

:class:`TorchVecPBNEnv` is the same for the ``PBN-v0`` MDP of truth-table networks (``pbn_env.py:125-188``): the
device twin of :class:`gym_pbn_amd.envs.VecPBNEnv`, one fused launch per step over an exact device set of target
states (:mod:`gym_pbn_amd.stateset`).
"""

from __future__ import annotations

from . import _lib as L
from . import spaces
from .batch import EnvConfig, Net, PBNBatch
from .network import PredictorNetwork, load_network


class _TorchVecBase:
    """What the device-resident envs share: a :class:`PBNBatch` on torch's current stream, the conversions between
    torch tensors and what the launches read and write, and ``close``. A subclass sets ``batch``, ``device``,
    ``num_envs``, ``N``, ``W`` and lists the state sets it owns in ``_sets``."""

    _sets = ()

    def _use_stream(self):
        import torch

        self.batch.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def _bits(self, words=None):
        """[B][N] uint8 node values (k_unpack) from packed words [B][W] (None = the live state)."""
        import torch

        out = torch.empty((self.num_envs, self.N), dtype=torch.uint8, device=self.device)
        self.batch.unpack_bits_device(out.data_ptr(), 0 if words is None else words.data_ptr())
        return out

    def observation_words(self):
        """The live state as packed words ``[B][W]`` int64: a fresh device tensor per call."""
        import torch

        self._use_stream()
        words = torch.empty((self.num_envs, self.W), dtype=torch.int64, device=self.device)
        self.batch.get_state_device(words.data_ptr())
        return words

    def _mask(self, mask):
        """A reset mask (None: every env) as the uint8 tensor a launch reads, or None."""
        import torch

        if mask is None:
            return None
        # same stream as the kernel: the allocator cannot hand the copy's memory out before it ran
        return mask.to(device=self.device, dtype=torch.uint8).contiguous()

    def _actions(self, actions, two_d: bool):
        """``actions`` as a contiguous int32 device tensor with one row per env: ``[B][A]`` (``two_d``; ``[B]`` is
        taken as ``A = 1``) or ``[B]``."""
        import torch

        a = actions
        if two_d and a.dim() == 1:
            a = a.unsqueeze(1)
        a = a.to(device=self.device, dtype=torch.int32).contiguous()
        if not two_d:
            a = a.reshape(-1)
        if a.shape[0] != self.num_envs:
            raise ValueError(f"actions for {a.shape[0]} envs, the batch has {self.num_envs}")
        return a

    @staticmethod
    def _decode_flags(flags):
        """The flag bytes a step launch wrote -> ``(terminated, truncated, capped)`` bool tensors."""
        return (flags & L.FLAG_TERMINATED) != 0, (flags & L.FLAG_TRUNCATED) != 0, (flags & L.FLAG_CAPPED) != 0

    def close(self):
        import torch

        torch.cuda.current_stream(self.device).synchronize()
        self.batch.set_stream(None)
        self.batch.close()
        for s in self._sets:
            s.close()


class TorchVecPBNTargetMultiEnv(_TorchVecBase):
    def __init__(self, network, attractors, n_envs: int, horizon: int = 100, device: int = 0, seed: int = 0,
                 env_id_base: int = 0, update_cap: int = 1 << 20, auto_reset: bool = False):
        import torch

        if not isinstance(network, (PredictorNetwork, Net)):
            network = load_network(network)
        self.net = network if isinstance(network, Net) else Net(network)
        self.num_envs = int(n_envs)
        self.N, self.W = self.net.n_nodes, self.net.n_words
        self.device = torch.device("cuda", device)
        self.cfg = EnvConfig(self.net, attractors, horizon=horizon)
        self.batch = PBNBatch(self.net, self.num_envs, device=device, env_id_base=env_id_base, seed=seed)
        self.update_cap = int(update_cap)
        self.auto_reset = bool(auto_reset)
        self.observation_space = spaces.MultiBinary(self.N)  # pbn_target_multi.py:56-59
        self.action_space = spaces.MultiDiscrete(self.N + 1)
        B = self.num_envs
        with torch.cuda.device(self.device):
            self._reward = torch.empty(B, dtype=torch.int32, device=self.device)
            self._flags = torch.empty(B, dtype=torch.uint8, device=self.device)
            self._nup = torch.empty(B, dtype=torch.int32, device=self.device)
        self._use_stream()

    def reset(self, mask=None):
        """Reset every env (``mask`` None) or the envs where the device bool/uint8 ``mask`` is set
        (``reset``, :227-259, Philox draws); returns observations [B][N] uint8 on the device."""
        self._use_stream()
        m = self._mask(mask)
        self.batch.env_reset_device(self.cfg, 0 if m is None else m.data_ptr())
        return self._bits()

    def step(self, actions):
        """``actions``: int tensor [B] or [B][A] of node + 1 values (0 = none), on the GPU.
        Returns ``(obs [B][N] uint8, reward [B] int32, terminated [B] bool, truncated [B] bool,
        info)`` as device tensors; ``info`` holds ``n_updates``, ``capped`` and ``obs_words``."""
        import torch

        a = self._actions(actions, two_d=True)
        self._use_stream()
        words = torch.empty((self.num_envs, self.W), dtype=torch.int64, device=self.device)
        self.batch.env_step_multi_device(self.cfg, a.data_ptr(), a.shape[1], words.data_ptr(),
                                         self._reward.data_ptr(), self._flags.data_ptr(), self._nup.data_ptr(),
                                         offset=1, dedup=True, update_cap=self.update_cap)
        term, trunc, capped = self._decode_flags(self._flags)
        info = {"n_updates": self._nup.clone(), "capped": capped, "obs_words": words}
        obs = self._bits(words)
        reward = self._reward.clone()
        if self.auto_reset:
            done = (term | trunc).to(torch.uint8).contiguous()
            self.batch.env_reset_device(self.cfg, done.data_ptr())
        return obs, reward, term, trunc, info


def _packed_attractors(network, net, all_attractors, device: int, seed: int):
    """``all_attractors`` in any accepted form -> a list of packed ``[S_k][W]`` uint64 arrays (no tuples made
    for the forms that are packed already)."""
    import numpy as np

    from .attractors import AttractorResult, find_attractors
    from .batch import pack_bits

    W = network.n_words
    if all_attractors is None:  # the full STG, as PBNEnv / VecPBNEnv (pbn_env.py:54)
        from .stg import compute_attractors

        all_attractors = compute_attractors(network)
    elif isinstance(all_attractors, str):
        if all_attractors != "find":
            raise ValueError(f"all_attractors={all_attractors!r}: a list, an AttractorResult, \"find\" or None")
        res = find_attractors(net, device=device, seed=seed, table_graph="stg")
        if not res.attractors:
            raise RuntimeError(f"no attractor fits the state set: {len(res.incomplete)} closure(s) ran past max_states")
        if res.incomplete:
            import warnings

            warnings.warn(f"{sum(e['n_seeds'] for e in res.incomplete)} seed(s) ended in closures past max_states; "
                          "the env uses the attractors that were enumerated")
        all_attractors = res
    if isinstance(all_attractors, AttractorResult):
        if all_attractors.n_nodes != network.n_nodes:
            raise ValueError(f"attractors of {all_attractors.n_nodes} nodes for a network of {network.n_nodes}")
        all_attractors = all_attractors.attractors
    out = []
    for a in all_attractors:
        if isinstance(a, np.ndarray) and a.dtype == np.uint64:
            out.append(np.ascontiguousarray(a).reshape(-1, W))
        else:  # state tuples, node 0 first
            bits = np.array([tuple(int(v) for v in s) for s in a], dtype=np.uint8).reshape(-1, network.n_nodes)
            out.append(pack_bits(bits).reshape(-1, W))
    if not out or not all(len(a) for a in out):
        raise ValueError("need at least one non-empty attractor")
    return out


class TorchVecPBNEnv(_TorchVecBase):
    """B copies of the ``PBN-v0`` MDP (``pbn_env.py:125-188``) resident on the device: the twin of
    :class:`gym_pbn_amd.envs.VecPBNEnv` for agents on the GPU.

    ``step(actions)`` takes an int tensor ``[B]`` on the device (0 = no action, ``a`` flips node ``a``) and is one
    launch (``pbn_tenv_step_device``): flip, one ``PBN.step`` update, membership of the new state in the target
    set, reward and flags; it returns device tensors ``(obs [B][N] uint8, reward [B] int32, terminated [B] bool,
    truncated [B] bool, info)`` with ``info["obs_words"]`` (packed ``[B][W]`` int64) and ``info["label"]`` (the
    target set's label of each env's state, -1 outside). Nothing crosses PCIe per step, and the attractors may
    hold up to ``2**24`` states (the host envs keep Python sets and stop at ``2**16``).

    Same transitions, rewards (the reference's literals 20 / -4 / -1) and termination as ``VecPBNEnv`` for the
    same seed. ``reset`` and ``auto_reset`` draw from the attracting states on the device
    (``pbn_tenv_reset_device``: Philox stream 9, counter ``{0, reset_count, global env id}``, row =
    ``mulhi(word 0, n)``), so their picks differ from ``VecPBNEnv``'s host ``default_rng`` draws: a documented
    stream of its own.

    ``all_attractors``: ``None`` (the full STG, up to 22 nodes); a list of attractors, each a list of state
    tuples or a packed ``[S][W]`` uint64 array; an :class:`~gym_pbn_amd.attractors.AttractorResult`; or
    ``"find"`` (:func:`~gym_pbn_amd.attractors.find_attractors` on the ``"stg"`` graph, no limit on their
    size but the set's). The target set is ``goal_config["target_nodes"]`` united with every attractor that
    meets it (``pbn_env.py:57-59``).
    """

    REWARD_TARGET, STEP_COST, ACTION_COST = 20, 4, 1  # pbn_env.py:156-188

    def __init__(self, PBN_data=None, logic_func_data=None, goal_config=None, n_envs: int = 1, *,
                 all_attractors=None, device: int = 0, seed: int = 0, env_id_base: int = 0, auto_reset: bool = False):
        import numpy as np
        import torch

        from .attractors import rows_in
        from .batch import pack_bits
        from .network import TruthTableNetwork
        from .stateset import StateSet

        if PBN_data is not None and len(PBN_data) != 0:
            net = TruthTableNetwork.from_pbn_data(PBN_data)
        elif logic_func_data is not None:
            net = TruthTableNetwork.from_logic_funcs(*logic_func_data)
        else:
            raise ValueError("TorchVecPBNEnv needs PBN_data or logic_func_data")
        if goal_config is None or "target_nodes" not in goal_config:
            raise KeyError("target_nodes")  # pbn_env.py:51
        self.network = net
        self.net = Net(net)
        self.N, self.W = net.n_nodes, net.n_words
        self.num_envs = int(n_envs)
        self.device = torch.device("cuda", device)
        self.attractors = _packed_attractors(net, self.net, all_attractors, device, seed)
        # target expansion on packed rows (pbn_env.py:57-59): the union of the target and every attractor meeting it
        tn = [tuple(int(v) for v in s) for s in goal_config["target_nodes"]]
        base = pack_bits(np.array(tn, dtype=np.uint8).reshape(-1, self.N)).reshape(-1, self.W)
        parts = [base] + [a for a in self.attractors if rows_in(a, base).any()]
        target = np.unique(np.concatenate(parts), axis=0)
        self.target_words = target
        self.target = StateSet(target, self.N, device=device)
        self._sets = (self.target,)
        attracting = np.unique(np.concatenate(self.attractors), axis=0)
        self.n_attracting = int(attracting.shape[0])
        self.batch = PBNBatch(self.net, self.num_envs, device=device, env_id_base=env_id_base, seed=seed)
        self.auto_reset = bool(auto_reset)
        self.observation_space = spaces.bool_multibinary(self.N)  # pbn_env.py:81-83
        self.action_space = spaces.Discrete(self.N)
        B = self.num_envs
        with torch.cuda.device(self.device):
            # uploaded once: the table reset and auto-reset draw from
            self._attracting = torch.from_numpy(attracting.view(np.int64)).to(self.device).contiguous()
            self._flags = torch.empty(B, dtype=torch.uint8, device=self.device)
        self._use_stream()

    def info(self) -> dict:
        """The target set's ``pbn_stateset_info`` (``n_states``, ``table_slots``, ``max_probe``, ...) and
        ``n_attracting``, the number of attracting states reset draws from."""
        d = self.target.info()
        d["n_attracting"] = self.n_attracting
        return d

    def reset(self, mask=None):
        """Every env (``mask`` None) or the envs where the device bool / uint8 ``mask`` is set take a state drawn
        uniformly from the attracting set, node 0 cleared (``PBN.reset``, ``pbn.py:118``); returns observations
        ``[B][N]`` uint8 on the device."""
        self._use_stream()
        self._reset(self._mask(mask))
        return self._bits()

    def _reset(self, m):
        self.batch.tenv_reset_device(self._attracting.data_ptr(), self.n_attracting, 0 if m is None else m.data_ptr())

    def _finish(self, words):
        """A step's tail once its launch wrote ``words`` and the flags: ``(obs, terminated, truncated)``, then the
        auto-reset of the envs that ended (``PBN-v0`` and the macro envs never truncate)."""
        import torch

        term = self._decode_flags(self._flags)[0]
        trunc = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        obs = self._bits(words)
        if self.auto_reset:
            self._reset(term.to(torch.uint8).contiguous())
        return obs, term, trunc

    def step(self, actions, check: bool = False):
        """``actions``: int tensor ``[B]`` on the GPU, values in ``[0, N-1]``. An env given any other value is left
        untouched, outputs included; ``check=True`` waits for the launch and raises ``ValueError`` then (the
        default stays asynchronous, and a later checked call reports)."""
        import torch

        a = self._actions(actions, two_d=False)
        self._use_stream()
        B = self.num_envs
        words = torch.empty((B, self.W), dtype=torch.int64, device=self.device)
        reward = torch.empty(B, dtype=torch.int32, device=self.device)
        label = torch.empty(B, dtype=torch.int32, device=self.device)
        self.batch.tenv_step_device(self.target, a.data_ptr(), reward.data_ptr(), self._flags.data_ptr(),
                                    d_obs=words.data_ptr(), d_labels=label.data_ptr(),
                                    reward_target=self.REWARD_TARGET, step_cost=self.STEP_COST,
                                    action_cost=self.ACTION_COST, check=check)
        obs, term, trunc = self._finish(words)
        return obs, reward, term, trunc, {"obs_words": words, "label": label}


def labelled_attractors(network, attractors, net=None, device: int = 0, seed: int = 0):
    """``attractors`` in any form :class:`TorchVecPBNTargetMultiSetEnv` accepts -> ``(rows, labels, row_off)``: the
    attractors' states as packed ``[S][W]`` uint64 rows ordered by label (= the attractor's index), their labels
    ``[S]`` int32 and ``row_off`` ``[K + 1]`` uint32, attractor ``k`` owning rows ``row_off[k] .. row_off[k + 1] - 1``.
    Host only unless ``attractors == "find"`` (which needs ``net`` and a device).

    An attractor given as cube tuples (ints and ``'*'``) is expanded (``expand_cubes``, overlapping cubes united);
    the expansion is counted first and refused with ``ValueError`` when the set would pass ``STATESET_MAX_STATES``."""
    import numpy as np

    from .attractors import AttractorResult, expand_cubes

    N = network.n_nodes
    if attractors is None:
        raise ValueError("attractors: an AttractorResult, \"find\", or a list of attractors")
    if not isinstance(attractors, (str, AttractorResult)):
        items, total = [], 0
        for a in attractors:
            if not isinstance(a, np.ndarray) and any(v == "*" for c in a for v in c):
                total += sum(1 << sum(1 for v in c if v == "*") for c in a)
                if total > L.STATESET_MAX_STATES:
                    raise ValueError(f"the cubes expand to more than STATESET_MAX_STATES = {L.STATESET_MAX_STATES} "
                                     "states; keep them as cubes (TorchVecPBNTargetMultiEnv)")
                a = np.unique(expand_cubes([tuple(c) for c in a], N), axis=0)
            items.append(a)
        attractors = items
    packed = _packed_attractors(network, net, attractors, device, seed)
    rows = np.ascontiguousarray(np.concatenate(packed), dtype=np.uint64)
    if len(rows) > L.STATESET_MAX_STATES:
        raise ValueError(f"{len(rows)} attracting states: more than STATESET_MAX_STATES = {L.STATESET_MAX_STATES}")
    labels = np.concatenate([np.full(len(a), k, np.int32) for k, a in enumerate(packed)])
    row_off = np.concatenate([[0], np.cumsum([len(a) for a in packed])]).astype(np.uint32)
    return rows, labels, row_off


class TorchVecPBNTargetMultiSetEnv(_TorchVecBase):
    """:class:`TorchVecPBNTargetMultiEnv` over attractors given as exact state lists: one labelled
    :class:`~gym_pbn_amd.stateset.StateSet` (label = the attractor's index) takes the place of the cubes, so an
    attractor may have any shape and up to ``2**24`` states in all, ``info["label"]`` says which attractor each env
    landed in, and every env has a source attractor (where ``reset`` puts it) and a target attractor (where
    ``terminated`` is raised) of its own -- the ``state_attractor_id, target_attractor_id`` the reference's ``reset``
    draws per episode (``pbn_target_multi.py:232-235``). The defaults are what the reference then does: source
    attractor 0, target attractor ``K - 1``.

    ``network``: a bundled name, a ``PredictorNetwork``, a ``TruthTableNetwork`` or a ``Net``. ``attractors``: an
    :class:`~gym_pbn_amd.attractors.AttractorResult`; ``"find"``; or a list of attractors, each a packed ``[S][W]``
    uint64 array, a list of state tuples, or a list of cube tuples (expanded; refused past ``2**24`` states).

    ``step`` is one launch (``pbn_env_set_step_device``) with the same draws as ``TorchVecPBNTargetMultiEnv`` for the
    same seed; ``reset`` draws a state of the source attractor on the device (Philox stream 9, as ``TorchVecPBNEnv``).
    """

    def __init__(self, network, attractors, n_envs: int, horizon: int = 100, device: int = 0, seed: int = 0,
                 env_id_base: int = 0, update_cap: int = 1 << 20, auto_reset: bool = False,
                 reward_success: int = 1000, action_cost: int = 1):
        import numpy as np
        import torch

        from .network import TruthTableNetwork
        from .stateset import StateSet

        if not isinstance(network, (PredictorNetwork, TruthTableNetwork, Net)):
            network = load_network(network)
        self.net = network if isinstance(network, Net) else Net(network)
        self.network = self.net.network
        self.num_envs = int(n_envs)
        self.N, self.W = self.net.n_nodes, self.net.n_words
        self.device = torch.device("cuda", device)
        rows, labels, row_off = labelled_attractors(self.network, attractors, self.net, device, seed)
        self.n_attractors = len(row_off) - 1
        self.row_off = row_off
        self.set = StateSet(rows, self.N, labels=labels, device=device)
        self._sets = (self.set,)
        self.horizon, self.update_cap = int(horizon), int(update_cap)
        self.reward_success, self.action_cost = int(reward_success), int(action_cost)
        self.auto_reset = bool(auto_reset)
        self.batch = PBNBatch(self.net, self.num_envs, device=device, env_id_base=env_id_base, seed=seed)
        self.observation_space = spaces.MultiBinary(self.N)  # pbn_target_multi.py:56-59
        self.action_space = spaces.MultiDiscrete(self.N + 1)
        B = self.num_envs
        with torch.cuda.device(self.device):
            # uploaded once: the table reset and auto-reset draw from
            self._rows = torch.from_numpy(rows.view(np.int64)).to(self.device).contiguous()
            self._row_off = torch.from_numpy(row_off.view(np.int32)).to(self.device).contiguous()
            self.source = torch.zeros(B, dtype=torch.int32, device=self.device)
            self.target = torch.full((B,), self.n_attractors - 1, dtype=torch.int32, device=self.device)
            self._flags = torch.empty(B, dtype=torch.uint8, device=self.device)
        self._use_stream()

    def _assign(self, held, value, m):
        """``held[e] = value[e]`` (an int or a device int tensor ``[B]``) for the envs of mask ``m`` (None: all)."""
        import torch

        if value is None:
            return
        if torch.is_tensor(value):
            v = value.to(device=self.device, dtype=torch.int32).reshape(-1)
            if v.shape[0] != self.num_envs:
                raise ValueError(f"labels for {v.shape[0]} envs, the batch has {self.num_envs}")
        else:
            if not 0 <= int(value) < self.n_attractors:
                raise ValueError(f"attractor {value} outside [0, {self.n_attractors})")
            v = torch.full_like(held, int(value))
        if m is None:
            held.copy_(v)
        else:
            held.copy_(torch.where(m != 0, v, held))

    def _reset(self, m):
        self.batch.env_set_reset_device(self._rows.data_ptr(), self._row_off.data_ptr(), self.n_attractors,
                                        d_source_labels=self.source.data_ptr(),
                                        d_mask=0 if m is None else m.data_ptr())

    def reset(self, mask=None, source=None, target=None):
        """Every env (``mask`` None) or the envs where the device bool / uint8 ``mask`` is set take a state drawn
        uniformly from their source attractor and ``n_steps = 0``. ``source`` / ``target``: an int or a device int
        tensor ``[B]`` of attractor indices, stored for the envs being reset and kept until their next reset that
        names one. An env whose source is no attractor is left as it is (``batch.env_set_check()`` reports it).
        Returns observations ``[B][N]`` uint8 on the device."""
        self._use_stream()
        m = self._mask(mask)
        self._assign(self.source, source, m)
        self._assign(self.target, target, m)
        self._reset(m)
        return self._bits()

    def step(self, actions):
        """``actions``: int tensor ``[B]`` or ``[B][A]`` of node + 1 values (0 = none), on the GPU. Returns ``(obs
        [B][N] uint8, reward [B] int32, terminated [B] bool, truncated [B] bool, info)`` as device tensors; ``info``
        holds ``n_updates``, ``capped``, ``obs_words`` and ``label`` (the attractor the env landed in, -1 when
        capped); ``terminated`` is ``label == target`` of the env."""
        import torch

        a = self._actions(actions, two_d=True)
        self._use_stream()
        B = self.num_envs
        words = torch.empty((B, self.W), dtype=torch.int64, device=self.device)
        reward = torch.empty(B, dtype=torch.int32, device=self.device)
        nup = torch.empty(B, dtype=torch.int32, device=self.device)
        label = torch.empty(B, dtype=torch.int32, device=self.device)
        self.batch.env_set_step_device(self.set, a.data_ptr(), a.shape[1], words.data_ptr(), reward.data_ptr(),
                                       self._flags.data_ptr(), nup.data_ptr(), label.data_ptr(),
                                       d_target_labels=self.target.data_ptr(), offset=1, dedup=True,
                                       update_cap=self.update_cap, horizon=self.horizon,
                                       reward_success=self.reward_success, action_cost=self.action_cost)
        term, trunc, capped = self._decode_flags(self._flags)
        info = {"n_updates": nup, "capped": capped, "obs_words": words, "label": label}
        obs = self._bits(words)
        if self.auto_reset:
            self._reset((term | trunc).to(torch.uint8).contiguous())
        return obs, reward, term, trunc, info


__all__ = ["TorchVecPBNTargetMultiEnv", "TorchVecPBNEnv", "TorchVecPBNTargetMultiSetEnv", "labelled_attractors"]
