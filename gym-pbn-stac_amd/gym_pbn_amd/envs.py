"""Drop-in env surfaces over the device batch (gym_PBN.envs conventions).

* :class:`Graph`            -- ``gym_PBN/envs/bittner/base.py`` ``Graph`` (step/flipNode/setState/getState/...).
* :class:`PBN`              -- ``gym_PBN/envs/common/pbn.py`` ``PBN`` (reset/flip/step/state).
* :class:`PBNTargetEnv`     -- ``gym_PBN/envs/pbn_target.py`` single-flip target env (R5, intended semantics).
* :class:`PBNTargetMultiEnv` -- ``gym_PBN/envs/pbn_target_multi.py`` single env (reset/step, R6).
* :class:`VecPBNTargetMultiEnv` -- the same MDP over B envs in one call (Stable-Baselines3 VecEnv shaped).
* :class:`PBNEnv`           -- ``gym_PBN/envs/pbn_env.py`` ``PBNEnv`` step/reward conventions (R7).

Every transition runs on the GPU through libpbnsim (Philox mode). Return
conventions follow the reference: observations of the multi env are tuples,
rewards ints, ``info["observation_idx"]`` the state as an int with node 0 as
the most significant bit (``pbn_target_multi.py:295-298``).
"""

from __future__ import annotations

import random
from collections import deque
from typing import Optional

import numpy as np

from . import spaces
from . import _lib as L
from .attractors import find_state_attractors, resolve_all_attractors
from .batch import EnvConfig, Net, PBNBatch, pack_bits, unpack_bits
from .network import PredictorNetwork, TruthTableNetwork, load_network


def state_to_idx(bits) -> int:
    """``int("".join(str(x) for x in state), 2)`` (pbn_target_multi.py:295-298)."""
    v = 0
    for x in bits:
        v = (v << 1) | int(x)
    return v


class Graph:
    """Single-env mirror of ``base.Graph`` backed by a one-env device batch."""

    def __init__(self, network, device: int = 0, seed: int = 0, env_id: int = 0):
        if not isinstance(network, PredictorNetwork):
            network = load_network(network)
        self.network = network
        self._b = PBNBatch(Net(network), 1, device=device, env_id_base=env_id, seed=seed)
        self._initialised = False

    @property
    def N(self) -> int:  # base.py:195-197
        return self.network.n_nodes

    def getIDs(self):  # base.py:332-334
        return [int(x) for x in self.network.node_ids]

    def genRandState(self):  # base.py:368-370
        self._b.randomize()
        self._initialised = True

    def setState(self, state):  # base.py:364-366
        bits = np.array([int(x) for x in state], dtype=np.uint8)
        if bits.shape[0] != self.N:
            raise ValueError(f"state has {bits.shape[0]} values, graph has {self.N} nodes")
        self._b.set_bits(bits[None])
        self._initialised = True

    def getState(self) -> tuple:  # base.py:320-324
        return tuple(self._b.get_bits()[0].tolist())

    def getLabeledState(self) -> dict:  # base.py:314-318
        return dict(zip(self.getIDs(), self.getState()))

    def flipNode(self, index: int):  # base.py:280-284
        if index >= self.N:
            raise ValueError(f"Invalid action, no node at index {index}")
        self._b.flip(np.array([[index + 1]], dtype=np.int32), offset=1, dedup=True)

    def step(self, changed_nodes=None, i=None) -> tuple:  # base.py:306-312 (changed_nodes is ignored there too)
        if not self._initialised:
            raise Exception("Forgot to initialise the states")  # base.py:90-91
        if i is None:
            self._b.step(1)
        else:
            # base.py:307-309: `self.nodes[i]` -- Python list indexing (negative i counts from the
            # end, anything else out of range raises IndexError); no node draw is made, the
            # predictor choice is this update's Philox choice draw
            i = int(i)
            if not -self.N <= i < self.N:
                raise IndexError("list index out of range")
            self._b.step_forced(np.array([[i % self.N]], dtype=np.uint32))
        return self.getState()


class PBN:
    """Single-env mirror of ``common.pbn.PBN`` (truth-table engine).

    Built from ``PBN_data`` or ``logic_func_data = (nodes, node_functions)``
    (``pbn.py:15-51``). ``queue_replay(node_idx, k53)`` makes the next steps use the
    reference's own draws (``randint(1, N-1)`` and ``uniform(0, 1) * 2**53``)
    instead of the Philox stream -- the parity hook the env tests use.
    """

    def __init__(self, PBN_data=None, logic_func_data=None, network: Optional[TruthTableNetwork] = None,
                 device: int = 0, seed: int = 0, env_id: int = 0):
        if network is None:
            network = self.table_network(PBN_data, logic_func_data)
        self.network = network
        self.N = network.n_nodes
        self._device, self._env_id = device, env_id
        self._b = PBNBatch(Net(network), 1, device=device, env_id_base=env_id, seed=seed)
        self._replay: deque = deque()

    @staticmethod
    def table_network(PBN_data=None, logic_func_data=None) -> TruthTableNetwork:
        """The network of the constructor's arguments (``pbn.py:15-51``), without a device."""
        if PBN_data is not None and len(PBN_data) != 0:
            return TruthTableNetwork.from_pbn_data(PBN_data)
        if logic_func_data is not None:
            return TruthTableNetwork.from_logic_funcs(*logic_func_data)
        raise ValueError("PBN needs PBN_data or logic_func_data")

    @property
    def state(self) -> np.ndarray:
        return self._b.get_bits()[0].astype(bool)

    def reseed(self, seed: int) -> None:
        """Re-key the Philox stream (state kept): the device side of ``random.seed`` / ``np.random.seed``."""
        words = self._b.get_state()
        self._b.close()
        self._b = PBNBatch(Net(self.network), 1, device=self._device, env_id_base=self._env_id, seed=int(seed))
        self._b.set_state(words)

    def queue_replay(self, node_idx, k53) -> None:
        self._replay.extend(zip((int(i) for i in node_idx), (int(k) for k in k53)))

    def reset(self, state=None) -> np.ndarray:  # pbn.py:96-119
        if state is None:
            self._b.randomize()  # also clears node 0
        else:
            if len(state) != self.N:
                raise Exception(
                    f"The length of the state given ({len(state)}) is different from the PBN size ({self.N})."
                )
            bits = np.array(state, dtype=bool).astype(np.uint8)
            bits[0] = 0
            self._b.set_bits(bits[None])
        return self.state

    def flip(self, index: int):  # pbn.py:121-127
        if not (-self.N <= index < self.N):
            raise IndexError(index)
        # action value v flips node v - 1 (value 0 means "no action", so node 0 needs offset 1)
        self._b.flip(np.array([[index % self.N + 1]], dtype=np.int32), offset=1, dedup=True)

    def step(self):  # pbn.py:129-133
        if self._replay:
            i, k = self._replay.popleft()
            self._b.step_replay(np.array([[i]], np.uint32), np.array([[k]], np.uint64))
        else:
            self._b.step(1)


class VecPBNEnv:
    """B copies of the ``PBN-v0`` MDP (``pbn_env.py:125-188``) stepped in one launch.

    ``step(actions)`` takes ``[B]`` ints: node ``a`` is flipped when ``a != 0`` (``PBNEnv``
    flips ``action``, not ``action - 1``, :141-142), then one ``PBN.step`` (R4) per env;
    reward +20 and terminated when the state is in ``target_nodes`` (expanded by the
    attractors that meet it, :57-59), else -4 and another -1 for an action; truncated
    is always False. Rewards are computed on the host from the packed states.
    ``all_attractors``: as for :class:`PBNEnv` (``None``: the full STG; ``"find"``: device
    discovery; a list: taken as given).
    ``auto_reset`` resets ended envs to a state drawn uniformly from the attracting set
    (SB3 VecEnv convention; the reference env never resets itself).
    """

    def __init__(self, PBN_data=None, logic_func_data=None, goal_config=None, n_envs: int = 1, *,
                 all_attractors=None, device: int = 0, seed: int = 0, env_id_base: int = 0, auto_reset: bool = False):
        if PBN_data is not None and len(PBN_data) != 0:
            net = TruthTableNetwork.from_pbn_data(PBN_data)
        else:
            net = TruthTableNetwork.from_logic_funcs(*logic_func_data)
        self.network = net
        self.N = net.n_nodes
        self.num_envs = int(n_envs)
        if all_attractors is None:
            from .stg import compute_attractors

            all_attractors = compute_attractors(net)
        elif isinstance(all_attractors, str) and all_attractors == "find":  # opt-in: found on the device
            all_attractors = find_state_attractors(net, device=device, seed=seed)
        self.all_attractors = [set(tuple(int(v) for v in s) for s in a) for a in all_attractors]
        target = set(goal_config["target_nodes"])
        for attractor in self.all_attractors:
            if target & attractor:
                target |= attractor
        self.target_nodes = target
        self._target_words = np.unique(pack_bits(np.array(sorted(target), np.uint8)), axis=0) if target else None
        self._attracting = np.array(sorted(set.union(*self.all_attractors)), np.uint8)
        self.batch = PBNBatch(Net(net), self.num_envs, device=device, env_id_base=env_id_base, seed=seed)
        self.auto_reset = auto_reset
        self._rng = np.random.default_rng(seed)
        # per-env spaces, as PBNEnv's (pbn_env.py:81-83)
        self.observation_space = spaces.bool_multibinary(self.N)
        self.action_space = spaces.Discrete(self.N)

    def _in_target(self, words) -> np.ndarray:
        if self._target_words is None:
            return np.zeros(words.shape[0], bool)
        W = words.shape[1]
        key = np.ascontiguousarray(words).view(np.dtype((np.void, 8 * W))).ravel()
        tk = np.ascontiguousarray(self._target_words).view(np.dtype((np.void, 8 * W))).ravel()
        return np.isin(key, tk)

    def reset(self, mask=None) -> np.ndarray:
        """States drawn uniformly from the attracting set (node 0 cleared as PBN.reset does)."""
        m = np.ones(self.num_envs, bool) if mask is None else np.asarray(mask, bool)
        bits = self.batch.get_bits()
        pick = self._attracting[self._rng.integers(0, len(self._attracting), size=self.num_envs)]
        bits[m] = pick[m]
        bits[:, 0] = 0
        self.batch.set_bits(bits)
        return bits

    def step(self, actions):
        a = np.asarray(actions, dtype=np.int64).reshape(self.num_envs)
        if (a < 0).any() or (a >= self.N).any():
            raise Exception("Invalid action, not in action space.")  # pbn_env.py:138-139
        if (a != 0).any():
            self.batch.flip((a + 1).astype(np.int32)[:, None] * (a != 0)[:, None], offset=1, dedup=True)
        self.batch.step(1)
        words = self.batch.get_state()
        term = self._in_target(words)
        reward = np.where(term, 20, -4 - (a != 0).astype(np.int64)).astype(np.int64)
        trunc = np.zeros(self.num_envs, bool)
        obs = unpack_bits(words, self.N)
        if self.auto_reset and term.any():
            self.reset(term)
        return obs, reward, term, trunc, {"obs_words": words}


class VecPBNTargetMultiEnv:
    """B copies of the multi-flip until-attractor MDP (pbn_target_multi.py:119-259) in one launch.

    ``step(actions)`` takes ``[B][A]`` int actions (node+1, 0 = none; de-duplicated
    per row like a torch tensor input) and returns numpy arrays
    ``(obs [B][N] uint8, reward [B] int32, terminated [B] bool, truncated [B] bool, info)``
    with ``info["n_updates"]`` (node updates per env) and ``info["capped"]``.
    ``auto_reset`` resets envs that ended (SB3 VecEnv semantics); the reference
    env itself never resets on its own.
    """

    def __init__(self, network, attractors, n_envs: int, horizon: int = 100, device: int = 0, seed: int = 0,
                 env_id_base: int = 0, update_cap: int = 1 << 20, auto_reset: bool = False):
        net = network if isinstance(network, Net) else Net(network)
        self.net = net
        self.num_envs = int(n_envs)
        self.N = net.n_nodes
        # "find": discovered on the device (gym_pbn_amd.attractors), opt-in
        attractors = resolve_all_attractors(net, attractors, device=device, seed=seed)
        self.cfg = EnvConfig(net, attractors, horizon=horizon)
        self.batch = PBNBatch(net, n_envs, device=device, env_id_base=env_id_base, seed=seed)
        self.update_cap = int(update_cap)
        self.auto_reset = auto_reset
        # per-env spaces, as PBNTargetMultiEnv's (pbn_target_multi.py:56-59)
        self.observation_space = spaces.MultiBinary(self.N)
        self.action_space = spaces.MultiDiscrete(self.N + 1)

    def reset(self, mask=None) -> np.ndarray:
        self.batch.env_reset(self.cfg, mask)
        return self.batch.get_bits()

    def step(self, actions):
        a = np.asarray(actions)
        if a.ndim == 1:
            a = a[:, None]
        obs, rew, flags, nup = self.batch.env_step_multi(self.cfg, a, offset=1, dedup=True,
                                                         update_cap=self.update_cap)
        term = (flags & L.FLAG_TERMINATED) != 0
        trunc = (flags & L.FLAG_TRUNCATED) != 0
        info = {"n_updates": nup, "capped": (flags & L.FLAG_CAPPED) != 0, "obs_words": obs}
        if self.auto_reset and (term | trunc).any():
            self.batch.env_reset(self.cfg, (term | trunc).astype(np.uint8))
        return unpack_bits(obs, self.N), rew, term, trunc, info


class PBNTargetMultiEnv:
    """Single-env mirror of ``PBNTargetMultiEnv`` with ``BittnerMulti7`` attractor handling."""

    def __init__(self, network, attractors=None, horizon: int = 100, device: int = 0, seed: int = 0,
                 update_cap: int = 1 << 20, name: Optional[str] = None, *, all_attractors=None):
        if attractors is None:
            attractors = all_attractors  # the reference's name for the same list; "find" = discover them
        if attractors is None:
            raise ValueError("all_attractors is required (cabean output, or \"find\"; see gym_pbn_amd.io.cabean)")
        if not isinstance(network, PredictorNetwork):
            network = load_network(network)
        self.network = network
        self.name = name or network.name
        self._v = VecPBNTargetMultiEnv(network, attractors, 1, horizon=horizon, device=device, seed=seed,
                                       update_cap=update_cap)
        self.all_attractors = self._v.cfg.attractors
        self.horizon = horizon
        self.target = self.all_attractors[-1]
        self.n_steps = 0
        self.observation_space = spaces.MultiBinary(self._v.N)  # pbn_target_multi.py:56-59
        self.action_space = spaces.MultiDiscrete(self._v.N + 1)

    @property
    def graph_state(self) -> tuple:
        return tuple(self._v.batch.get_bits()[0].tolist())

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):  # :227-259
        if options is not None and "state" in options:
            bits = np.array([int(x) for x in options["state"]], dtype=np.uint8)
            self._v.batch.set_bits(bits[None])
            self._v.batch.set_n_steps(np.zeros(1, np.int64))
        else:
            self._v.reset()
        self.n_steps = 0
        obs = self.graph_state
        tgt = tuple(x if x != "*" else 0 for x in self.target[0])
        info = {"observation_idx": state_to_idx(obs), "observation_dict": obs}
        return (obs, tgt), info

    def step(self, actions):  # :119-154
        dedup = not isinstance(actions, list)
        if hasattr(actions, "detach"):
            actions = actions.detach().cpu().numpy()
        a = np.asarray(actions, dtype=np.int32).reshape(1, -1)
        b = self._v.batch
        obs, rew, flags, nup = b.env_step_multi(self._v.cfg, a, offset=1, dedup=dedup,
                                                update_cap=self._v.update_cap)
        self.n_steps += 1
        if flags[0] & L.FLAG_CAPPED:
            raise RuntimeError(f"update cap ({self._v.update_cap}) reached before an attracting state")
        o = tuple(unpack_bits(obs, self.network.n_nodes)[0].tolist())
        info = {"observation_idx": state_to_idx(o), "observation_dict": o, "n_updates": int(nup[0])}
        return o, int(rew[0]), bool(flags[0] & L.FLAG_TERMINATED), bool(flags[0] & L.FLAG_TRUNCATED), info


def _cube_match(cube, state) -> bool:
    return all(c == "*" or int(c) == int(x) for c, x in zip(cube, state))


class PBNTargetEnv:
    """``PBNTargetEnv`` (``pbn_target.py:241-352``, the ``Bittner-N-v0`` envs) -- R5.

    ``step`` raises at HEAD in both modes, so this follows the intended
    semantics, build-defined: flip node ``action - 1`` (0 = none), one R1 update
    (``force=True``) or updates until the state is attracting (``force=False``, the
    ``is_attracting_state`` loop); reward +20 and terminated when the state matches a
    cube of the target attractor (``in_target`` :289-301, '*' = any), else -5;
    ``truncated = n_steps == horizon``. ``reset`` draws two distinct attractors
    (``random.sample``, :333) and fills '*' bits with ``randint(0, 1)`` (:334-341).
    Transitions run on the GPU (Philox); host draws come from a per-env ``random.Random``.
    """

    def __init__(self, network, all_attractors, horizon: int = 100, device: int = 0, seed: int = 0,
                 update_cap: int = 1 << 20, name: Optional[str] = None):
        all_attractors = resolve_all_attractors(network, all_attractors, device=device, seed=seed)  # "find"
        self.graph = Graph(network, device=device, seed=seed)
        self.N = self.graph.N
        self.name = name or self.graph.network.name
        self.all_attractors = [list(a) for a in all_attractors]
        self.cubes = [c for a in self.all_attractors for c in a]
        self.horizon = int(horizon)
        self.update_cap = int(update_cap)
        self.n_steps = 0
        self.target = None
        self._rng = random.Random()
        self.observation_space = spaces.MultiBinary(self.N)  # pbn_target.py:90-93
        self.action_space = spaces.Discrete(self.N + 1)  # intervention nodes + no action
        # force=False runs in the until-attractor kernel, testing the state after every update
        self._cfg = EnvConfig(self.graph._b.net, self.all_attractors, horizon=self.horizon,
                              first_update_tested=True)

    def _seed(self, seed):  # pbn_target.py:205-207
        self._rng.seed(seed)

    def is_attracting_state(self, state) -> bool:
        return any(_cube_match(c, state) for c in self.cubes)

    def in_target(self, observation) -> bool:  # :289-301
        if self.target is None:
            raise ValueError("Target should have been initialized during env.reset()")
        return any(_cube_match(c, observation) for c in self.target)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):  # :328-352
        if seed:  # `if seed:` -- seed 0 is not applied (Q9)
            self._seed(seed)
        state_attractor, target_attractor = self._rng.sample(self.all_attractors, 2)
        state = list(self._rng.choice(state_attractor))
        target = list(self._rng.choice(target_attractor))
        for i in range(len(state)):
            if state[i] == "*":
                state[i] = self._rng.randint(0, 1)
            if target[i] == "*":
                target[i] = self._rng.randint(0, 1)
        self.graph.setState(state)
        self.n_steps = 0
        obs = self.graph.getState()
        self.target = target_attractor
        return (tuple(state), tuple(target)), {"observation_idx": state_to_idx(obs), "observation_dict": obs}

    def step(self, action: int = 0, force: bool = True):
        if not (0 <= int(action) <= self.N):
            raise Exception(f"Invalid action {action}, not in action space.")
        self.n_steps += 1
        if not self.graph._initialised:
            raise Exception("Forgot to initialise the states")
        if force:
            if action != 0:
                self.graph.flipNode(int(action) - 1)
            obs = self.graph.step()
            n = 1
        else:  # flip + updates until attracting, in one kernel call
            words, _, flags, nup = self.graph._b.env_step_multi(self._cfg, np.array([[int(action)]], np.int32),
                                                                offset=1, dedup=True, update_cap=self.update_cap)
            if flags[0] & L.FLAG_CAPPED:
                raise RuntimeError(f"update cap ({self.update_cap}) reached before an attracting state")
            obs = tuple(unpack_bits(words, self.N)[0].tolist())
            n = int(nup[0])
        terminated = self.in_target(obs)
        reward = 20 if terminated else -5  # :303-326
        truncated = self.n_steps == self.horizon
        return np.array(obs), reward, terminated, truncated, {"observation_idx": state_to_idx(obs),
                                                              "observation_dict": obs, "n_updates": n}


class PBNEnv:
    """``PBNEnv`` (``pbn_env.py``) over the device truth-table engine (R7).

    Same constructor as the reference. ``all_attractors`` are derived from the full
    asynchronous STG (:func:`gym_pbn_amd.stg.compute_attractors`, ``pbn_env.py:54``)
    unless given with the keyword-only ``all_attractors`` (needed past ~20 nodes):
    a list of attractors (each an iterable of state tuples) is taken as given, and
    ``"find"`` has them found on the device by reachability from simulated states
    (:func:`gym_pbn_amd.attractors.find_attractors` on the same ``"stg"`` graph; exact
    attractors, sampled coverage; at most 2**16 states in all).
    ``goal_config["target_nodes"]`` (a set of state tuples) is required as in the
    reference (``:44-51``). Host-side draws (``reset``'s ``random.choice`` calls) come
    from a per-env ``random.Random`` that ``reset(seed)`` seeds like ``random.seed``
    (``:89-91``); the transitions run on the GPU (Philox, re-keyed by ``reset(seed)``).
    """

    def __init__(self, render_mode: str = "human", render_no_cache: bool = False, PBN_data=None,
                 logic_func_data=None, name: str = None, goal_config: dict = None, reward_config: dict = None,
                 *, all_attractors=None, device: int = 0, seed: int = 0):
        network = None
        if isinstance(all_attractors, str) and all_attractors == "find":  # opt-in: found on the device
            network = PBN.table_network(PBN_data, logic_func_data)
            all_attractors = find_state_attractors(network, device=device, seed=seed)
        self.PBN = PBN(PBN_data, logic_func_data, network=network, device=device, seed=seed)
        goal_config = self._check_config(goal_config, "goal", {"target", "all_attractors"})
        if goal_config is None or "target_nodes" not in goal_config:
            raise KeyError("target_nodes")  # pbn_env.py:51
        if type(goal_config["target_nodes"]) is not set:
            raise AssertionError("Did you put multiple attractors as the target by mistake?")
        if all_attractors is None:
            from .stg import compute_attractors

            all_attractors = compute_attractors(self.PBN.network)
        # ordered copies: reset's random.choice picks by position, and a set rebuilt from another
        # process's iteration order need not iterate in that order again
        self._attractor_lists = [list(dict.fromkeys(tuple(int(v) for v in s) for s in a)) for a in all_attractors]
        self.all_attractors = [set(a) for a in self._attractor_lists]
        self.target_nodes = set(goal_config["target_nodes"])
        for attractor in self.all_attractors:  # pbn_env.py:57-59
            if self.target_nodes & attractor:
                self.target_nodes = self.target_nodes.union(attractor)
        self.attracting_states = set.union(*self.all_attractors)
        reward_config = self._check_config(
            reward_config, "reward", {"successful_reward", "wrong_attractor_cost", "action_cost"},
            default_values={"successful_reward": 10, "wrong_attractor_cost": 2, "action_cost": 1})
        self.successful_reward = reward_config["successful_reward"]
        self.wrong_attractor_cost = reward_config["wrong_attractor_cost"]
        self.action_cost = reward_config["action_cost"]
        self.name = name
        self.render_mode = render_mode
        self.step_no = 0
        self.observation_space = spaces.bool_multibinary(self.PBN.N)  # pbn_env.py:81-83
        self.action_space = spaces.Discrete(self.PBN.N)
        self._rng = random.Random()

    @staticmethod
    def _check_config(config, _type, required_keys, default_values=None):  # pbn_env.py:93-123
        if config:
            missing = required_keys - set(config.keys())
            if len(missing) > 1:
                raise ValueError(f"Invalid {_type} config provided. The following required values are missing: "
                                 f"{', '.join(missing)}.")
            return config
        return default_values

    def _seed(self, seed: int = None):  # pbn_env.py:89-91
        self._rng.seed(seed)
        self.PBN.reseed(0 if seed is None else seed)

    @staticmethod
    def _state_to_idx(state) -> int:
        return state_to_idx(np.asarray(state, dtype=np.int8).tolist())

    def is_attracting_state(self, state) -> bool:  # pbn_env.py:19-21
        return True

    def reset(self, seed: int = None, options: dict = None):  # pbn_env.py:190-213
        if seed is not None:
            self._seed(seed)
        if options is not None and "state" in options:
            state = options["state"]  # the reference draws the state below regardless
        else:
            state = self._rng.choice(tuple(self.attracting_states))
        attr = None
        while attr is None or len(attr) > 10:
            attr = self._rng.choice(self._attractor_lists)
        state = self._rng.choice(tuple(attr))
        observation = self.PBN.reset(state)
        if tuple(int(x) for x in observation) not in self.attracting_states:
            raise ValueError("state initial state should be an attractor")
        self.step_no = 0
        return observation, {"observation_idx": self._state_to_idx(observation)}

    def _get_reward(self, observation, action):  # pbn_env.py:156-188
        reward, terminated = 0, False
        if tuple(int(x) for x in observation) in self.target_nodes:
            reward += 20
            terminated = True
        else:
            reward -= 4
            if action != 0:
                reward -= 1
        return reward, terminated, False

    def step(self, action: int):  # pbn_env.py:125-154
        if not self.action_space.contains(action):
            raise Exception(f"Invalid action {action}, not in action space.")  # :138-139
        if action != 0:
            self.PBN.flip(int(action))  # flips node `action`, not action-1 (:141-142)
        self.PBN.step()  # is_attracting_state is always True: exactly one update (:144-146)
        observation = self.PBN.state
        reward, terminated, truncated = self._get_reward(observation, action)
        return observation, reward, terminated, truncated, {"observation_idx": self._state_to_idx(observation)}


__all__ = ["Graph", "PBN", "PBNTargetEnv", "PBNTargetMultiEnv", "VecPBNTargetMultiEnv", "VecPBNEnv", "PBNEnv",
           "state_to_idx", "pack_bits"]
