"""Device-resident vectorised macro-action envs: the classes behind :mod:`gym_pbn_amd.macro_env`.

Both are :class:`~gym_pbn_amd.torch_env.TorchVecPBNEnv` with another ``step``: same constructor, target set, reset,
``auto_reset``, ``info()`` and ``observation_words``; a macro step is one launch (``pbn_tenv_macro_device``).

Differences from ``PBN-v0`` that the reference makes and these classes keep:

* the primitive action ``a`` flips node ``a - 1`` (``sampled_data.py:62``, ``self_triggering.py:67``), so ``a`` runs
  over ``[0, N]`` and node 0 can be flipped; ``PBN-v0`` flips node ``a``;
* the flip is applied before *every* inner update, not once;
* ``terminated`` is the last inner state's; the reward sums every inner round's ``_get_reward`` (the literals
  20 / -4 / -1 of ``pbn_env.py:156-188``; the self-triggering env's own ``successful_reward`` attributes are never
  read by the reference).

A macro step advances the batch's ``update_count`` by ``T`` whatever the envs' durations were: inner round ``i`` is
update ``update_count + i`` of every env, and the next call starts past the longest run this one could have made.
The self-triggering stop draw is Philox stream 10, counter ``{update, global env id}``.
"""

from __future__ import annotations

from . import spaces
from .macro_env import (MACRO_INTERVAL, MACRO_TRIGGER, N_PROBS, TENV_MACRO_MAX_T, decode_discrete, gamma_powers,
                        stop_thresholds)
from .torch_env import TorchVecPBNEnv


class _TorchVecMacroEnv(TorchVecPBNEnv):
    MODE = None

    def __init__(self, PBN_data=None, logic_func_data=None, goal_config=None, n_envs: int = 1, *, T, gamma: float,
                 **kw):
        T = int(T)
        if not 1 <= T <= TENV_MACRO_MAX_T:
            raise ValueError(f"T={T} outside [1, {TENV_MACRO_MAX_T}] (PBN_TENV_MACRO_MAX_T)")
        super().__init__(PBN_data, logic_func_data, goal_config, n_envs, **kw)
        self.T, self.gamma = T, gamma
        self.primitive_action_space = spaces.Discrete(self.N + 1)  # sampled_data.py:43, self_triggering.py:44
        self.n_limits = T if self.MODE == MACRO_INTERVAL else N_PROBS
        self.limit_space = spaces.Discrete(self.n_limits, start=1)
        self.action_space = spaces.Tuple((self.primitive_action_space, self.limit_space))
        self.discrete_action_space = spaces.Discrete((self.N + 1) * self.n_limits)

    def _reward_args(self, B):
        raise NotImplementedError

    def step(self, actions, limits=None, check: bool = False):
        """``actions`` and ``limits``: int tensors ``[B]`` on the GPU (primitive action in ``[0, N]``; interval in
        ``[1, T]``, or stop probability in tenths in ``[1, 10]``). With ``limits`` None, ``actions`` holds indices
        into ``discrete_action_space``, decoded on the device (:func:`~gym_pbn_amd.macro_env.decode_discrete`).
        An env given a value outside its range is left untouched, outputs included; ``check=True`` waits for the
        launch and raises ``ValueError`` then. Returns ``(obs [B][N] uint8, reward [B], terminated [B] bool,
        truncated [B] bool, info)``; ``info`` holds ``obs_words``, ``label``, ``interval`` (inner rounds run) and
        ``first_hit`` (the first round whose state was in the target, -1: none)."""
        import torch

        a = actions.to(device=self.device).reshape(-1)
        if limits is None:
            a, lim = decode_discrete(a.to(torch.int64), self.N + 1)
            lim = lim.clamp(0, TENV_MACRO_MAX_T + 1)  # stays refused, and fits the int32 the kernel reads
        else:
            lim = limits.to(device=self.device).reshape(-1)
        a = a.to(torch.int32).contiguous()
        lim = lim.to(torch.int32).contiguous()
        B = self.num_envs
        if a.shape[0] != B or lim.shape[0] != B:
            raise ValueError(f"actions for {a.shape[0]} envs and limits for {lim.shape[0]}, the batch has {B}")
        self._use_stream()
        words = torch.empty((B, self.W), dtype=torch.int64, device=self.device)
        label = torch.empty(B, dtype=torch.int32, device=self.device)
        interval = torch.empty(B, dtype=torch.int32, device=self.device)
        first_hit = torch.empty(B, dtype=torch.int32, device=self.device)
        reward, kw = self._reward_args(B)
        self.batch.tenv_macro_device(self.target, self.MODE, self.T, a.data_ptr(), lim.data_ptr(),
                                     self._flags.data_ptr(), d_obs=words.data_ptr(), d_interval=interval.data_ptr(),
                                     d_first_hit=first_hit.data_ptr(), d_labels=label.data_ptr(),
                                     reward_target=self.REWARD_TARGET, step_cost=self.STEP_COST,
                                     action_cost=self.ACTION_COST, check=check, **kw)
        obs, term, trunc = self._finish(words)
        return obs, reward, term, trunc, {"obs_words": words, "label": label, "interval": interval,
                                          "first_hit": first_hit}


class TorchVecPBNSampledDataEnv(_TorchVecMacroEnv):
    """B copies of ``PBNSampledDataEnv`` (``sampled_data.py:15-85``) resident on the device: ``step`` takes a
    primitive action and an interval in ``[1, T]`` per env, runs that many rounds of flip + ``PBN.step`` +
    ``_get_reward`` in one launch and returns the int32 sum of the rounds' rewards.

    ``T`` must be given: the reference's default ``2**N`` is refused (the cap is ``PBN_TENV_MACRO_MAX_T`` = 65536
    rounds per macro step). ``gamma`` is kept as the reference keeps it; its ``step`` does not discount. The other
    arguments are :class:`~gym_pbn_amd.torch_env.TorchVecPBNEnv`'s."""

    MODE = MACRO_INTERVAL

    def __init__(self, PBN_data=None, logic_func_data=None, goal_config=None, n_envs: int = 1, *, T: int = None,
                 gamma: float = 0.99, **kw):
        if T is None:
            raise ValueError("T must be given: the reference's default T = 2**N is not offered on the device, where "
                             f"T is at most PBN_TENV_MACRO_MAX_T = {TENV_MACRO_MAX_T}")
        super().__init__(PBN_data, logic_func_data, goal_config, n_envs, T=T, gamma=gamma, **kw)
        self.interval_space = self.limit_space  # sampled_data.py:44

    def _reward_args(self, B):
        import torch

        reward = torch.empty(B, dtype=torch.int32, device=self.device)
        return reward, {"d_reward_i32": reward.data_ptr()}


class TorchVecPBNSelfTriggeringEnv(_TorchVecMacroEnv):
    """B copies of ``PBNSelfTriggeringEnv`` (``self_triggering.py:15-92``) resident on the device: ``step`` takes a
    primitive action and a stop probability ``p`` in tenths (``[1, 10]``) per env and runs rounds of flip +
    ``PBN.step`` + ``_get_reward`` until a draw ``uniform(0, 1) <= p / 10`` or ``T`` rounds, in one launch. The
    reward is the float64 sum of ``gamma ** i`` times round ``i``'s reward, accumulated in the reference's order
    with the reference's roundings.

    The stop draws are this library's own Philox stream (10, keyed by the update counter and the global env id),
    not the reference's global ``random``: the same MDP, a documented stream of its own."""

    MODE = MACRO_TRIGGER

    def __init__(self, PBN_data=None, logic_func_data=None, goal_config=None, n_envs: int = 1, *, T: int = 5,
                 gamma: float = 0.99, **kw):
        import numpy as np
        import torch

        super().__init__(PBN_data, logic_func_data, goal_config, n_envs, T=T, gamma=gamma, **kw)
        self.prob_space = self.limit_space  # self_triggering.py:45
        with torch.cuda.device(self.device):
            self._gpow = torch.from_numpy(gamma_powers(gamma, self.T)).to(self.device).contiguous()
            self._stop_thr = torch.from_numpy(stop_thresholds().view(np.int64)).to(self.device).contiguous()

    def _reward_args(self, B):
        import torch

        reward = torch.empty(B, dtype=torch.float64, device=self.device)
        return reward, {"d_reward_f64": reward.data_ptr(), "d_gpow": self._gpow.data_ptr(),
                        "d_stop_thr": self._stop_thr.data_ptr()}


__all__ = ["TorchVecPBNSampledDataEnv", "TorchVecPBNSelfTriggeringEnv"]
