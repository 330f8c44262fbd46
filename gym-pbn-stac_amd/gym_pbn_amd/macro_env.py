"""The macro-action MDPs of truth-table networks on the device.

``PBNSampledDataEnv`` (``sampled_data.py:15-85``) and ``PBNSelfTriggeringEnv`` (``self_triggering.py:15-92``) let
the agent pick a primitive action and a duration; the env repeats flip + ``PBN.step`` + ``_get_reward`` for that
long and returns one accumulated reward. :class:`TorchVecPBNSampledDataEnv` and
:class:`TorchVecPBNSelfTriggeringEnv` run B such envs with one launch per macro step (``pbn_tenv_macro_device``,
kernel ``k_tenv_macro``); they live in :mod:`gym_pbn_amd.torch_macro_env` and are reachable from here by name.

This module itself imports neither libpbnsim nor torch: the tables the kernel reads and the layout of the discrete
action space are plain functions, so that they can be pinned without a device.
"""

from __future__ import annotations

import numpy as np

MACRO_INTERVAL = 0  # PBN_MACRO_INTERVAL: the limit is the number of rounds
MACRO_TRIGGER = 1   # PBN_MACRO_TRIGGER: the limit is the stop probability in tenths
TENV_MACRO_MAX_T = 65536  # PBN_TENV_MACRO_MAX_T
N_PROBS = 10  # self_triggering.py:45: prob_space = Discrete(10, start=1)


def stop_thresholds() -> np.ndarray:
    """uint64 ``[11]``: entry ``p`` is ``floor((p / 10) * 2**53)``, entry 0 unused (0).

    The reference stops when ``random.uniform(0, 1) <= p / 10`` (``self_triggering.py:61,79``); ``uniform(0, 1)`` is
    ``random()`` = ``k53 * 2**-53`` for an integer ``k53 < 2**53``. Scaling the float ``p / 10`` by ``2**53`` is
    exact, so ``k53 * 2**-53 <= p / 10`` iff ``k53 <= floor((p / 10) * 2**53)``: the kernel compares integers.
    Entry 10 is ``2**53``: every ``k53`` stops."""
    thr = np.zeros(N_PROBS + 1, dtype=np.uint64)
    for p in range(1, N_PROBS + 1):
        thr[p] = int((p / 10) * 9007199254740992.0)  # exact product, already an integer or floored by int()
    return thr


def gamma_powers(gamma: float, T: int) -> np.ndarray:
    """float64 ``[T]``: entry ``i`` is Python's ``gamma ** i``, the factor of ``self_triggering.py:77``. Computed
    by the interpreter and handed to the kernel as a table, so the discounted sum matches the reference bit for
    bit without a ``pow`` on the device."""
    g = float(gamma)
    return np.array([g ** i for i in range(int(T))], dtype=np.float64)


def decode_discrete(idx, n_primitive: int):
    """``(action, limit)`` of an index into the reference's ``discrete_action_space`` (``Discrete(n_primitive *
    n_limits)``): ``action = idx % n_primitive``, ``limit = idx // n_primitive + 1``. Works on ints, numpy
    arrays and torch integer tensors alike (floor division)."""
    return idx % n_primitive, idx // n_primitive + 1


def __getattr__(name):
    # the env classes need libpbnsim and torch: loaded on first use
    if name in ("TorchVecPBNSampledDataEnv", "TorchVecPBNSelfTriggeringEnv"):
        from . import torch_macro_env

        return getattr(torch_macro_env, name)
    raise AttributeError(name)


__all__ = ["stop_thresholds", "gamma_powers", "decode_discrete", "TorchVecPBNSampledDataEnv",
           "TorchVecPBNSelfTriggeringEnv", "MACRO_INTERVAL", "MACRO_TRIGGER", "TENV_MACRO_MAX_T"]
