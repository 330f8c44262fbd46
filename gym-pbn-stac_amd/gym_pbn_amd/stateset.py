"""Exact sets of packed states that a kernel can query (``pbn_stateset_*``, ``csrc/pbn_stateset.hpp``).

The reference envs keep attractors and targets as Python sets of state tuples (``pbn_env.py:57-59``) and test
``state in set`` one env at a time. A :class:`StateSet` is the same thing for packed ``[S][W]`` uint64 rows:
built once on the host (deterministic open-addressing layout), optionally uploaded, and then queried for a whole
batch in one launch (:meth:`gym_pbn_amd.batch.PBNBatch.classify`) or inside the fused ``PBN-v0`` step
(:class:`gym_pbn_amd.torch_env.TorchVecPBNEnv`). Every state carries an int label (e.g. its attractor's index);
a lookup returns the label, or -1 for a non-member. Up to ``2**24`` states.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L


class StateSet:
    """``StateSet(states, n_nodes, labels=None, device=0)``.

    ``states``: packed rows ``[S][W]`` uint64 (``W = ceil(n_nodes / 64)``; bits past node ``N - 1`` must be
    zero). ``labels``: ``[S]`` ints ``>= 0`` (``None``: all 0). A row given twice with one label is kept once;
    with two labels it is a ``ValueError``. ``device=None`` builds the host copy only: :meth:`lookup` works,
    device calls are refused (``PBN_E_STATE``) -- the same definition, pinned without a GPU.
    """

    def __init__(self, states, n_nodes: int, labels=None, device: Optional[int] = 0):
        self.n_nodes = int(n_nodes)
        self.n_words = (self.n_nodes + 63) // 64
        w = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, self.n_words)
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
            if lab.shape[0] != w.shape[0]:
                raise ValueError(f"{lab.shape[0]} labels for {w.shape[0]} states")
            if lab.size and (lab.min() < 0 or lab.max() > 0x7FFFFFFF):
                raise ValueError("labels must lie in [0, 2^31)")
            lab = lab.astype(np.int32)
        self.device = None if device is None else int(device)
        h = C.c_void_p()
        L.check(L.lib.pbn_stateset_create(self.n_nodes, -1 if device is None else int(device),
                                          L.ptr(w if w.size else None, L._u64p), L.ptr(lab, L._i32p), w.shape[0],
                                          C.byref(h)))
        self._h = h

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(L, "lib", None) is not None:
            L.lib.pbn_stateset_destroy(h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        i = L.StateSetInfo()
        L.check(L.lib.pbn_stateset_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in L.StateSetInfo._fields_}

    def __len__(self) -> int:
        return int(self.info()["n_states"])

    def hull(self):
        """``(all_words, any_words)``: the AND and the OR of the members' words, ``[W]`` uint64 each. Node ``i`` has
        one value in every member iff bit ``i`` of ``all ^ any`` is 0: what the until-attractor kernel tests before
        it probes the table."""
        a = np.empty(self.n_words, dtype=np.uint64)
        o = np.empty(self.n_words, dtype=np.uint64)
        L.check(L.lib.pbn_stateset_get_hull(self._h, L.ptr(a, L._u64p), L.ptr(o, L._u64p), None))
        return a, o

    @property
    def n_labels(self) -> int:
        """The largest label + 1 (0 for the empty set)."""
        top = C.c_int32(-1)
        L.check(L.lib.pbn_stateset_get_hull(self._h, None, None, C.byref(top)))
        return int(top.value) + 1

    def lookup(self, states) -> np.ndarray:
        """Labels ``[n]`` int32 of packed ``states`` ``[n][W]`` on the host (-1: not a member)."""
        w = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, self.n_words)
        out = np.empty(w.shape[0], dtype=np.int32)
        if w.shape[0]:
            L.check(L.lib.pbn_stateset_lookup(self._h, L.ptr(w, L._u64p), w.shape[0], L.ptr(out, L._i32p)))
        return out


__all__ = ["StateSet"]
