"""The tables and the action layout of the macro-action envs (``gym_pbn_amd.macro_env``), pinned without a device:
the kernel compares integers against ``stop_thresholds`` and multiplies by ``gamma_powers``, so these two are
where the reference's ``uniform(0, 1) <= prob`` and ``gamma ** i`` enter. Every comparison is exact."""

import math
import sys
from fractions import Fraction

import numpy as np

from gym_pbn_amd.macro_env import decode_discrete, gamma_powers, stop_thresholds


def test_the_helpers_load_neither_the_library_nor_torch():
    import subprocess

    code = ("import sys; import gym_pbn_amd.macro_env as m; m.stop_thresholds(); "
            "assert 'gym_pbn_amd._lib' not in sys.modules and 'torch' not in sys.modules")
    # a fresh interpreter (this one has long loaded both), on this one's module path
    subprocess.run([sys.executable, "-c", f"import sys; sys.path[:] = {list(sys.path)!r}; {code}"], check=True)


def test_stop_thresholds_are_the_floor_of_the_float_probability():
    thr = stop_thresholds()
    assert thr.dtype == np.uint64 and thr.shape == (11,)
    for p in range(1, 11):
        assert int(thr[p]) == math.floor(Fraction(float(p / 10)) * 2 ** 53), p
    assert int(thr[10]) == 2 ** 53


def test_the_integer_compare_is_the_reference_float_compare():
    """``random.uniform(0, 1)`` is ``0 + (1 - 0) * random()`` = ``k53 * 2**-53``; the reference stops on
    ``<= p / 10`` (self_triggering.py:61,79)."""
    thr = [int(t) for t in stop_thresholds()]
    rng = np.random.default_rng(0)
    k53 = [int(v) for v in rng.integers(0, 1 << 53, size=10_000, dtype=np.uint64)]
    # the edges of every threshold, and of the range
    k53 += [0, (1 << 53) - 1] + [t + d for t in thr[1:10] for d in (-1, 0, 1)]
    for p in range(1, 11):
        prob = p / 10
        for k in k53:
            assert (k <= thr[p]) == (0 + (1 - 0) * (k * 2.0 ** -53) <= prob), (p, k)


def test_gamma_powers_are_the_interpreters():
    g = gamma_powers(0.99, 64)
    assert g.dtype == np.float64 and g.shape == (64,)
    for i in range(64):
        assert g[i] == 0.99 ** i, i
    assert g[0] == 1.0


def test_decode_discrete_round_trips_the_discrete_space():
    n_primitive, T = 7, 5
    seen = set()
    for idx in range(n_primitive * T):
        a, lim = decode_discrete(idx, n_primitive)
        assert 0 <= a < n_primitive and 1 <= lim <= T
        assert a + n_primitive * (lim - 1) == idx
        seen.add((a, lim))
    assert len(seen) == n_primitive * T
    idx = np.arange(n_primitive * T)
    a, lim = decode_discrete(idx, n_primitive)
    assert np.array_equal(a + n_primitive * (lim - 1), idx)
    assert decode_discrete(n_primitive * T, n_primitive)[1] == T + 1  # one past the space: a limit the env refuses
