"""The host side of the until-attractor env over a state set (no GPU): how ``TorchVecPBNTargetMultiSetEnv`` turns its
``attractors`` argument into labelled rows (``torch_env.labelled_attractors``), and the state set's hull words."""

import numpy as np
import pytest

from shape_cases import tt_net


def _rows(rng, N, count):
    W = (N + 63) // 64
    r = rng.integers(0, 1 << 63, size=(count, W), dtype=np.uint64) << np.uint64(1) | rng.integers(
        0, 2, size=(count, W), dtype=np.uint64)
    if N % 64:
        r[:, -1] &= (np.uint64(1) << np.uint64(N % 64)) - np.uint64(1)
    return np.unique(r, axis=0)


def _bits(words, N):
    idx = np.arange(N)
    return ((words[:, idx // 64] >> (idx % 64).astype(np.uint64)) & np.uint64(1)).astype(int)


@pytest.mark.parametrize("N", [18, 65, 200])
def test_attractor_forms_give_one_labelled_table(N):
    """Packed arrays, lists of state tuples, cube lists and an AttractorResult name the same attractors: rows ordered
    by label, row_off[k] the first row of attractor k, labels = the attractor's index, all of it a StateSet."""
    from gym_pbn_amd.attractors import AttractorResult
    from gym_pbn_amd.stateset import StateSet
    from gym_pbn_amd.torch_env import labelled_attractors

    net = tt_net(N)
    assert net.n_nodes == N
    W = net.n_words
    rng = np.random.default_rng(N)
    pool = _rows(rng, N, 40)
    a0, a1 = pool[:1], pool[1:14]
    # attractor 2 as cubes: two overlapping cubes with 3 and 2 free nodes around one state
    x = _bits(pool[20:21], N)[0].tolist()
    free_a, free_b = [1, 3, N - 1], [3, 4]
    cube_a = tuple("*" if i in free_a else v for i, v in enumerate(x))
    cube_b = tuple("*" if i in free_b else v for i, v in enumerate(x))
    as_tuples = [tuple(r) for r in _bits(a1, N).tolist()]
    rows, labels, row_off = labelled_attractors(net, [a0, as_tuples, [cube_a, cube_b]])
    n2 = 8 + 4 - 2  # the cubes share the states with node 4 at x's value and nodes 1, N - 1 at x's
    assert rows.dtype == np.uint64 and rows.shape == (1 + 13 + n2, W)
    assert row_off.dtype == np.uint32 and row_off.tolist() == [0, 1, 14, 14 + n2]
    assert labels.dtype == np.int32 and labels.tolist() == [0] + [1] * 13 + [2] * n2
    assert np.array_equal(rows[:1], a0) and np.array_equal(rows[1:14], a1)
    got = _bits(rows[14:], N)
    assert len(np.unique(rows[14:], axis=0)) == n2
    for g in got:  # every row lies in one of the two cubes
        assert any(all(c == "*" or c == v for c, v in zip(cube, g)) for cube in (cube_a, cube_b))
    s = StateSet(rows, N, labels=labels, device=None)
    assert len(s) == len(rows) and s.n_labels == 3
    assert np.array_equal(s.lookup(rows), labels)
    for k in range(3):
        assert (s.lookup(rows[int(row_off[k]):int(row_off[k + 1])]) == k).all()
    # an AttractorResult and packed arrays: the same table
    res = AttractorResult(N, attractors=[a0, a1, rows[14:]])
    r2, l2, o2 = labelled_attractors(net, res)
    assert np.array_equal(r2, rows) and np.array_equal(l2, labels) and np.array_equal(o2, row_off)
    # the hull words: AND / OR over the members
    all_w, any_w = s.hull()
    assert np.array_equal(all_w, np.bitwise_and.reduce(rows, axis=0))
    assert np.array_equal(any_w, np.bitwise_or.reduce(rows, axis=0))
    one = StateSet(a0, N, device=None)
    assert np.array_equal(one.hull()[0], a0[0]) and np.array_equal(one.hull()[1], a0[0]) and one.n_labels == 1


def test_refusals():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.attractors import AttractorResult
    from gym_pbn_amd.torch_env import labelled_attractors

    net = tt_net(65)
    wide = tuple(["*"] * 25 + [0] * 40)  # 2^25 states
    with pytest.raises(ValueError, match="STATESET_MAX_STATES"):
        labelled_attractors(net, [[wide]])
    half = tuple(["*"] * 23 + [0] * 42)  # 2^23 each: the third passes 2^24 before anything is expanded
    with pytest.raises(ValueError, match="STATESET_MAX_STATES"):
        labelled_attractors(net, [[tuple([1] * 65)], [half, half, half]])
    with pytest.raises(ValueError, match="non-empty"):
        labelled_attractors(net, [[tuple([1] * 65)], []])
    with pytest.raises(ValueError, match="non-empty"):
        labelled_attractors(net, [])
    with pytest.raises(ValueError):
        labelled_attractors(net, None)
    with pytest.raises(ValueError, match="70 nodes"):
        labelled_attractors(net, AttractorResult(70, attractors=[np.zeros((1, 2), np.uint64)]))
    with pytest.raises(ValueError, match="find"):
        labelled_attractors(net, "cabean")
    # one state under two attractors is refused by the set
    from gym_pbn_amd.stateset import StateSet

    rows, labels, _ = labelled_attractors(net, [[tuple([1] * 65)], [tuple([1] * 65)]])
    with pytest.raises(ValueError, match="different label"):
        StateSet(rows, 65, labels=labels, device=None)
    # the entry points report NULL arguments like every other
    assert _lib.lib.pbn_env_set_step_device(*([None] * 3), 1, 1, 1, 1, 1, 1, 1, 0, 0, *([None] * 6)) == _lib.PBN_E_INVALID
    assert _lib.last_error() == "batch is NULL"
    assert _lib.lib.pbn_env_set_reset_device(None, None, None, 1, 0, None, None) == _lib.PBN_E_INVALID
    assert _lib.lib.pbn_env_set_check(None) == _lib.PBN_E_INVALID
    assert _lib.lib.pbn_stateset_get_hull(None, None, None, None) == _lib.PBN_E_INVALID


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ is not installed")
def test_hull_header_logic_is_clean_under_asan_and_ubsan():
    """``make statesethullcheck``: tests/host/stateset_hull_check.cpp on csrc/pbn_stateset.hpp alone (no HIP header,
    no library, no GPU) with ASan + UBSan: the builder's hull words and label count against a loop over the rows for
    W = 1 .. 8, and the pre-filter k_env_set runs: no member rejected, a flipped agreed node rejected."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(["make", "-C", str(root / "gym-pbn-stac_amd"), "statesethullcheck"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "stateset_hull_check ok" in r.stdout
