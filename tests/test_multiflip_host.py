"""The multi-flip until-attractor MDP (``gym_pbn_amd.multiflip``, ``pbn_stg_flipset_*_device``) without a GPU: the host
statement of the max over flip sets against a direct restatement on tied integer worths, the host statement of the
arrival worth ``M`` against exact ``Fraction`` arithmetic and against a brute-force push of the env's step loop, the
refusals of the C entry points on a host-only handle and of ``MultiFlipProblem``'s parameter checks, and the rule
header under ASan + UBSan (``make flipsetrulecheck``).

The bound of ``M`` lives here (``arrival_bound``); the GPU tests import it. ``M`` is ``n`` applications of an operator
that does not expand the sup norm -- ``n - 2`` sweeps and two expectations on a transient row, one expectation on a
labelled one -- each within ``sweep_bound`` (which is ``expect_bound`` plus the rounded add of the source) of its exact
value: ``summed_bound(N, n, x0max=max|g|)`` of ``test_absorb_host.py``.
"""

import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

from test_absorb_host import as_fractions, dense_chain, exact_sweep, golden_case, summed_bound, tt6_case
from test_attractors_host import all_states, case_network
from test_control_host import U53, exact_expect, host_nbr
from test_transition_host import case_by


def arrival_bound(n_nodes, n_updates, gmax):
    return summed_bound(n_nodes, n_updates, x0max=float(gmax))


# ---------------------------------------------------------------- the max
def restated_max(m, nbr, nodes, A, cost, noop_cost):
    """Row by row: every combination as a tuple ``(-value, flips, end)``, the smallest tuple wins."""
    S = len(m)
    v, end, flips = np.full(S, -np.inf), np.full(S, -1, dtype=np.int32), np.zeros(S, dtype=np.int32)
    for s in range(S):
        best = None
        for d in range(1, A + 1):
            for F in itertools.combinations(nodes, d):
                y = s
                for i in F:
                    y = int(nbr[y, i])
                    assert y >= 0
                key = (-(m[y] - cost * len(F)), d, y)
                best = key if best is None or key < best else best
        if noop_cost is not None:
            key = (-(m[s] - noop_cost), 0, s)
            best = key if best is None or key < best else best
        if best is not None:
            v[s], flips[s], end[s] = -best[0], best[1], best[2]
    return v, end, flips


@pytest.mark.parametrize("name", ["cube5", "tt6-step"])
def test_host_max_against_a_direct_restatement(name):
    """Tied integer worths (four values), every ``A`` in 1 .. 4 and one past the number of allowed nodes, costs 0, 0.5
    and 1, ``noop_cost`` None, 0 and 2: value, end row and flip count equal the restatement's; given as states or as
    ``nbr``; and the policy's set has ``1 .. A`` allowed nodes."""
    from gym_pbn_amd.multiflip import host_multiflip_max

    if name == "cube5":
        states, N, nodes = all_states(5), 5, [0, 2, 3]
    else:
        c = tt6_case()
        states, N, nodes = c["states"], 6, [1, 2, 3, 4, 5]  # node 0 is clear in every row: its flip leaves the set
    nbr = host_nbr(states, N, nodes)
    rng = np.random.default_rng(11)
    m = rng.integers(0, 4, size=len(states)).astype(np.float64)
    for A in (1, 2, 3, 4, len(nodes) + 1):
        for cost in (0.0, 0.5, 1.0):
            for noop in (None, 0.0, 2.0):
                want = restated_max(m, nbr, nodes, min(A, len(nodes)), cost, noop)
                got = host_multiflip_max(m, nbr, nodes, A, cost, noop)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), (A, cost, noop)
                again = host_multiflip_max(m, np.ascontiguousarray(states, dtype=np.uint64), nodes, A, cost, noop)
                for g, w in zip(again, want):
                    assert np.array_equal(g, w)
                v, end, flips = got
                F = states[:, 0] ^ states[end, 0]
                pop = np.array([bin(int(f)).count("1") for f in F])
                assert np.array_equal(pop, flips) and flips.max() <= A
                assert (flips >= (0 if noop is not None else 1)).all()
                assert all(int(f) & ~sum(1 << i for i in nodes) == 0 for f in F)
    if name == "tt6-step":
        with pytest.raises(ValueError, match="leaves the state set"):
            host_multiflip_max(m, host_nbr(states, N, nodes), [0, 1], 1, 1.0)
    # one value per row cannot exclude the empty set: the walk i, i comes back at cost 2k and beats every action
    m2 = np.zeros(len(states))
    m2[0] = 100.0
    v, end, flips = host_multiflip_max(m2, nbr, nodes, 2, 1.0)
    assert end[0] != 0 and flips[0] == 1 and v[0] == -1.0


def test_the_benchmarks_torch_legs_are_the_same_max():
    """``tools/bench_multiflip.py``'s two torch legs (the recursion in torch ops, plain enumeration) on CPU tensors over
    the 5-cube: ``v`` bit-equal to ``host_multiflip_max``, the policy equal, on tied and on random worths."""
    import importlib.util
    from pathlib import Path

    import torch

    from gym_pbn_amd.multiflip import host_multiflip_max

    spec = importlib.util.spec_from_file_location("bench_multiflip", Path(__file__).resolve().parents[1] / "tools" / "bench_multiflip.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    nodes = [0, 1, 3, 4]
    nbr = host_nbr(all_states(5), 5, nodes)
    cols = [torch.from_numpy(nbr[:, i].astype(np.int64)) for i in nodes]
    rng = np.random.default_rng(4)
    for m in (rng.integers(0, 3, size=32).astype(np.float64), rng.uniform(-9.0, 9.0, size=32)):
        for A in (1, 2, 3):
            for k in (0.0, 1.0):
                want = host_multiflip_max(m, nbr, nodes, A, k)
                for leg in (bench.torch_recursion, bench.torch_enumeration):
                    v, end, flips = leg(cols, torch.from_numpy(m), A, k)
                    assert np.array_equal(v.numpy().view(np.uint64), want[0].view(np.uint64)), (leg.__name__, A, k)
                    assert np.array_equal(end.numpy(), want[1]) and np.array_equal(flips.numpy(), want[2])


# ---------------------------------------------------------------- the arrival worth
def random_v(S, seed=5):
    return np.random.default_rng(seed).uniform(-50.0, 50.0, size=S)


def test_host_arrival_against_exact_arithmetic():
    """Golden (8, 2, 6), ``n = 6``, target class 1, ``R = 1000``, ``gamma = 0.9``: ``M`` within ``arrival_bound`` of the
    same formula in ``Fraction``s from the same doubles ``g``."""
    from gym_pbn_amd.multiflip import host_multiflip_arrival

    n, R, gamma, target = 6, 1000.0, 0.9, 1
    case = golden_case((8, 2, 6))
    label, N = case["label"], case["N"]
    v = random_v(len(label))
    got = host_multiflip_arrival(case["mass"], case["succ"], label, case["n_movable"], target, v, n, R, gamma)
    g = np.where(label == target, R, gamma * v)
    z = as_fractions(g.reshape(-1, 1))
    for _ in range(n - 2):
        z = exact_sweep(case, z, [0.0])
    e = lambda x: exact_expect(case["mass"], case["succ"], case["n_movable"], x)  # noqa: E731

    def exact_e(fr):  # exact_expect takes doubles; here the input is already rational
        den = (1 << 53) * case["n_movable"]
        out = []
        for s in range(len(fr)):
            acc = fr[s]
            for i in np.flatnonzero(case["mass"][s]):
                acc += Fraction(int(case["mass"][s, i]), den) * (fr[int(case["succ"][s, i])] - fr[s])
            out.append(acc)
        return out

    eg, eez = e(g), exact_e(exact_e(z[0]))
    want = [eg[s] if label[s] >= 0 else eez[s] for s in range(len(label))]
    dev = float(max(abs(Fraction(float(a)) - b) for a, b in zip(got, want)))
    bound = arrival_bound(N, n, np.abs(g).max())
    print(f"|M - exact| {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound
    held = label >= 0
    assert (got[held & (label == target)] == R).all()  # a constant comes back exactly: the class is closed
    assert (np.abs(got[~held]) < R).all() and got[~held].max() > 100.0
    with pytest.raises(ValueError, match="at least 2"):
        host_multiflip_arrival(case["mass"], case["succ"], label, case["n_movable"], target, v, 1, R, gamma)


def test_arrival_case_split_against_the_step_loop_restated():
    """Golden (8, 2, 6) at cap 6. Brute force, from every ``t`` the flips may lead to, with the dense ``P``: a labelled
    ``t`` makes one update and is worth ``g`` where it lands; a transient ``t`` makes updates 1 and 2, then the state is
    tested after update 2, 3, ..., cap: a labelled state stops and is worth ``g`` there, what is still transient after
    the cap's update is worth ``g`` there too (``gamma V``: the cap ends the step, not the episode). The formula side is
    within ``arrival_bound``; the dense push adds at most ``(N + 3) u max|g|`` per update."""
    from gym_pbn_amd.multiflip import host_multiflip_arrival

    cap, R, gamma, target = 6, 1000.0, 0.9, 0
    case = golden_case((8, 2, 6))
    label, N = case["label"], case["N"]
    S = len(label)
    v = random_v(S, seed=9)
    g = np.where(label == target, R, gamma * v)
    P = dense_chain(case)
    tr = label < 0
    want = np.empty(S)
    want[~tr] = (P @ g)[~tr]
    d = (np.eye(S) @ P) @ P  # d[t]: the law of the state after update 2
    worth = np.zeros(S)
    for u in range(2, cap + 1):
        worth += d[:, ~tr] @ g[~tr]
        d = d * tr[None, :]
        if u < cap:
            d = d @ P
    worth += d @ g
    want[tr] = worth[tr]
    got = host_multiflip_arrival(case["mass"], case["succ"], label, case["n_movable"], target, v, cap, R, gamma)
    gmax = np.abs(g).max()
    bound = arrival_bound(N, cap, gmax) + cap * (N + 3) * U53 * gmax
    dev = np.abs(got - want).max()
    print(f"|M - step loop| {dev:.3e}, bound {bound:.3e}; M in [{got.min():.2f}, {got.max():.2f}]")
    assert dev <= bound
    # the split matters: taking every row as transient (or as labelled) is off by far more than the bound
    assert np.abs((P @ g) - want)[tr].max() > 1.0


# ---------------------------------------------------------------- refusals
def test_refusals_of_the_entry_points_and_of_the_problem():
    import types

    import gym_pbn_amd
    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import Net
    from gym_pbn_amd.multiflip import MultiFlipProblem, MultiFlipSolution, host_multiflip_arrival, host_multiflip_max
    from gym_pbn_amd.transition import TransitionGraph

    assert gym_pbn_amd.MultiFlipProblem is MultiFlipProblem and gym_pbn_amd.MultiFlipSolution is MultiFlipSolution
    assert gym_pbn_amd.host_multiflip_max is host_multiflip_max
    assert gym_pbn_amd.host_multiflip_arrival is host_multiflip_arrival
    lib = _lib.lib
    pm = Net(case_network(case_by(10, 2, 0)))
    s = np.ascontiguousarray(all_states(10)[:5])
    h = C.c_void_p()
    assert lib.pbn_stg_create(pm.handle, -1, 0, _lib.ptr(s, _lib._u64p), 5, C.byref(h)) == 0
    fake, other, third, fourth = (C.c_void_p(64 * k) for k in (1, 2, 3, 4))  # never dereferenced: refused first
    err = _lib.last_error
    INV, STATE = _lib.PBN_E_INVALID, _lib.PBN_E_STATE
    # pbn_stg_flipset_level_device(g, nbr, m, cost, in_base, in_tag, out_base, out_tag)
    args = [fake, fake, 1.0, fake, fake, other, other]
    assert lib.pbn_stg_flipset_level_device(None, *args) == INV and err() == "stg is NULL"
    for k, name in ((0, "d_nbr"), (5, "d_out_base"), (6, "d_out_tag")):
        a = list(args)
        a[k] = None
        assert lib.pbn_stg_flipset_level_device(h, *a) == INV and err() == f"{name} is NULL"
    for k in (3, 4):  # half an input summary
        a = list(args)
        a[k] = None
        assert lib.pbn_stg_flipset_level_device(h, *a) == INV and "both, or both NULL" in err()
    assert lib.pbn_stg_flipset_level_device(h, fake, None, 1.0, None, None, other, other) == INV and err() == "d_m is NULL"
    for cost in (-1.0, -1e-300, float("nan"), float("inf")):
        assert lib.pbn_stg_flipset_level_device(h, fake, fake, cost, fake, fake, other, other) == INV
        assert "is not a finite cost >= 0" in err() and err().startswith("cost=")
    assert lib.pbn_stg_flipset_level_device(h, fake, fake, 1.0, fake, third, fake, fourth) == INV and "aliases" in err()
    assert lib.pbn_stg_flipset_level_device(h, fake, fake, 1.0, third, fake, fourth, fake) == INV and "aliases" in err()
    for a in (args, [fake, fake, 0.0, None, None, other, other], [fake, None, 0.0, fake, fake, other, other]):
        assert lib.pbn_stg_flipset_level_device(h, *a) == STATE and "host-only" in err()
    # pbn_stg_flipset_select_device(g, base, tag, m, cost, noop_cost, v, policy_end, policy_flips)
    args = [fake, fake, fake, 1.0, None, fake, fake, fake]
    assert lib.pbn_stg_flipset_select_device(None, *args) == INV and err() == "stg is NULL"
    for k, name in ((0, "d_base"), (1, "d_tag"), (2, "d_m"), (5, "d_v"), (6, "d_policy_end"), (7, "d_policy_flips")):
        a = list(args)
        a[k] = None
        assert lib.pbn_stg_flipset_select_device(h, *a) == INV and err() == f"{name} is NULL"
    for cost in (-0.5, float("nan")):
        a = list(args)
        a[3] = cost
        assert lib.pbn_stg_flipset_select_device(h, *a) == INV and err().startswith("cost=")
        a = list(args)
        a[4] = C.byref(C.c_double(cost))
        assert lib.pbn_stg_flipset_select_device(h, *a) == INV and err().startswith("noop_cost=")
    for noop in (None, C.byref(C.c_double(0.0)), C.byref(C.c_double(2.0))):
        a = list(args)
        a[4] = noop
        assert lib.pbn_stg_flipset_select_device(h, *a) == STATE and "host-only" in err()
    lib.pbn_stg_destroy(h)
    # MultiFlipProblem: the parameters are judged first, the handle next
    g = TransitionGraph(case_network(case_by(10, 2, 0)), all_states(10), device=None)
    ab = types.SimpleNamespace(graph=g, n_classes=2)
    ok = dict(max_flips=2, n_updates=4)
    for bad, match in ((dict(max_flips=0), r"max_flips=0 outside \[1, 15\]"), (dict(max_flips=16), "max_flips=16 outside"),
                       (dict(n_updates=1), "n_updates=1"), (dict(n_updates=0), "n_updates=0"),
                       (dict(update_cap=1), "update_cap=1"), (dict(gamma=1.0), "gamma=1.0 outside"),
                       (dict(gamma=-0.1), "gamma=-0.1 outside"), (dict(action_cost=-1), "action_cost=-1"),
                       (dict(noop_cost=-2.0), "noop_cost=-2.0"), (dict(action_cost=float("nan")), "action_cost=nan"),
                       (dict(nodes=[]), "no allowed node and no noop_cost"), (dict(nodes=[3, 10]), "nodes outside")):
        with pytest.raises(ValueError, match=match):
            MultiFlipProblem(ab, 1, **{**ok, **bad})
    for target in (-1, 2):
        with pytest.raises(ValueError, match="outside the classes"):
            MultiFlipProblem(ab, target, **ok)
    for kw in (ok, dict(ok, nodes=[], noop_cost=0.0), dict(ok, max_flips=15, noop_cost=3)):
        with pytest.raises(_lib.PbnError) as ei:
            MultiFlipProblem(ab, 1, **kw)
        assert ei.value.code == STATE
    g.close()


# ---------------------------------------------------------------- the rule header
@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ is not installed")
def test_flipset_rule_header_is_clean_under_asan_and_ubsan():
    """``make flipsetrulecheck``: tests/host/flipset_rule_check.cpp on csrc/pbn_flipset_rule.hpp (no HIP header, no
    library, no GPU) with ASan + UBSan: the level recursion against enumeration, and the kernels' walk replayed."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(["make", "-C", str(root / "gym-pbn-stac_amd"), "flipsetrulecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "flipset_rule_check ok" in r.stdout
