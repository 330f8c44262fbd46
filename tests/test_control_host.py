"""Optimal control over a transition graph (``gym_pbn_amd.control``, ``pbn_stg_*_device``) without a GPU: the refusals of
the new C entry points on a host-only handle, the numpy statement of the backup (``host_backup``) against exact
rational arithmetic on the integer masses, value iteration with it against host policy iteration, and the launch-shape
header under ASan + UBSan (``make controlplancheck``).

The exact statements live here (``exact_expect``, ``exact_backup``, ``host_problem``, ``expect_bound``): the GPU tests
import them.
"""

import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

from test_attractors_host import all_states, case_network
from test_transition_host import TWO53, case_by

U53 = 2.0 ** -53
TT6_SEED = 0


# ---------------------------------------------------------------- problems on the host
def dict_rows(states, cells):
    """``[S][N]`` int32: the row of ``states[s] ^ bit(i)`` where ``cells[s][i]`` is set (-1: no row), else ``fill``."""
    states = np.ascontiguousarray(states, dtype=np.uint64)
    index = {row.tobytes(): r for r, row in enumerate(states)}
    assert len(index) == len(states)
    out = np.full(cells.shape, -1, dtype=np.int32)
    for s, i in zip(*np.nonzero(cells)):
        t = states[s].copy()
        t[i // 64] ^= np.uint64(1) << np.uint64(i % 64)
        out[s, i] = index.get(t.tobytes(), -1)
    return out


def host_nbr(states, n_nodes, nodes):
    """The flip neighbours of every row from a Python dict of the rows: -1 outside the set and for masked nodes."""
    cells = np.zeros((len(states), n_nodes), dtype=bool)
    cells[:, list(nodes)] = True
    return dict_rows(states, cells)


def host_succ(states, mass):
    """``succ`` as ``k_stg_rows`` defines it: the neighbour's row where ``mass > 0``, the row itself elsewhere."""
    t = dict_rows(states, mass > 0)
    own = np.repeat(np.arange(len(states), dtype=np.int32)[:, None], mass.shape[1], axis=1)
    return np.where(mass > 0, t, own)


def host_problem(net, states, graph, target_rows, nodes=None):
    """``dict(mass, succ, nbr, n_movable, target, N)`` of a closed set, all on the host."""
    from gym_pbn_amd.transition import host_edge_mass

    mass = host_edge_mass(net, states, graph)
    first = 1 if graph == "step" else 0
    N = net.n_nodes
    succ = host_succ(states, mass)
    assert (succ >= 0).all(), "the set is not closed"
    nodes = range(first, N) if nodes is None else nodes
    target = np.zeros(len(states), dtype=bool)
    target[list(target_rows)] = True
    return dict(mass=mass, succ=succ, nbr=host_nbr(states, N, nodes), n_movable=N - first, target=target, N=N)


@functools.lru_cache(maxsize=None)
def golden_problem():
    """Golden net (8, 2, 6) over all 256 states; target: rows 3, 77 and 200."""
    return host_problem(case_network(case_by(8, 2, 6)), all_states(8), None, (3, 77, 200))


def tt_network(n, k, seed):
    from gym_pbn_amd.network import TruthTableNetwork, synthetic_truth_table_pbn

    return TruthTableNetwork.from_pbn_data(synthetic_truth_table_pbn(n, k, seed))


def node0_clear_states(n):
    return (np.arange(1 << (n - 1), dtype=np.uint64) << np.uint64(1)).reshape(-1, 1)


@functools.lru_cache(maxsize=None)
def tt6_problem():
    """``synthetic_truth_table_pbn(6, 3, seed)`` under ``"step"`` over the 32 states with node 0 clear; target: rows 5, 18."""
    return host_problem(tt_network(6, 3, TT6_SEED), node0_clear_states(6), "step", (5, 18))


PROBLEMS = {"golden-N8": golden_problem, "tt6-step": tt6_problem}


# ---------------------------------------------------------------- exact arithmetic
def exact_expect(mass, succ, n_movable, v):
    """``E[v(next) | s]`` as ``Fraction``s from the integer masses and the doubles ``v`` (exact rationals)."""
    den = TWO53 * n_movable
    fv = [Fraction(float(x)) for x in v]
    out = []
    for s in range(len(fv)):
        e = fv[s]
        for i in np.flatnonzero(mass[s]):
            e += Fraction(int(mass[s, i]), den) * (fv[int(succ[s, i])] - fv[s])
        out.append(e)
    return out


def expect_bound(n_nodes, vmax):
    """``(2 N + 8) * 2**-53 * max|v|``: see ``test_host_backup_against_exact_arithmetic``."""
    return (2 * n_nodes + 8) * U53 * float(vmax)


def backup_bound(n_nodes, hmax, action_cost):
    """The bound on ``Ua`` (and so on ``U``, ``V'``): ``expect_bound(N, max|h|) + k * expect_bound(N, 1) + 2 u (max|h| +
    k)``: see ``test_host_backup_against_exact_arithmetic``."""
    k = abs(float(action_cost))
    return expect_bound(n_nodes, hmax) + k * expect_bound(n_nodes, 1.0) + 2 * U53 * (float(hmax) + k)


def float_h(target, v, R, c, gamma):
    """``h`` as every implementation computes it: two roundings, the same on host and device."""
    return np.where(target, float(R), gamma * np.asarray(v, np.float64) - float(c))


def exact_backup(p, v, R, c, k, gamma):
    """``(U, Ua, V', Q)`` as ``Fraction``s, from the doubles ``h = float_h(v)``: ``Q[s]`` maps an action (-1 or a
    node) to its exact value."""
    h = float_h(p["target"], v, R, c, gamma)
    u = exact_expect(p["mass"], p["succ"], p["n_movable"], h)
    nt = exact_expect(p["mass"], p["succ"], p["n_movable"], (~p["target"]).astype(np.float64))
    ua = [a - Fraction(float(k)) * b for a, b in zip(u, nt)]
    q = []
    for s in range(len(u)):
        qs = {-1: u[s]}
        for i in np.flatnonzero(p["nbr"][s] >= 0):
            qs[int(i)] = ua[int(p["nbr"][s, i])]
        q.append(qs)
    return u, ua, [max(qs.values()) for qs in q], q, h


# ---------------------------------------------------------------- refusals of the C entry points
def test_refusals_of_every_new_entry_point():
    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import Net

    lib = _lib.lib
    pm = Net(case_network(case_by(10, 2, 0)))
    s = np.ascontiguousarray(all_states(10)[:5])
    h = C.c_void_p()
    assert lib.pbn_stg_create(pm.handle, -1, 0, _lib.ptr(s, _lib._u64p), 5, C.byref(h)) == 0
    fake = C.c_void_p(64)  # never dereferenced: every call below is refused first
    err = _lib.last_error
    INV, RNG, STATE = _lib.PBN_E_INVALID, _lib.PBN_E_RANGE, _lib.PBN_E_STATE
    mask = np.array([0x3FF], dtype=np.uint64)
    pm_ = _lib.ptr(mask, _lib._u64p)
    # pbn_stg_flip_rows_device
    assert lib.pbn_stg_flip_rows_device(None, 0, 1, pm_, fake) == INV and err() == "stg is NULL"
    for first, n in ((6, 0), (0, 6), (5, 1), (3, 3), (1 << 63, 1 << 63)):
        assert lib.pbn_stg_flip_rows_device(h, first, n, pm_, fake) == RNG, (first, n)
        assert "reach past the 5 states" in err()
    for stray in (1 << 10, 1 << 63, 0x7FF):
        bad = np.array([stray], dtype=np.uint64)
        assert lib.pbn_stg_flip_rows_device(h, 0, 5, _lib.ptr(bad, _lib._u64p), fake) == INV
        assert err() == "action_mask has bits set beyond node 9"
    assert lib.pbn_stg_flip_rows_device(h, 0, 5, pm_, None) == INV and err() == "d_nbr is NULL"
    for m in (pm_, None, _lib.ptr(np.zeros(1, np.uint64), _lib._u64p)):
        for first, n in ((0, 5), (4, 1), (5, 0)):
            assert lib.pbn_stg_flip_rows_device(h, first, n, m, fake) == STATE and "host-only" in err()
    # pbn_stg_expect_device
    args = [fake, fake, fake, fake, None, 0.0, None]
    assert lib.pbn_stg_expect_device(None, *args) == INV and err() == "stg is NULL"
    for k, name in enumerate(("d_mass", "d_succ", "d_v", "d_out")):
        a = list(args)
        a[k] = None
        assert lib.pbn_stg_expect_device(h, *a) == INV and err() == f"{name} is NULL"
    assert lib.pbn_stg_expect_device(h, fake, fake, fake, fake, fake, 1.0, None) == INV and err() == "d_out_pen is NULL"
    assert lib.pbn_stg_expect_device(h, *args) == STATE and "host-only" in err()
    assert lib.pbn_stg_expect_device(h, fake, fake, fake, fake, fake, 1.0, fake) == STATE
    # pbn_stg_backup_device
    args = [fake] * 5
    assert lib.pbn_stg_backup_device(None, *args) == INV and err() == "stg is NULL"
    for k, name in enumerate(("d_nbr", "d_u", "d_ua", "d_v", "d_policy")):
        a = list(args)
        a[k] = None
        assert lib.pbn_stg_backup_device(h, *a) == INV and err() == f"{name} is NULL"
    assert lib.pbn_stg_backup_device(h, *args) == STATE and "host-only" in err()
    # pbn_stg_lookup_device
    assert lib.pbn_stg_lookup_device(None, fake, 1, fake) == INV and err() == "stg is NULL"
    assert lib.pbn_stg_lookup_device(h, None, 1, fake) == INV and err() == "d_words is NULL"
    assert lib.pbn_stg_lookup_device(h, fake, 1, None) == INV and err() == "d_rows is NULL"
    assert lib.pbn_stg_lookup_device(h, fake, (1 << 32) + 1, fake) == RNG and "PBN_STG_LOOKUP_MAX" in err()
    for n in (0, 1, 1 << 32):
        assert lib.pbn_stg_lookup_device(h, fake, n, fake) == STATE and "host-only" in err()
    lib.pbn_stg_destroy(h)
    # a mask of two words: the last word's stray bits only
    from test_attractors_host import embed_network

    big = Net(embed_network(case_network(case_by(10, 2, 0)), 65, list(range(55, 65))))
    w = np.zeros((1, 2), dtype=np.uint64)
    assert lib.pbn_stg_create(big.handle, -1, 0, _lib.ptr(w, _lib._u64p), 1, C.byref(h)) == 0
    ok = np.array([0xFFFFFFFFFFFFFFFF, 1], dtype=np.uint64)
    assert lib.pbn_stg_flip_rows_device(h, 0, 1, _lib.ptr(ok, _lib._u64p), fake) == STATE
    bad = np.array([0, 2], dtype=np.uint64)
    assert lib.pbn_stg_flip_rows_device(h, 0, 1, _lib.ptr(bad, _lib._u64p), fake) == INV
    assert err() == "action_mask has bits set beyond node 64"
    lib.pbn_stg_destroy(h)


def test_python_objects_refuse_a_host_only_graph():
    import gym_pbn_amd
    from gym_pbn_amd import _lib
    from gym_pbn_amd.control import ControlProblem, ControlSolution, host_backup
    from gym_pbn_amd.transition import TransitionGraph

    assert gym_pbn_amd.ControlProblem is ControlProblem and gym_pbn_amd.host_backup is host_backup
    assert gym_pbn_amd.ControlSolution is ControlSolution
    g = TransitionGraph(case_network(case_by(10, 2, 0)), all_states(10), device=None)
    with pytest.raises(_lib.PbnError) as ei:
        ControlProblem(g, np.zeros(1024, dtype=bool))
    assert ei.value.code == _lib.PBN_E_STATE
    with pytest.raises(_lib.PbnError) as ei:
        g.row_of(np.zeros((1, 1), dtype=np.int64))
    assert ei.value.code == _lib.PBN_E_STATE
    g.close()


def test_for_env_refuses_large_networks():
    from types import SimpleNamespace

    from gym_pbn_amd.control import ControlProblem

    with pytest.raises(ValueError, match="2\\*\\*24"):
        ControlProblem.for_env(SimpleNamespace(N=26))


# ---------------------------------------------------------------- host_backup against exact arithmetic
@pytest.mark.parametrize("name", sorted(PROBLEMS))
@pytest.mark.parametrize("scale", [1.0, 1e6])
def test_host_backup_against_exact_arithmetic(name, scale):
    """``U``, ``V'`` and the policy's value against ``Fraction`` arithmetic on the integer masses.

    **The bound of one expectation**, first order in ``u = 2**-53``. The float64 value is ``v_s + (sum_i m_i d_i) *
    2**-53 / n`` with ``d_i = fl(v_t - v_s)``, ``|d_i| <= 2 max|v|``; ``m_i`` is an exact double and the scaling by
    ``2**-53`` is exact. With ``p_i = m_i / (2**53 n)``, ``sum_i p_i <= 1``: each of the ``N`` terms carries one rounded
    difference and one rounded product (``2 u p_i |d_i|``), the sum of ``N`` terms adds at most ``N - 1`` roundings of
    partial sums that are at most ``sum_i p_i |d_i|`` after scaling (``(N - 1) u * 2 max|v|``, in any order), the
    division is one rounding of a number of size at most ``2 max|v|`` and the final add one rounding of a number of
    size at most ``max|v|``: ``(4 + 2 (N - 1) + 2 + 1) u max|v| = (2 N + 5) u max|v| <= (2 N + 8) * 2**-53 * max|v|``.

    **The backup.** ``h`` is computed in doubles (two roundings, the same in every implementation) and the exact
    side starts from those doubles, so ``U = E[h]`` is held to ``expect_bound(N, max|h|)``. ``Ua = fl(U - fl(k * nT))``:
    the error of ``U``, ``k`` times the error of ``nT = E[1 - T]`` (``expect_bound(N, 1)``), one rounded product of size
    at most ``k`` and one rounded difference of size at most ``max|h| + k``: ``backup_bound``. ``V'`` is a max of such
    numbers, and the policy is held to value: its exact ``Q`` is within twice that bound of the exact max."""
    from gym_pbn_amd.control import host_backup, host_expect

    p = PROBLEMS[name]()
    N, S = p["N"], len(p["target"])
    R, c, k, gamma = 20, 4, 1, 0.99
    v = np.random.default_rng(11).uniform(-1.0, 1.0, size=S) * scale
    # one expectation, of v itself
    got = host_expect(p["mass"], p["succ"], p["n_movable"], v)
    want = exact_expect(p["mass"], p["succ"], p["n_movable"], v)
    dev = max(abs(Fraction(float(g)) - w) for g, w in zip(got, want))
    bound = expect_bound(N, np.abs(v).max())
    print(f"{name} scale {scale:g}: expect deviates {float(dev):.3e}, bound {bound:.3e}")
    assert dev <= bound
    assert np.array_equal(host_expect(p["mass"], p["succ"], p["n_movable"], np.ones(S)), np.ones(S))
    # the backup
    v_new, pi, u, ua = host_backup(p["mass"], p["succ"], p["nbr"], p["n_movable"], p["target"], v, reward_target=R,
                                   step_cost=c, action_cost=k, gamma=gamma, full=True)
    xu, xua, xv, xq, h = exact_backup(p, v, R, c, k, gamma)
    hmax = np.abs(h).max()
    b_u, b_a = expect_bound(N, hmax), backup_bound(N, hmax, k)
    d_u = max(abs(Fraction(float(a)) - b) for a, b in zip(u, xu))
    d_a = max(abs(Fraction(float(a)) - b) for a, b in zip(ua, xua))
    d_v = max(abs(Fraction(float(a)) - b) for a, b in zip(v_new, xv))
    print(f"{name} scale {scale:g}: U {float(d_u):.3e} (bound {b_u:.3e}), Ua {float(d_a):.3e}, V' {float(d_v):.3e} "
          f"(bound {b_a:.3e})")
    assert d_u <= b_u and d_a <= b_a and d_v <= b_a
    assert pi.dtype == np.int32 and pi.shape == (S,)
    for s in range(S):
        assert int(pi[s]) in xq[s], (s, int(pi[s]))  # an action of that state: never nbr == -1, never a masked node
        assert xq[s][int(pi[s])] >= xv[s] - 2 * b_a
    assert (pi >= 0).any()


def test_host_backup_ties_and_no_actions():
    """No action allowed: ``V' = U`` and ``pi = -1``. Ties: the no-op first, then the lowest node."""
    from gym_pbn_amd.control import host_backup

    p = golden_problem()
    S = 256
    v = np.random.default_rng(3).normal(size=S)
    none = np.full_like(p["nbr"], -1)
    v_new, pi, u, _ = host_backup(p["mass"], p["succ"], none, p["n_movable"], p["target"], v, full=True)
    assert np.array_equal(v_new, u) and (pi == -1).all()
    # action_cost 0 and a constant v: every action has the value of the no-op wherever nT agrees -- the no-op wins
    v_new, pi = host_backup(p["mass"], p["succ"], p["nbr"], p["n_movable"], np.zeros(S, bool), np.zeros(S),
                            action_cost=0)
    assert (pi == -1).all() and np.array_equal(v_new, np.full(S, -4.0))
    # rows whose best flips tie exactly: hand-made arrays, two states, both flips lead to the other state
    mass = np.zeros((2, 2), dtype=np.uint64)
    succ = np.array([[0, 0], [1, 1]], dtype=np.int32)
    nbr = np.array([[1, 1], [0, 0]], dtype=np.int32)
    v_new, pi = host_backup(mass, succ, nbr, 2, np.array([False, True]), np.zeros(2), gamma=0.5)
    assert pi.tolist() == [0, -1] and v_new.tolist() == [20.0, 20.0]


# ---------------------------------------------------------------- optimality
def policy_system(p, pi, R, c, k, gamma):
    """``(A, b)`` with ``A V = b`` the evaluation of policy ``pi``: ``V[s] = sum_s' P(s' | t) (T[s'] R + (1 - T[s'])
    (-c - k [flip] + gamma V[s']))``, ``t`` the row the action leads to."""
    S, N = p["mass"].shape
    prob = p["mass"].astype(np.float64) / float(TWO53 * p["n_movable"])
    P = np.zeros((S, S))
    for i in range(N):
        np.add.at(P, (np.arange(S), p["succ"][:, i]), prob[:, i])
    P[np.arange(S), np.arange(S)] += 1.0 - prob.sum(axis=1)
    flip = pi >= 0
    t = np.where(flip, p["nbr"][np.arange(S), np.maximum(pi, 0)], np.arange(S))
    assert (t >= 0).all()
    Pt = P[t]
    notT = (~p["target"]).astype(np.float64)
    A = np.eye(S) - gamma * Pt * notT[None, :]
    b = Pt @ np.where(p["target"], float(R), 0.0) - (Pt @ notT) * (c + k * flip)
    return A, b


def evaluate_exactly(p, pi, R, c, k, gamma):
    """``(V, err)``: ``numpy.linalg.solve`` of the policy's system and an a-posteriori bound on its own error, ``||A V -
    b||_inf / (1 - gamma)`` (``A = I - gamma M`` with ``||M||_inf <= 1``, so ``||A^-1||_inf <= 1 / (1 - gamma)``)."""
    A, b = policy_system(p, pi, R, c, k, gamma)
    V = np.linalg.solve(A, b)
    return V, np.abs(A @ V - b).max() / (1.0 - gamma)


def greedy(p, V, R, c, k, gamma):
    from gym_pbn_amd.control import host_backup

    return host_backup(p["mass"], p["succ"], p["nbr"], p["n_movable"], p["target"], V, reward_target=R, step_cost=c,
                       action_cost=k, gamma=gamma)[1]


def policy_iteration(p, R, c, k, gamma):
    """Howard's policy iteration from the all-no-op policy: ``(V*, pi*, err)``. An action is changed only where it
    gains more than ``1e-9`` (so equal-valued actions cannot cycle)."""
    S = len(p["target"])
    pi = np.full(S, -1, dtype=np.int32)
    for _ in range(200):
        V, err = evaluate_exactly(p, pi, R, c, k, gamma)
        g = greedy(p, V, R, c, k, gamma)
        Vg = evaluate_exactly(p, g, R, c, k, gamma)[0]
        if (Vg <= V + 1e-9).all():
            return V, pi, err
        pi = g
    raise AssertionError("policy iteration did not settle")


def value_iteration(p, R, c, k, gamma, tol=1e-10, max_iters=5000):
    from gym_pbn_amd.control import host_backup, host_expect

    S = len(p["target"])
    n_t = host_expect(p["mass"], p["succ"], p["n_movable"], (~p["target"]).astype(np.float64))
    v = np.zeros(S)
    for it in range(1, max_iters + 1):
        nxt, pi = host_backup(p["mass"], p["succ"], p["nbr"], p["n_movable"], p["target"], v, reward_target=R,
                              step_cost=c, action_cost=k, gamma=gamma, n_t=n_t)
        r = np.abs(nxt - v).max()
        v = nxt
        if r <= tol:
            break
    return v, pi, r, it


def sweep_eps(N, R, c, k, gamma):
    """The rounding of one sweep, a priori: ``|V| <= M = max(R, (c + k) / (1 - gamma))`` at every iterate from 0, so
    ``|h| <= M + c``; ``backup_bound`` of that, plus the two roundings of ``h`` itself (``2 u (M + c)``)."""
    M = max(R, (c + k) / (1.0 - gamma))
    return backup_bound(N, M + c, k) + 2 * U53 * (M + c)


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_value_iteration_reaches_the_optimum_of_policy_iteration(name):
    """``gamma = 0.9``. Value iteration run to residual ``r`` is within ``gamma / (1 - gamma) * r`` of the fixed point of
    the rounded backup, which is within ``eps / (1 - gamma)`` of ``V*`` (``eps``: ``sweep_eps``); the reference's own
    error (``evaluate_exactly``) is added. Its greedy policy's exact value is held to the same band."""
    p = PROBLEMS[name]()
    R, c, k, gamma = 20, 4, 1, 0.9
    Vs, pis, err = policy_iteration(p, R, c, k, gamma)
    v, pi, r, iters = value_iteration(p, R, c, k, gamma)
    band = gamma / (1.0 - gamma) * r + sweep_eps(p["N"], R, c, k, gamma) / (1.0 - gamma) + err
    dev = np.abs(v - Vs).max()
    print(f"{name}: {iters} sweeps, residual {r:.3e}, |V - V*| {dev:.3e}, band {band:.3e} (reference error {err:.1e}); "
          f"{int((pis >= 0).sum())} of {len(pis)} states flip, V* in [{Vs.min():.3f}, {Vs.max():.3f}]")
    assert r <= 1e-10 and dev <= band
    Vg, err_g = evaluate_exactly(p, pi, R, c, k, gamma)
    dev_g = np.abs(Vg - Vs).max()
    print(f"{name}: greedy policy's value deviates {dev_g:.3e}")
    assert dev_g <= band + err_g
    assert (pis >= 0).any() and (Vs >= evaluate_exactly(p, np.full(len(pis), -1, np.int32), R, c, k, gamma)[0] - band).all()


# ---------------------------------------------------------------- the launch-shape header
@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ is not installed")
def test_control_plan_header_is_clean_under_asan_and_ubsan():
    """``make controlplancheck``: tests/host/control_plan_check.cpp on csrc/pbn_control_plan.hpp (no HIP header, no
    library, no GPU) with ASan + UBSan: the plan against a restatement of its rule, and the kernels' walk replayed."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(["make", "-C", str(root / "gym-pbn-stac_amd"), "controlplancheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "control_plan_check ok" in r.stdout
