"""Optimal control over a transition graph on the device (``csrc/pbn_control.hip``; ``gym_pbn_amd.control``).

``nbr`` is checked bit for bit against a Python dict of the rows. The float64 kernels are checked against exact
``Fraction`` arithmetic on the integer masses where the set is small and against the numpy statement (``host_backup``)
elsewhere, within the rounding bounds derived in ``test_control_host.py``; the policy is held to value, not to
equality. The closed loop runs the optimal policy in ``TorchVecPBNEnv`` and compares the discounted return with ``V*``.
"""

import functools
from fractions import Fraction

import numpy as np
import pytest

from test_attractors_host import all_states, case_attractors, case_network, embed_network, lift_states
from test_control_host import (U53, backup_bound, exact_expect, expect_bound, host_nbr, node0_clear_states,
                               sweep_eps, tt_network)
from test_transition_host import case_by

pytestmark = pytest.mark.gpu

EXACT_MAX_CELLS = 1 << 14  # Fraction arithmetic up to this many cells, numpy above


# ---------------------------------------------------------------- the state sets
def _golden_53():
    c = case_by(8, 2, 2)
    att = next(a for a in case_attractors(c) if len(a) == 53)
    return case_network(c), att, None


def _golden_1024():
    return case_network(case_by(10, 2, 0)), all_states(10), None


def _bittner28_120():
    from test_transition_gpu import bittner28_attractor_120

    res, k = bittner28_attractor_120()
    return res.network, res.attractors[k], None


def _embedded(n_total):
    small = case_network(case_by(10, 2, 0))
    place = list(range(n_total - 10, n_total))
    frozen = np.random.default_rng(5).integers(0, 2, size=n_total, dtype=np.uint8)
    return embed_network(small, n_total, place), lift_states(all_states(10), 10, n_total, place, frozen), None


def _tt9():
    return tt_network(9, 3, 0), node0_clear_states(9), "step"


def _tt_all(n, k):
    return tt_network(n, k, 0), all_states(n), "stg"


def _frozen_1():
    """One node that copies itself: the two states never move, and the flip of node 0 swaps them."""
    return embed_network(case_network(case_by(10, 2, 0)), 1, []), all_states(1), None


SETS = {
    "golden-N8-att53": _golden_53,          # G = 8, a partial last wave, flips leave the set
    "golden-N10-all": _golden_1024,         # G = 16 with idle lanes, closed under flips
    "bittner28-att120": _bittner28_120,     # G = 32
    "embedded-65": lambda: _embedded(65),   # W = 2, two strides per row, the second nearly empty
    "embedded-257": lambda: _embedded(257), # W = 5, five strides per row
    "tt9-step": _tt9,                       # first_node = 1, n_movable = 8
    # the remaining group sizes: every kernel instantiation runs
    "frozen-1": _frozen_1,                  # G = 1, no shuffle
    "tt2-stg": lambda: _tt_all(2, 1),       # G = 2
    "tt3-stg": lambda: _tt_all(3, 2),       # G = 4
    "embedded-40": lambda: _embedded(40),   # G = 64 with one cell per lane: the four-row trip at the full wave
}
FULL_SPACES = ("golden-N10-all", "tt9-step", "frozen-1", "tt2-stg", "tt3-stg")  # closed under flips


@functools.lru_cache(maxsize=None)
def device_set(name):
    """``(graph, states, mass, succ)`` of a set, built once for the module: the graph on the device, its integer
    arrays as numpy (pinned bit for bit by ``test_transition_gpu.py``)."""
    from gym_pbn_amd.transition import TransitionGraph

    net, states, graph = SETS[name]()
    states = np.ascontiguousarray(states, dtype=np.uint64)
    g = TransitionGraph(net, states, table_graph=graph)
    assert g.closed
    return g, states, g.mass.cpu().numpy().astype(np.uint64), g.succ.cpu().numpy()


def target_rows(S):
    return [S - 1] if S <= 8 else sorted({1, S // 3, (2 * S) // 3 + 1})


def host_target(S):
    t = np.zeros(S, dtype=bool)
    t[target_rows(S)] = True
    return t


# ---------------------------------------------------------------- nbr
@pytest.mark.parametrize("masked", [False, True], ids=["movable", "masked"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_nbr_bit_for_bit(name, masked):
    """``nbr`` against a dict of the rows: the row of every allowed flip, -1 where it leaves the set, -1 for every
    node that is not allowed (every third movable node here, or the default: the movable nodes)."""
    from gym_pbn_amd.control import ControlProblem

    g, states, _, _ = device_set(name)
    N, S = g.n_nodes, g.n_states
    nodes = list(range(g.first_node, N, 3)) if masked else None
    p = ControlProblem(g, host_target(S), nodes=nodes)
    allowed = list(range(g.first_node, N)) if nodes is None else nodes
    assert p.nodes == allowed
    import torch

    assert p.nbr.dtype == torch.int32 and tuple(p.nbr.shape) == (S, N) and p.nbr.is_cuda
    got = p.nbr.cpu().numpy()
    want = host_nbr(states, N, allowed)
    assert np.array_equal(got, want)
    off = [i for i in range(N) if i not in set(allowed)]
    assert (got[:, off] == -1).all()
    leaves = bool((want[:, allowed] < 0).any())
    assert leaves == (name not in FULL_SPACES)
    if leaves:
        with pytest.raises(ValueError, match="leave the state set"):
            ControlProblem(g, host_target(S), nodes=nodes, strict=True)
    else:
        ControlProblem(g, host_target(S), nodes=nodes, strict=True)


def test_row_of_device_words():
    """``row_of``: the rows of a shuffled copy of the states and of states outside the set, W = 1 and W = 5."""
    import torch

    for name in ("golden-N8-att53", "embedded-257"):
        g, states, _, _ = device_set(name)
        S, W = states.shape
        perm = np.random.default_rng(1).permutation(S)
        out = states[perm].copy()
        if W == 1:  # every seventh: a state of the complement
            rest = np.setdiff1d(np.arange(1 << g.n_nodes, dtype=np.uint64), states[:, 0])
            out[::7, 0] = rest[: len(out[::7])]
        else:  # every seventh: a frozen node flipped
            out[::7, 0] ^= np.uint64(1)
        index = {row.tobytes(): r for r, row in enumerate(states)}
        want = np.array([index.get(r.tobytes(), -1) for r in out], dtype=np.int32)
        words = torch.from_numpy(out.view(np.int64)).to("cuda:0")
        got = g.row_of(words)
        assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        assert (want < 0).any() and (want >= 0).any()
        assert g.row_of(words[:0]).shape == (0,)
        with pytest.raises(ValueError, match="int64"):
            g.row_of(words.to(torch.int32))


# ---------------------------------------------------------------- expect
@pytest.mark.parametrize("scale", [1.0, 1e6])
@pytest.mark.parametrize("name", sorted(SETS))
def test_expect_against_exact_arithmetic(name, scale):
    """``expect(v)`` within ``expect_bound`` of the exact value where ``S * N <= 2**14``, within twice that bound of
    ``host_expect`` elsewhere (both sides are within the bound of the exact value); ``expect(1) == 1`` exactly; and
    against ``pull(v)`` within the sum of both bounds. ``pull``'s own bound has the same form: ``p_i`` carries one
    rounding (``u p_i |v|`` summed: ``u max|v|``), the ``N`` products one each (``u max|v|`` in all, the weights sum to
    at most 1), the sum ``N - 1`` additions, ``stay = 1 - sum p`` ``N + 1`` roundings of numbers at most 1, the stay
    product and the final add one each: ``(2 N + 4) u max|v| <= (2 N + 8) * 2**-53 * max|v|``."""
    import torch

    from gym_pbn_amd.control import host_expect

    g, states, mass, succ = device_set(name)
    N, S = g.n_nodes, g.n_states
    v = np.random.default_rng(17).uniform(-1.0, 1.0, size=S) * scale
    got_t = g.expect(v)
    assert got_t.dtype == torch.float64 and got_t.is_cuda and tuple(got_t.shape) == (S,)
    got = got_t.cpu().numpy()
    bound = expect_bound(N, np.abs(v).max())
    if S * N <= EXACT_MAX_CELLS:
        want = exact_expect(mass, succ, g.n_movable, v)
        dev = float(max(abs(Fraction(float(a)) - b) for a, b in zip(got, want)))
        print(f"{name} scale {scale:g}: expect deviates {dev:.3e} from the exact value, bound {bound:.3e}")
        assert dev <= bound
    else:
        dev = np.abs(got - host_expect(mass, succ, g.n_movable, v)).max()
        print(f"{name} scale {scale:g}: expect deviates {dev:.3e} from host_expect, bound 2 x {bound:.3e}")
        assert dev <= 2 * bound
    assert torch.equal(g.expect(torch.ones(S, dtype=torch.float64, device="cuda:0")),
                       torch.ones(S, dtype=torch.float64, device="cuda:0"))
    dev = np.abs(got - g.pull(v).cpu().numpy()).max()
    print(f"{name} scale {scale:g}: expect deviates {dev:.3e} from pull, bound {2 * bound:.3e}")
    assert dev <= 2 * bound
    # the penalised output of the same pass: out - cost * pen, two roundings
    pen = np.random.default_rng(18).uniform(0.0, 1.0, size=S)
    out, out_pen = g.expect(v, pen=pen, cost=1.5)
    assert torch.equal(out, got_t)
    assert np.abs(out_pen.cpu().numpy() - (got - 1.5 * pen)).max() <= 2 * U53 * (np.abs(v).max() + 1.5)


def test_expect_is_deterministic_and_independent_of_the_grid(monkeypatch):
    """Two calls give identical bits, and three workgroups over the 4,096 rows of golden (12, 3, 1) (``PBNSIM_STG_GRID``:
    every group walks the grid-stride loop) give the bits of the uncapped run -- ``expect``, ``backup`` and ``nbr``."""
    import torch

    from gym_pbn_amd.control import ControlProblem
    from gym_pbn_amd.transition import TransitionGraph

    net = case_network(case_by(12, 3, 1))
    S = 4096
    v = torch.from_numpy(np.random.default_rng(2).normal(size=S) * 1e3).to("cuda:0")
    g = TransitionGraph(net, all_states(12))
    a, b = g.expect(v), g.expect(v)
    assert torch.equal(a, b)
    p = ControlProblem(g, host_target(S))
    va, pa = p.backup(v)
    vb, pb = p.backup(v)
    assert torch.equal(va, vb) and torch.equal(pa, pb)
    # under a torch stream of the caller's: the sweep's torch ops and the library's launches stay in order
    twenty = p.solve(tol=0.0, max_iters=20, check_every=20)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vs, ps = p.backup(v)
        again = p.solve(tol=0.0, max_iters=20, check_every=20)
        es = g.expect(v)
    side.synchronize()
    assert torch.equal(vs, va) and torch.equal(ps, pa) and torch.equal(es, a)
    assert torch.equal(again.v, twenty.v) and torch.equal(again.policy, twenty.policy) and again.residual == twenty.residual
    monkeypatch.setenv("PBNSIM_STG_GRID", "3")
    g3 = TransitionGraph(net, all_states(12))
    assert torch.equal(g3.expect(v), a)
    p3 = ControlProblem(g3, host_target(S))
    assert torch.equal(p3.nbr, p.nbr)
    v3, pi3 = p3.backup(v)
    assert torch.equal(v3, va) and torch.equal(pi3, pa)


# ---------------------------------------------------------------- backup
@pytest.mark.parametrize("name", sorted(SETS))
def test_backup_against_host_backup(name):
    """``V'`` within ``backup_bound`` of ``host_backup``. The policy is held to value: ``Q_host(s, pi_dev[s]) >= max_a
    Q_host(s, a) - 2 * bound``, never an action with ``nbr == -1`` and never a masked node. With no node allowed
    ``V' == U`` bit for bit and ``pi == -1``."""
    import torch

    from gym_pbn_amd.control import ControlProblem, host_backup

    g, states, mass, succ = device_set(name)
    N, S = g.n_nodes, g.n_states
    R, c, k, gamma = 20, 4, 1, 0.99
    T = host_target(S)
    nodes = list(range(g.first_node, N, 2))
    v = np.random.default_rng(23).uniform(-30.0, 30.0, size=S)
    for allowed in (None, nodes):
        p = ControlProblem(g, T, gamma=gamma, nodes=allowed)
        nbr = host_nbr(states, N, p.nodes)
        v_dev, pi_dev = p.backup(v)
        assert v_dev.dtype == torch.float64 and pi_dev.dtype == torch.int32
        v_dev, pi_dev = v_dev.cpu().numpy(), pi_dev.cpu().numpy()
        v_host, pi_host, u, ua = host_backup(mass, succ, nbr, g.n_movable, T, v, reward_target=R, step_cost=c,
                                             action_cost=k, gamma=gamma, full=True)
        hmax = max(R, gamma * np.abs(v).max() + c)
        bound = backup_bound(N, hmax, k)
        dev = np.abs(v_dev - v_host).max()
        print(f"{name} ({len(p.nodes)} nodes): V' deviates {dev:.3e}, bound {bound:.3e}; policies agree at "
              f"{int((pi_dev == pi_host).sum())} of {S} states")
        assert dev <= bound
        assert ((pi_dev >= -1) & (pi_dev < N)).all()
        flip = pi_dev >= 0
        to = nbr[np.arange(S), np.maximum(pi_dev, 0)]
        assert (to[flip] >= 0).all() and np.isin(pi_dev[flip], p.nodes).all()
        q_taken = np.where(flip, ua[np.maximum(to, 0)], u)
        assert (q_taken >= v_host - 2 * bound).all()
        assert flip.any() or S <= 8  # a tiny set's random v may leave nothing to gain
        ud, uad = p.q_values(v)
        assert np.abs(ud.cpu().numpy() - u).max() <= bound and np.abs(uad.cpu().numpy() - ua).max() <= bound
    p = ControlProblem(g, T, gamma=gamma, nodes=[])
    assert (p.nbr == -1).all().item()
    v_dev, pi_dev = p.backup(v)
    assert torch.equal(v_dev, p.q_values(v)[0]) and (pi_dev == -1).all().item()


def test_backup_ties_prefer_the_no_op_then_the_lowest_node():
    """No target, ``v = 0``, ``action_cost = 0``: every action is worth ``-step_cost`` exactly (a constant comes back
    from ``expect`` exactly), so the no-op wins everywhere. With a negative action cost of ``-1`` every flip is worth
    ``-step_cost + 1`` exactly (``nT == 1``) and the lowest allowed node that stays in the set wins."""
    from gym_pbn_amd.control import ControlProblem

    for name in ("golden-N8-att53", "embedded-65"):
        g, states, _, _ = device_set(name)
        S, N = g.n_states, g.n_nodes
        none = np.zeros(S, dtype=bool)
        v_new, pi = ControlProblem(g, none, action_cost=0).backup(np.zeros(S))
        assert (pi == -1).all().item() and (v_new == -4.0).all().item()
        nodes = list(range(1, N))
        p = ControlProblem(g, none, action_cost=-1, nodes=nodes)
        v_new, pi = p.backup(np.zeros(S))
        nbr = host_nbr(states, N, nodes)
        want = np.array([next((i for i in nodes if nbr[s, i] >= 0), -1) for s in range(S)], dtype=np.int32)
        assert np.array_equal(pi.cpu().numpy(), want)
        assert np.array_equal(v_new.cpu().numpy(), np.where(want >= 0, -3.0, -4.0))
        assert (want >= 0).any() and (name != "golden-N8-att53" or len(set(want.tolist())) > 2)


# ---------------------------------------------------------------- solve
def solve_band(N, R, c, k, gamma, residual):
    """Value iteration stopped at sup-norm change ``residual``: within ``gamma / (1 - gamma) * residual`` of the fixed
    point of the rounded backup, which is within ``sweep_eps / (1 - gamma)`` of the exact one."""
    return gamma / (1.0 - gamma) * residual + sweep_eps(N, R, c, k, gamma) / (1.0 - gamma)


@pytest.mark.parametrize("name", ["golden-N10-all", "tt9-step"])
def test_solve_against_host_value_iteration(name):
    """``gamma = 0.9``. The device ``V`` after ``n`` sweeps against the host ``V`` after the same ``n`` sweeps from the
    same start: each sweep adds at most its own rounding (``sweep_eps``, device and host) to a difference the backup
    contracts by ``gamma``: ``(eps_dev + eps_host) (1 - gamma**n) / (1 - gamma)``. And ``V* >= evaluate(all no-op)`` at
    every state, up to both solve bands."""
    import torch

    from gym_pbn_amd.control import ControlProblem, ControlSolution, host_backup, host_expect

    g, states, mass, succ = device_set(name)
    N, S = g.n_nodes, g.n_states
    R, c, k, gamma, n = 20, 4, 1, 0.9, 60
    T = host_target(S)
    p = ControlProblem(g, T, gamma=gamma)
    nbr = host_nbr(states, N, p.nodes)
    sol = p.solve(tol=0.0, max_iters=n, check_every=n)
    assert isinstance(sol, ControlSolution) and sol.iters == n and sol.v.dtype == torch.float64
    n_t = host_expect(mass, succ, g.n_movable, (~T).astype(np.float64))
    v = np.zeros(S)
    for _ in range(n):
        v, pi = host_backup(mass, succ, nbr, g.n_movable, T, v, reward_target=R, step_cost=c, action_cost=k,
                            gamma=gamma, n_t=n_t)
    eps = sweep_eps(N, R, c, k, gamma)
    band = 2 * eps * (1.0 - gamma ** n) / (1.0 - gamma)
    dev = np.abs(sol.v.cpu().numpy() - v).max()
    print(f"{name}: after {n} sweeps device and host differ by {dev:.3e}, band {band:.3e}; residual {sol.residual:.3e}")
    assert dev <= band
    best = p.solve(tol=1e-9)
    assert best.residual <= 1e-9 and best.iters < 100000 and best.iters % 16 == 0
    noop = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    v0, r0, it0 = p.evaluate(noop, tol=1e-9)
    assert r0 <= 1e-9
    slack = solve_band(N, R, c, k, gamma, best.residual) + solve_band(N, R, c, k, gamma, r0)
    gain = (best.v - v0).cpu().numpy()
    print(f"{name}: solve {best.iters} sweeps (residual {best.residual:.2e}), no-op {it0} sweeps; V* - V_noop in "
          f"[{gain.min():.3e}, {gain.max():.3f}], slack {slack:.2e}; {int((best.policy >= 0).sum())} states flip")
    assert (gain >= -slack).all() and gain.max() > 1.0
    # the optimal policy's own value is V*
    vp, rp, _ = p.evaluate(best.policy, tol=1e-9)
    assert np.abs((vp - best.v).cpu().numpy()).max() <= slack + solve_band(N, R, c, k, gamma, rp)
    if name == "tt9-step":  # node 0 is no action under "step"
        with pytest.raises(ValueError, match="no action there"):
            p.evaluate(torch.zeros(S, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError, match="outside"):
        p.evaluate(torch.full((S,), N, dtype=torch.int32, device="cuda:0"))


# ---------------------------------------------------------------- the closed loop
LOOP_SEED = 0
LOOP_TARGET_ROWS = (3, 40, 77, 100)
LOOP_START_ROWS = tuple(r for r in range(8, 128, 8) if r not in LOOP_TARGET_ROWS)


def test_closed_loop_return_matches_the_optimal_value():
    """The optimal policy acts in ``TorchVecPBNEnv`` from device state words, and the discounted return of 65,536 envs
    over 150 steps (stopped at each env's termination) has the mean ``V*`` promises: ``|mean(G - V[row(s0)])| <= 6
    std(G - V[row(s0)]) / sqrt(B) + gamma**150 R / (1 - gamma) + the solve band``, every env counted. The same for
    the all-no-op policy against ``evaluate``, and the two differ by more than both bands.

    Network ``synthetic_truth_table_pbn(8, 3, seed=0)``, ``gamma = 0.9``; the target is rows 3, 40, 77 and 100 of the
    128 states with node 0 clear, the starts are those and rows 8, 16, .., 120 (without 40). Chosen on the CPU with host policy
    iteration: over that start distribution the exact mean ``V*`` is 7.380 and the exact mean no-op value -28.702, a
    gap of 36.08 (seeds 1-5: 33.8 to 36.6)."""
    import torch

    from gym_pbn_amd.control import ControlProblem
    from gym_pbn_amd.network import synthetic_truth_table_pbn
    from gym_pbn_amd.torch_env import TorchVecPBNEnv

    N, B, steps, gamma = 8, 65536, 150, 0.9
    tup = lambda r: tuple(((r << 1) >> i) & 1 for i in range(N))  # noqa: E731
    target = [tup(r) for r in LOOP_TARGET_ROWS]
    starts = [tup(r) for r in LOOP_START_ROWS]
    R = TorchVecPBNEnv.REWARD_TARGET

    def run(policy_of, seed):
        env = TorchVecPBNEnv(synthetic_truth_table_pbn(N, 3, LOOP_SEED), goal_config={"target_nodes": target},
                             n_envs=B, all_attractors=[target, starts], seed=seed)
        assert len(env.target_words) == len(target)
        prob = ControlProblem.for_env(env, gamma=gamma)
        assert prob.graph.n_states == 128 and prob.nodes == list(range(1, N)) and int(prob.target.sum()) == len(target)
        assert (prob.reward_target, prob.step_cost, prob.action_cost) == (20.0, 4.0, 1.0)
        sol, v, band = policy_of(prob)
        env.reset()
        s0 = prob.graph.row_of(env.observation_words())
        assert (s0 >= 0).all().item()
        assert set(s0.unique().tolist()) == set(LOOP_TARGET_ROWS) | set(LOOP_START_ROWS)
        G = torch.zeros(B, dtype=torch.float64, device="cuda:0")
        alive = torch.ones(B, dtype=torch.bool, device="cuda:0")
        disc = 1.0
        for _ in range(steps):
            a = sol.act(env.observation_words(), check=False) if sol is not None else \
                torch.zeros(B, dtype=torch.int64, device="cuda:0")
            _, reward, term, _, _ = env.step(a)
            G += torch.where(alive, reward.to(torch.float64) * disc, torch.zeros_like(G))
            alive &= ~term
            disc *= gamma
        env.close()
        d = G - v[s0.long()]
        mean, std = float(d.mean()), float(d.std())
        allowed = 6.0 * std / np.sqrt(B) + gamma ** steps * R / (1.0 - gamma) + band
        return mean, std, allowed, float(v[s0.long()].mean()), float(G.mean()), float((~alive).double().mean())

    def optimal(prob):
        sol = prob.solve(tol=1e-9)
        assert sol.residual <= 1e-9
        with pytest.raises(ValueError, match="no row"):
            sol.act(torch.ones((1, 1), dtype=torch.int64, device="cuda:0"), check=True)  # node 0 set: not a row
        assert sol.act(torch.ones((1, 1), dtype=torch.int64, device="cuda:0")).tolist() == [0]
        return sol, sol.v, solve_band(N, 20, 4, 1, gamma, sol.residual)

    def no_op(prob):
        noop = torch.full((prob.graph.n_states,), -1, dtype=torch.int32, device="cuda:0")
        v, r, _ = prob.evaluate(noop, tol=1e-9)
        assert r <= 1e-9
        return None, v, solve_band(N, 20, 4, 1, gamma, r)

    m1, s1, a1, v1, g1, done1 = run(optimal, seed=5)
    print(f"optimal: mean V* {v1:.4f}, mean return {g1:.4f}, mean(G - V) {m1:.4e} (std {s1:.3f}), allowed {a1:.4e}; "
          f"{done1:.4f} of the envs ended")
    m0, s0, a0, v0, g0, done0 = run(no_op, seed=5)
    print(f"no-op:   mean V  {v0:.4f}, mean return {g0:.4f}, mean(G - V) {m0:.4e} (std {s0:.3f}), allowed {a0:.4e}; "
          f"{done0:.4f} of the envs ended")
    assert abs(m1) <= a1
    assert abs(m0) <= a0
    assert v1 - v0 > a1 + a0 and g1 - g0 > a1 + a0
    assert abs((v1 - v0) - 36.08) < 1.0  # the gap chosen on the CPU, up to the start draws' sampling
