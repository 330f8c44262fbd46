"""The multi-flip until-attractor MDP on the device (``csrc/pbn_flipset.hip``; ``gym_pbn_amd.multiflip``).

The max over flip sets is held bit for bit to plain enumeration (``host_multiflip_max``) on the device's own worths,
random and tied, to ``k_stg_backup`` at one flip, and to itself from call to call and under any grid. The arrival worth
``M`` is held to the host statement within twice ``arrival_bound`` (``test_multiflip_host.py``), value iteration to host
value iteration, and the closed loop runs the optimal policy in ``TorchVecPBNTargetMultiSetEnv`` and compares the
discounted return with ``V*``.
"""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from test_absorb_gpu import device_case, same_bits
from test_absorb_host import golden_case
from test_attractors_host import case_attractors, case_network
from test_control_host import U53
from test_multiflip_host import arrival_bound
from test_transition_host import case_by

pytestmark = pytest.mark.gpu

# the nodes an action may flip: tt6-step's states all have node 0 clear (a -1 column), embedded-65's set is closed
# under the flips of the ten embedded places only
NODES = {"frozen-1": [0], "tt6-step": [1, 2, 3, 4, 5], "golden-N8": list(range(8)), "golden-N10": list(range(10)),
         "embedded-65": list(range(55, 65))}


def node_mask(nodes, W):
    mask = np.zeros(W, dtype=np.uint64)
    for i in nodes:
        mask[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return mask


def flip_rows(g, nodes):
    import torch

    from gym_pbn_amd import _lib

    nbr = torch.empty((g.n_states, g.n_nodes), dtype=torch.int32, device="cuda:0")
    with g._on_default_stream(nbr.device):
        _lib.check(_lib.lib.pbn_stg_flip_rows_device(g.handle, 0, g.n_states, _lib.ptr(node_mask(nodes, g.n_words), _lib._u64p),
                                                     nbr.data_ptr()))
    return nbr


@functools.lru_cache(maxsize=None)
def flip_case(name):
    """``(graph, nodes, nbr (device), nbr (numpy))`` of a case, built once."""
    g = device_case(name)["graph"]
    nbr = flip_rows(g, NODES[name])
    host = nbr.cpu().numpy()
    off = [i for i in range(g.n_nodes) if i not in set(NODES[name])]
    assert (host[:, NODES[name]] >= 0).all() and (host[:, off] == -1).all()
    return g, NODES[name], nbr, host


def device_max(g, nbr, m, A, cost, noop=None):
    """The entry points alone: ``A`` levels and the select, ``(v, policy_end, policy_flips)`` as device tensors."""
    import torch

    from gym_pbn_amd import _lib

    S = g.n_states
    base = [torch.full((S, 2), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    tag = [torch.full((S, 2), -9, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    v = torch.empty(S, dtype=torch.float64, device="cuda:0")
    end, flips = (torch.empty(S, dtype=torch.int32, device="cuda:0") for _ in range(2))
    noop_p = None if noop is None else C.byref(C.c_double(noop))
    with g._on_default_stream(v.device):
        src = None
        for lev in range(A):
            _lib.check(_lib.lib.pbn_stg_flipset_level_device(
                g.handle, nbr.data_ptr(), m.data_ptr(), float(cost), None if src is None else src[0].data_ptr(),
                None if src is None else src[1].data_ptr(), base[lev & 1].data_ptr(), tag[lev & 1].data_ptr()))
            src = (base[lev & 1], tag[lev & 1])
        _lib.check(_lib.lib.pbn_stg_flipset_select_device(g.handle, src[0].data_ptr(), src[1].data_ptr(), m.data_ptr(),
                                                          float(cost), noop_p, v.data_ptr(), end.data_ptr(), flips.data_ptr()))
    return v, end, flips


def worths(S, kind, seed=17):
    """Random signed worths, or worths quantised to five values (quarters: every ``m - cost * d`` below is exact)."""
    u = np.random.default_rng(seed).uniform(size=S)
    return (u * 2000.0 - 1000.0) if kind == "random" else np.floor(u * 5.0) / 4.0


# ---------------------------------------------------------------- the max
@pytest.mark.parametrize("name", sorted(NODES))
def test_max_bit_for_bit_against_enumeration(name):
    """For ``A`` in 1 .. 4 and one past the number of allowed nodes, random and tied worths, costs 1 and 0, ``noop_cost``
    None, 0 and 2: ``v`` bit-equal to ``host_multiflip_max`` on the same ``m``, ``policy_end`` and ``policy_flips`` equal
    (the order is total: larger value, fewer flips, lower end row, the empty set on a tie)."""
    import torch

    from gym_pbn_amd.multiflip import host_multiflip_max

    g, nodes, nbr, nbr_host = flip_case(name)
    S = g.n_states
    checked = 0
    for kind in ("random", "tied"):
        m_host = worths(S, kind)
        m = torch.from_numpy(m_host).to("cuda:0")
        for A in sorted({1, 2, 3, 4, min(len(nodes) + 1, 15)}):
            for cost, noop in ((1.0, None), (1.0, 0.0), (1.0, 2.0), (0.0, None), (0.0, 0.0), (0.5, 2.0)):
                v, end, flips = device_max(g, nbr, m, A, cost, noop)
                wv, wend, wflips = host_multiflip_max(m_host, nbr_host, nodes, A, cost, noop)
                got = v.cpu().numpy()
                assert np.array_equal(got.view(np.uint64), wv.view(np.uint64)), (kind, A, cost, noop)
                assert np.array_equal(end.cpu().numpy(), wend), (kind, A, cost, noop)
                assert np.array_equal(flips.cpu().numpy(), wflips), (kind, A, cost, noop)
                checked += 1
                if noop is None:
                    assert (wflips >= 1).all() and (wend != np.arange(S)).all()
        assert kind == "random" or np.unique(m_host).size <= 5  # ties were there to break
    assert checked == 2 * 6 * len({1, 2, 3, 4, min(len(nodes) + 1, 15)})


@pytest.mark.parametrize("name", sorted(NODES))
def test_one_free_flip_is_the_single_flip_backup(name):
    """``A = 1``, ``cost = 0``: the values equal ``pbn_stg_backup_device`` with ``u = -inf`` and ``ua = m``, bit for bit."""
    import torch

    from gym_pbn_amd import _lib

    g, nodes, nbr, _ = flip_case(name)
    S = g.n_states
    for kind in ("random", "tied"):
        m = torch.from_numpy(worths(S, kind, seed=3)).to("cuda:0")
        v, _, flips = device_max(g, nbr, m, 1, 0.0)
        u = torch.full((S,), -math.inf, dtype=torch.float64, device="cuda:0")
        want = torch.empty_like(m)
        policy = torch.empty(S, dtype=torch.int32, device="cuda:0")
        with g._on_default_stream(m.device):
            _lib.check(_lib.lib.pbn_stg_backup_device(g.handle, nbr.data_ptr(), u.data_ptr(), m.data_ptr(), want.data_ptr(),
                                                      policy.data_ptr()))
        assert same_bits(v, want) and bool((flips == 1).all()) and bool((policy >= 0).all())


@pytest.mark.parametrize("name", ["golden-N10", "embedded-65"])
def test_the_grid_and_the_call_do_not_show(name, monkeypatch):
    """Bit-identical from call to call, and under ``PBNSIM_STG_GRID=1`` (one workgroup walks every row: 16 trips of the
    four-row kernel, 256 of the looping one) against the default grid; summaries included."""
    import torch

    from gym_pbn_amd.transition import TransitionGraph

    g, nodes, nbr, _ = flip_case(name)
    m = torch.from_numpy(worths(g.n_states, "tied", seed=8)).to("cuda:0")
    want = device_max(g, nbr, m, 3, 1.0, 2.0)
    again = device_max(g, nbr, m, 3, 1.0, 2.0)
    assert all(torch.equal(a, b) for a, b in zip(want, again)) and same_bits(want[0], again[0])
    monkeypatch.setenv("PBNSIM_STG_GRID", "1")
    g1 = TransitionGraph(g.net, g.states, table_graph=g.table_graph)
    nbr1 = flip_rows(g1, nodes)
    assert torch.equal(nbr1, nbr)
    got = device_max(g1, nbr1, m, 3, 1.0, 2.0)
    assert same_bits(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    g1.close()


# ---------------------------------------------------------------- the problem
def problem(name, target, n_updates, **kw):
    from gym_pbn_amd.absorption import Absorption
    from gym_pbn_amd.multiflip import MultiFlipProblem

    d = device_case(name)
    kw.setdefault("max_flips", 2)
    return MultiFlipProblem(Absorption(d["graph"], d["label"]), target, n_updates=n_updates, nodes=NODES[name], **kw)


ARRIVAL = [("frozen-1", 0, 3), ("golden-N8", 1, 6), ("golden-N8", 0, 2), ("golden-N10", 1, 16), ("embedded-65", 0, 6)]


@pytest.mark.parametrize("name,target,n", ARRIVAL, ids=[f"{a}-t{b}-n{c}" for a, b, c in ARRIVAL])
def test_arrival_against_the_host_statement(name, target, n):
    """``arrival(v)`` within ``2 * arrival_bound`` of ``host_multiflip_arrival``: both are within the bound of the exact
    value of the same ``n - 2`` sweeps and expectations. ``flipset_max`` of it is the entry points' result."""
    import torch

    from gym_pbn_amd.multiflip import host_multiflip_arrival

    d = device_case(name)
    case = d["case"]
    S = len(d["label"])
    p = problem(name, target, n, gamma=0.9)
    assert p.n_updates == n and 0.0 <= p.inner_residual <= 1.0
    v = np.random.default_rng(2).uniform(-50.0, 50.0, size=S)
    got = p.arrival(torch.from_numpy(v).to("cuda:0"))
    want = host_multiflip_arrival(case["mass"], case["succ"], d["label"], case["n_movable"], target, v, n, 1000.0, 0.9)
    gmax = max(1000.0, 0.9 * np.abs(v).max())
    bound = 2 * arrival_bound(case["N"], n, gmax)
    dev = np.abs(got.cpu().numpy() - want).max()
    print(f"{name} target {target} n {n}: |M - host| {dev:.3e}, allowed {bound:.3e}, fraction {dev / bound:.4f}")
    assert dev <= bound
    assert same_bits(got, p.arrival(torch.from_numpy(v).to("cuda:0")))
    mx = p.flipset_max(got)
    ref = device_max(p.graph, p.nbr, got, 2, 1.0)
    assert same_bits(mx[0], ref[0]) and torch.equal(mx[1], ref[1]) and torch.equal(mx[2], ref[2])


def test_refusals_that_need_a_device():
    """Classes that are not closed under the dynamics (tt6's first-hit classes), an allowed flip that leaves the set
    (embedded-65 with every node allowed), and ``evaluate``'s checks."""
    import torch

    from gym_pbn_amd.absorption import Absorption
    from gym_pbn_amd.multiflip import MultiFlipProblem

    with pytest.raises(ValueError, match="not closed under the dynamics"):
        problem("tt6-step", 0, 4)
    d = device_case("embedded-65")
    with pytest.raises(ValueError, match="leave the state set"):
        MultiFlipProblem(Absorption(d["graph"], d["label"]), 0, max_flips=2, n_updates=4)
    p = problem("golden-N8", 1, 4)
    own = torch.arange(256, device="cuda:0")
    with pytest.raises(ValueError, match="empty set"):
        p.evaluate(own)
    with pytest.raises(ValueError, match="more than max_flips"):
        p.evaluate(own ^ 7)
    with pytest.raises(ValueError, match="outside"):
        p.evaluate(own + 1)
    d = device_case("golden-N8")
    q = MultiFlipProblem(Absorption(d["graph"], d["label"]), 1, max_flips=3, n_updates=4, nodes=[0, 1])
    with pytest.raises(ValueError, match="not allowed"):
        q.evaluate(own ^ 7)
    v, _, _ = q.evaluate(own ^ 3, max_iters=2)
    assert tuple(v.shape) == (256,)


def test_act_names_the_policys_nodes():
    """embedded-65 (``W = 2``, nodes 55 .. 64: bits of both words), one backup's policy: ``act`` gives ``node + 1``
    ascending, the first repeated; the decoded set is ``flip_words``; a state that is no row gets zeros, ``check=True``
    raises; ``width`` pads."""
    import torch

    p = problem("embedded-65", 1, 4, max_flips=3)
    sol = p.solve(max_iters=1)
    assert sol.iters == 1 and sol.n_updates == 4
    S = p.graph.n_states
    words = p.states.clone()
    rows = sol.act(words).cpu().numpy()
    F = sol.flip_words().cpu().numpy().view(np.uint64)
    flips = sol.policy_flips.cpu().numpy()
    assert rows.shape == (S, 3) and rows.dtype == np.int32 and flips.min() >= 1 and flips.max() <= 3
    print(f"rows by flip count: {np.bincount(flips).tolist()}")
    for s in range(0, S, 7):
        named = sorted(set(rows[s].tolist()))
        assert len(named) == flips[s] and rows[s, 0] == named[0] and list(rows[s, :flips[s]]) == named
        assert (rows[s, flips[s]:] == named[0]).all()
        want = [0, 0]
        for a in named:
            want[(a - 1) // 64] |= 1 << ((a - 1) % 64)
        assert [int(F[s, 0]), int(F[s, 1])] == want and all(55 <= a - 1 <= 64 for a in named)
    wide = sol.act(words[:5], width=5).cpu().numpy()
    assert wide.shape == (5, 5) and (wide[:, :3] == rows[:5]).all() and (wide[:, 3:] == rows[:5, :1]).all()
    stray = words[:3].clone()
    stray[1, 0] ^= 1  # a frozen node: no row of the set
    got = sol.act(stray).cpu().numpy()
    assert (got[1] == 0).all() and (got[[0, 2]] == rows[[0, 2]]).all()
    with pytest.raises(ValueError, match="no row"):
        sol.act(stray, check=True)
    with pytest.raises(ValueError, match="below max_flips"):
        sol.act(words, width=2)


# ---------------------------------------------------------------- value iteration
@pytest.mark.parametrize("k", [1.0, 300.0], ids=["cost1", "cost300"])
def test_solve_against_host_value_iteration(k):
    """Golden (8, 2, 6), ``A = 2``, ``n_updates = 8``, ``gamma = 0.9``, target class 1, ``solve(tol=1e-10)`` against value
    iteration with the host statements to the same ``tol``; at the env's ``action_cost = 1`` (two flips reach the target
    attractor from most rows: a short iteration) and at 300 (flips are dear: the policy weighs them against the
    dynamics, and the iteration runs its full length). Both stop within ``tol * gamma / (1 - gamma)`` of their own
    fixed point, and the two backups differ per application by at most ``eps = 2 * arrival_bound + 2 u (max|g| + k A)``
    (the max adds one rounded multiply and one rounded subtract; a max of values that differ by ``eps`` differs by at
    most ``eps``), which a contraction of modulus ``gamma`` amplifies to ``eps / (1 - gamma)``: allowed ``2 * tol / (1 -
    gamma) + eps / (1 - gamma)``. ``evaluate(policy_end)`` reproduces ``v`` and a host policy-improvement step from
    ``v`` changes no row's value by more than the same."""
    from gym_pbn_amd.multiflip import host_multiflip_arrival, host_multiflip_max

    tol, gamma, A, n, R, target = 1e-10, 0.9, 2, 8, 1000.0, 1
    d = device_case("golden-N8")
    case = d["case"]
    _, nodes, _, nbr_host = flip_case("golden-N8")
    p = problem("golden-N8", target, n, max_flips=A, gamma=gamma, action_cost=k)
    sol = p.solve(tol=tol)
    assert sol.residual <= tol and sol.n_updates == n and sol.iters < 400

    def host_backup(v):
        m = host_multiflip_arrival(case["mass"], case["succ"], d["label"], case["n_movable"], target, v, n, R, gamma)
        return host_multiflip_max(m, nbr_host, nodes, A, k)

    v = np.zeros(256)
    for it in range(1000):
        nxt, _, _ = host_backup(v)
        res = np.abs(nxt - v).max()
        v = nxt
        if res <= tol:
            break
    assert res <= tol
    gmax = max(R, k * A / (1 - gamma))  # |V| <= max(R, k A / (1 - gamma)): the bound on |g|
    eps = 2 * arrival_bound(case["N"], n, gmax) + 2 * U53 * (gmax + k * A)
    allowed = 2 * tol / (1 - gamma) + eps / (1 - gamma)
    got = sol.v.cpu().numpy()
    dev = np.abs(got - v).max()
    ev, ev_res, _ = p.evaluate(sol.policy_end, tol=tol)
    dev_eval = float((ev - sol.v).abs().max())
    improved, _, _ = host_backup(got)
    dev_imp = np.abs(improved - got).max()
    flips = sol.policy_flips.cpu().numpy()
    print(f"solve: {sol.iters} backups ({it + 1} on the host), residual {sol.residual:.2e}; |v - host| {dev:.3e}, "
          f"|evaluate - v| {dev_eval:.3e}, improvement step {dev_imp:.3e}, allowed {allowed:.3e}; v in [{got.min():.2f}, "
          f"{got.max():.2f}], flips {np.bincount(flips).tolist()}")
    assert dev <= allowed and ev_res <= tol and dev_eval <= allowed and dev_imp <= allowed
    assert flips.min() >= 1 and flips.max() <= 2 and got.max() <= R
    # the second case is there because the first is short (two flips reach the target from most rows): where flips
    # are dear some row's value is not a direct jump's R - k or R - 2 k: its policy leans on the dynamics
    assert got.min() > 0.0 if k == 1.0 else bool(((got != R - 2 * k) & (got != R - k)).any())


# ---------------------------------------------------------------- the closed loop
LOOP_SEED = 31


@pytest.mark.parametrize("k,anywhere", [(1, False), (300, True)], ids=["cost1-attractor0", "cost300-anywhere"])
def test_optimal_policy_in_the_env_earns_v_star(k, anywhere):
    """Golden (10, 2, 0), ``TorchVecPBNTargetMultiSetEnv`` over its two attractors, ``update_cap = 16``, 65,536 envs reset
    into attractor 0 with target 1, ``for_env(max_flips=2, n_updates=16, gamma=0.9)``, one seed. At the env's
    ``action_cost = 1`` two flips reach the target attractor from every state of attractor 0: every env ends in one step
    and the return has no spread. The second case makes the return a random variable: ``action_cost = 300``, so that
    the policy weighs a flip against what the dynamics do for nothing, and the envs are then set to states drawn
    uniformly from all ``2**10``, transient ones included. The envs follow ``sol.act`` until every env has terminated or ``T`` steps have passed, ``T`` the first with ``gamma**T * max|v| <
    1e-3``. The mean discounted return is held to the mean of ``sol.v`` over the start states within

        6 * sample_sd / sqrt(n)  +  gamma**T * max|v|  +  T * 16 * pmax * 2**-32 * span  +  2 * tol / (1 - gamma)

    -- the sampling error of a mean from the run's own deviation; what the steps past ``T`` could still add; §18's grid
    term (the Philox choice word has 32 bits: per update and threshold one grid step of probability, over 16 updates
    and ``T`` steps, times the span of a return, ``R + k A / (1 - gamma)``); and the solve's own distance from ``V*``.
    Every emitted row names 1 .. 2 distinct nodes and the env's reward is ``1000 * terminated - k * |F|``. Observed:
    ratio 0.000 (one step, return 999, no spread) and 0.149 (three steps, mean 651.27 against 651.71, sd 126.0)."""
    import torch

    from gym_pbn_amd.multiflip import MultiFlipProblem
    from gym_pbn_amd.torch_env import TorchVecPBNTargetMultiSetEnv

    n, cap, gamma, A, tol = 65536, 16, 0.9, 2, 1e-9
    c = case_by(10, 2, 0)
    net, atts = case_network(c), case_attractors(c)
    env = TorchVecPBNTargetMultiSetEnv(net, atts, n_envs=n, update_cap=cap, seed=LOOP_SEED, horizon=1 << 20, action_cost=k)
    p = MultiFlipProblem.for_env(env, gamma=gamma, max_flips=A, n_updates=cap)
    assert p.action_cost == float(k) and p.reward_success == 1000.0
    assert p.target == 1 and p.n_updates == cap and p.graph.n_states == 1024 and p.nodes == list(range(10))
    assert np.array_equal(p.absorption.labels_host, golden_case((10, 2, 0))["label"])
    sol = p.solve(tol=tol)
    assert sol.residual <= tol
    vmax = float(sol.v.abs().max())
    T = int(math.ceil(math.log(1e-3 / vmax) / math.log(gamma)))
    while gamma ** T * vmax >= 1e-3:
        T += 1
    env.reset(source=0, target=1)
    if anywhere:
        env.batch.set_state(np.random.default_rng(LOOP_SEED).integers(0, 1024, size=n).astype(np.uint64).reshape(-1, 1))
    start = p.graph.row_of(env.observation_words()).long()
    assert anywhere or bool((p.absorption.labels[start] == 0).all())
    want = float(sol.v[start].mean())
    ret = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    done = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    disc, steps = 1.0, 0
    for steps in range(1, T + 1):
        a = sol.act(env.observation_words())
        live = ~done
        first, second = a[:, 0], a[:, 1]
        assert bool(((first >= 1) & (first <= 10) & (second >= first) & (second <= 10))[live].all())
        n_f = 1 + (second != first).to(torch.int32)
        a = torch.where(live[:, None], a, torch.zeros_like(a))
        _, reward, term, _, _ = env.step(a)
        assert bool((reward == 1000 * term.to(torch.int32) - k * n_f)[live].all())
        ret += torch.where(live, disc * reward.to(torch.float64), torch.zeros_like(ret))
        done |= term
        disc *= gamma
        if bool(done.all()):
            break
    env.close()
    mean, sd = float(ret.mean()), float(ret.std())
    pmax = int(np.diff(net.pred_offsets).max())
    span = 1000.0 + k * A / (1 - gamma)
    band = 6 * sd / math.sqrt(n) + gamma ** T * vmax + T * cap * pmax * 2.0 ** -32 * span + 2 * tol / (1 - gamma)
    ratio = abs(mean - want) / band
    print(f"closed loop, cost {k}, {'any state' if anywhere else 'attractor 0'}: T {T}, {steps} steps made, {int(done.sum())} of {n} terminated; mean return {mean:.4f}, mean V* "
          f"{want:.4f}, sd {sd:.3f}, band {band:.4f}, ratio {ratio:.3f}; {sol.iters} backups")
    assert ratio <= 1.0 and mean > 0.0
