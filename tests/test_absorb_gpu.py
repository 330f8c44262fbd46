"""Absorption over a transition graph on the device (``csrc/pbn_absorb.hip``; ``gym_pbn_amd.absorption``).

One sweep is held to the numpy statement (``host_absorb_sweep``) and to exact ``Fraction`` arithmetic within the bounds
derived in ``test_absorb_host.py``; the three bit-identity promises (call to call, any grid, any column chunking) and
the equality with ``k_stg_expect`` are held bit for bit; the horizon law is held to host sweeps and to a dense solve;
and the closed loop holds the env kernel's labels, caps and update counts to ``env_step_law``.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from test_absorb_host import (absorption_by_solve, as_fractions, exact_sweep, golden_case, max_deviation, summed_bound,
                              sweep_bound, tt6_case)
from test_attractors_host import all_states, case_attractors, case_network
from test_transition_host import case_by

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


# ---------------------------------------------------------------- the cases
def _n8():
    c = golden_case((8, 2, 6))
    return c["net"], c["states"], None, c["label"]


def _tt6():
    c = tt6_case()
    return c["net"], c["states"], "step", c["label"]


def _embedded_65():
    """N10-p2-s0 at places 55..64 of 65 nodes (W = 2, two cells per lane: the looping kernel); row r is the small
    network's state r, so the golden labels carry over."""
    from test_control_gpu import _embedded

    net, states, graph = _embedded(65)
    return net, states, graph, golden_case((10, 2, 0))["label"]


def _frozen_1():
    """One node that copies itself (G = 1, no shuffle): nothing moves; state 1 is class 0, state 0 is transient."""
    from test_control_gpu import _frozen_1 as frozen

    net, states, graph = frozen()
    return net, states, graph, np.array([-1, 0], dtype=np.int32)


def _golden(key):
    c = golden_case(key)
    return c["net"], c["states"], None, c["label"]


CASES = {"golden-N8": _n8, "tt6-step": _tt6, "embedded-65": _embedded_65, "frozen-1": _frozen_1,
         "golden-N10": lambda: _golden((10, 2, 0)), "golden-N12": lambda: _golden((12, 3, 1))}


@functools.lru_cache(maxsize=None)
def device_case(name):
    """``dict(graph, label (numpy), label_t (device int32), case)``: ``case`` is the host dict ``exact_sweep`` and
    ``host_absorb_sweep`` take, with the integer arrays read back from the device (pinned bit for bit by
    ``test_transition_gpu.py``)."""
    import torch

    from gym_pbn_amd.transition import TransitionGraph

    net, states, graph, label = CASES[name]()
    g = TransitionGraph(net, np.ascontiguousarray(states, dtype=np.uint64), table_graph=graph)
    assert g.closed
    case = dict(mass=g.mass.cpu().numpy().astype(np.uint64), succ=g.succ.cpu().numpy(), label=label,
                n_movable=g.n_movable, N=g.n_nodes)
    return dict(graph=g, label=label, label_t=torch.from_numpy(label.astype(np.int32)).to("cuda:0"), case=case)


def launch(g, label_t, x, out, n_cols, src):
    """``pbn_stg_absorb_device`` on device tensors ``[S][ld]``, ``src`` a sequence or None."""
    from gym_pbn_amd import _lib

    b = None if src is None else (C.c_double * len(src))(*[float(v) for v in src])
    with g._on_default_stream(x.device):
        _lib.check(_lib.lib.pbn_stg_absorb_device(g.handle, g.mass.data_ptr(), g.succ.data_ptr(), label_t.data_ptr(),
                                                  x.data_ptr(), out.data_ptr(), n_cols, x.shape[1], b))


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@functools.lru_cache(maxsize=None)
def eight_columns(name):
    """``(x [S][8], src [8], host [S][8], exact)``: random signed columns of different scales, non-zero sources, and
    both references of one sweep, computed once."""
    from gym_pbn_amd.absorption import host_absorb_sweep

    case = device_case(name)["case"]
    S = len(case["label"])
    rng = np.random.default_rng(29)
    x = rng.uniform(-1.0, 1.0, size=(S, 8)) * np.array([1.0, 3.0, 0.25, 1e3, 1.0, 7.0, 1e-3, 2.0])
    src = np.array([0.5, -1.0, 0.0, 2.5, 1.0, -0.125, 1e-3, 3.0])
    host = host_absorb_sweep(case["mass"], case["succ"], case["label"], case["n_movable"], x, src)
    return x, src, host, exact_sweep(case, as_fractions(x), src)


# ---------------------------------------------------------------- one sweep
@pytest.mark.parametrize("n_cols", range(1, 9))
@pytest.mark.parametrize("name", ["golden-N8", "tt6-step", "embedded-65", "frozen-1"])
def test_one_sweep_against_host_and_exact_arithmetic(name, n_cols):
    """Columns ``[0, n_cols)`` within ``2 * sweep_bound`` of ``host_absorb_sweep`` and within ``sweep_bound`` of the exact
    value; labelled rows bit-equal to their input; with ``ld = n_cols + 2`` the two spare columns of ``out`` keep their
    sentinel."""
    import torch

    d = device_case(name)
    g, label, N = d["graph"], d["label"], d["case"]["N"]
    x, src, host, exact = eight_columns(name)
    S = len(label)
    xin = np.concatenate([x[:, :n_cols], np.random.default_rng(n_cols).normal(size=(S, 2))], axis=1)
    xt = torch.from_numpy(np.ascontiguousarray(xin)).to("cuda:0")
    out = torch.full_like(xt, SENTINEL)
    launch(g, d["label_t"], xt, out, n_cols, src[:n_cols])
    got = out.cpu().numpy()
    assert (got[:, n_cols:] == SENTINEL).all()
    held = label >= 0
    assert held.any() and np.array_equal(got[held, :n_cols].view(np.uint64), xin[held, :n_cols].view(np.uint64))
    bounds = np.array([sweep_bound(N, np.abs(x[:, c]).max(), src[c]) for c in range(n_cols)])
    dev_host = np.abs(got[:, :n_cols] - host[:, :n_cols]).max(axis=0)
    dev_exact = np.array(max_deviation(got[:, :n_cols], exact[:n_cols]))
    print(f"{name} n_cols {n_cols}: largest deviation / bound: host {(dev_host / (2 * bounds)).max():.3f}, "
          f"exact {(dev_exact / bounds).max():.3f}")
    assert (dev_host <= 2 * bounds).all() and (dev_exact <= bounds).all()
    assert name == "frozen-1" or (got[~held, :n_cols] != xin[~held, :n_cols]).any()


@pytest.mark.parametrize("name", ["embedded-65", "golden-N8"])
def test_a_column_does_not_depend_on_its_launch(name):
    """Column ``c`` of the 8-column launch is bit-identical to the ``n_cols = 1`` launch of that column, for every ``c``;
    so are the columns of an 11-column :meth:`Absorption.sweep` (two launches, 8 + 3) and of the tiles in between."""
    import torch

    from gym_pbn_amd.absorption import Absorption

    d = device_case(name)
    x, src, _, _ = eight_columns(name)
    ab = Absorption(d["graph"], d["label"])
    xt = torch.from_numpy(x).to("cuda:0")
    eight = ab.sweep(xt, src)
    assert same_bits(eight, ab.sweep(xt, src))
    alone = [ab.sweep(xt[:, c].contiguous(), src[c:c + 1]) for c in range(8)]
    for c in range(8):
        assert alone[c].shape == (len(d["label"]),) and same_bits(eight[:, c], alone[c]), c
    for lo, hi in ((0, 2), (1, 4), (2, 7), (3, 8)):  # tiles 2, 4, 8 and the 5-column launch
        part = ab.sweep(xt[:, lo:hi].contiguous(), src[lo:hi])
        assert same_bits(part, eight[:, lo:hi]), (lo, hi)
    wide = torch.cat([xt, xt[:, :3] * 0.5], dim=1)
    wsrc = np.concatenate([src, src[:3]])
    got = ab.sweep(wide, wsrc)
    assert same_bits(got[:, :8], eight)
    for c in range(3):
        assert same_bits(got[:, 8 + c], ab.sweep((xt[:, c] * 0.5).contiguous(), src[c:c + 1])), c


def test_the_grid_does_not_show(monkeypatch):
    """Golden (12, 3, 1), 4,096 rows, ``PBNSIM_STG_GRID=3`` set before the graph is created (every group walks the
    grid-stride loop): bit-identical to the uncapped result, for every column tile, from call to call, and under a
    torch stream of the caller's."""
    import torch

    from gym_pbn_amd.absorption import Absorption
    from gym_pbn_amd.transition import TransitionGraph

    d = device_case("golden-N12")
    S = len(d["label"])
    x = torch.from_numpy(np.random.default_rng(3).normal(size=(S, 8)) * 10.0).to("cuda:0")
    src = np.arange(8) * 0.25 - 1.0
    ab = Absorption(d["graph"], d["label"])
    want = {n: ab.sweep(x[:, :n].contiguous(), src[:n]) for n in (1, 2, 3, 5, 8)}
    ten = ab.within(10)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = ab.within(10)
        swept = ab.sweep(x, src)
    side.synchronize()
    assert same_bits(again.prob, ten.prob) and same_bits(again.time, ten.time) and same_bits(swept, want[8])
    monkeypatch.setenv("PBNSIM_STG_GRID", "3")
    net, states, graph, _ = CASES["golden-N12"]()
    g3 = TransitionGraph(net, states, table_graph=graph)
    ab3 = Absorption(g3, d["label"])
    for n, w in want.items():
        got = ab3.sweep(x[:, :n].contiguous(), src[:n])
        assert same_bits(got, w) and same_bits(got, ab3.sweep(x[:, :n].contiguous(), src[:n])), n
    t3 = ab3.within(10)
    assert same_bits(t3.prob, ten.prob) and same_bits(t3.unabsorbed, ten.unabsorbed) and same_bits(t3.time, ten.time)


@pytest.mark.parametrize("name", ["golden-N8", "embedded-65", "golden-N12", "frozen-1"])
def test_without_labels_one_column_is_expect(name):
    """``label`` all -1, ``n_cols = 1``, ``src`` NULL: ``graph.expect(v)`` bit for bit, on the one-cell and the looping
    kernel."""
    import torch

    d = device_case(name)
    g = d["graph"]
    S = g.n_states
    v = torch.from_numpy(np.random.default_rng(4).normal(size=S) * 1e3).to("cuda:0")
    none = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    out = torch.full((S, 1), SENTINEL, dtype=torch.float64, device="cuda:0")
    launch(g, none, v.reshape(S, 1), out, 1, None)
    assert same_bits(out.reshape(S), g.expect(v))


# ---------------------------------------------------------------- the horizon law
def test_within_64_against_host_sweeps():
    """N10-p2-s0, 64 sweeps: every column within the summed bound of 64 host sweeps; ``sum_k prob + unabsorbed = 1``
    within ``K + 1`` times it."""
    from gym_pbn_amd.absorption import Absorption, AbsorptionResult, host_absorb_within

    d = device_case("golden-N10")
    case = d["case"]
    N, K = case["N"], 2
    r = Absorption(d["graph"], d["label"]).within(64)
    assert isinstance(r, AbsorptionResult) and r.n_updates == 64 and tuple(r.prob.shape) == (1024, K)
    h = host_absorb_within(case["mass"], case["succ"], case["label"], case["n_movable"], n_updates=64)
    b_p, b_t = summed_bound(N, 64), summed_bound(N, 64, b=1.0, x0max=0.0)
    prob, un, time = r.prob.cpu().numpy(), r.unabsorbed.cpu().numpy(), r.time.cpu().numpy()
    d_p, d_u, d_t = np.abs(prob - h["prob"]).max(), np.abs(un - h["unabsorbed"]).max(), np.abs(time - h["time"]).max()
    print(f"within(64): prob {d_p:.3e}, unabsorbed {d_u:.3e} (bound {b_p:.3e}), time {d_t:.3e} (bound {b_t:.3e}); "
          f"residual {r.residual:.3e}")
    assert d_p <= b_p and d_u <= b_p and d_t <= b_t
    assert np.abs(r.unabsorbed_1.cpu().numpy() - h["unabsorbed_1"]).max() <= summed_bound(N, 1)
    assert np.abs(prob.sum(axis=1) + un - 1.0).max() <= (K + 1) * b_p
    assert r.residual == un.max() and 0.0 < r.residual < 1.0
    held = d["label"] >= 0
    assert (un[held] == 0.0).all() and (time[held] == 0.0).all() and (prob[held].sum(axis=1) == 1.0).all()
    zero = Absorption(d["graph"], d["label"]).within(0)
    assert zero.n_updates == 0 and zero.unabsorbed_1 is None and (zero.unabsorbed.cpu().numpy() == ~held).all()


def test_solve_against_a_dense_solve():
    """N12-p3-s1: ``solve()`` stops at ``residual <= 1e-12`` within ``check_every`` of the 2,048 sweeps the float64
    restatement needs; ``prob`` against ``numpy.linalg.solve`` within ``residual + summed bound + 1e-11`` (the dense
    solve's own error); ``basin_weights()`` against the mean of that solution; ``at`` names rows by state words."""
    import torch

    from gym_pbn_amd.absorption import Absorption

    d = device_case("golden-N12")
    N = d["case"]["N"]
    ab = Absorption.from_attractors(d["graph"], case_attractors(case_by(12, 3, 1)))
    assert np.array_equal(ab.labels_host, d["label"]) and ab.n_classes == 2
    r = ab.solve()
    assert r.residual <= 1e-12 and abs(r.n_updates - 2048) <= 16 and r.n_updates % 16 == 0
    B = absorption_by_solve((12, 3, 1))
    band = r.residual + summed_bound(N, r.n_updates) + 1e-11
    dev = np.abs(r.prob.cpu().numpy() - B).max()
    w = r.basin_weights().cpu().numpy()
    print(f"solve: {r.n_updates} sweeps, residual {r.residual:.3e}, |prob - solve| {dev:.3e} (band {band:.3e}); basin "
          f"weights {w.tolist()}, max time {float(r.time.max()):.2f}")
    assert dev <= band
    assert np.abs(w - B.mean(axis=0)).max() <= band and abs(w.sum() - 1.0) <= 3 * band
    wts = np.random.default_rng(6).uniform(size=4096)
    assert np.abs(r.basin_weights(wts).cpu().numpy() - wts @ B).max() <= band * wts.sum()
    words = torch.tensor([[5], [4095], [77]], dtype=torch.int64, device="cuda:0")
    p, u, t = r.at(words)
    assert same_bits(p, r.prob[[5, 4095, 77]]) and same_bits(u, r.unabsorbed[[5, 4095, 77]]) and same_bits(t, r.time[[5, 4095, 77]])
    with pytest.raises(ValueError, match="no row"):
        r.at(torch.tensor([[1 << 12]], dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError, match="no row of the graph"):
        Absorption.from_attractors(d["graph"], [np.array([[1 << 12]], dtype=np.uint64)])
    with pytest.raises(ValueError, match="n_updates >= 2"):
        ab.within(1).env_step_law(words)
    # the other accepted forms name the same labels
    from gym_pbn_amd.attractors import AttractorResult
    from gym_pbn_amd.stateset import StateSet

    atts = case_attractors(case_by(12, 3, 1))
    res = AttractorResult(n_nodes=12, attractors=atts)
    assert np.array_equal(Absorption.from_attractors(d["graph"], res).labels_host, d["label"])
    sset = StateSet(np.concatenate(atts), 12, labels=np.concatenate([np.full(len(a), k) for k, a in enumerate(atts)]),
                    device=None)
    assert np.array_equal(Absorption.from_attractors(d["graph"], sset).labels_host, d["label"])
    tuples = [[tuple(int(v >> i) & 1 for i in range(12)) for v in a[:, 0]] for a in atts]
    assert np.array_equal(Absorption.from_attractors(d["graph"], tuples).labels_host, d["label"])


def test_refusals_that_need_a_device():
    """A graph that is not closed -- the lower half of golden (8, 2, 6)'s states: node 7 leaves it -- is refused by
    ``Absorption`` and by ``from_attractors`` (the kernel would read every leaked edge as "stays"); and the
    ``ValueError``s of ``from_attractors``: a state set of another network size, a member that is no row, an attractor
    that shares a state with an earlier one."""
    from gym_pbn_amd.absorption import Absorption
    from gym_pbn_amd.stateset import StateSet
    from gym_pbn_amd.transition import TransitionGraph

    c = golden_case((8, 2, 6))
    half = TransitionGraph(c["net"], all_states(8)[:128])
    assert not half.closed and half.leaks > 0
    lab = np.full(128, -1, dtype=np.int32)
    lab[[3, 77]] = 0
    with pytest.raises(ValueError, match="needs a closed set"):
        Absorption(half, lab)
    with pytest.raises(ValueError, match="needs a closed set"):
        Absorption.from_attractors(half, [all_states(8)[[3, 77]]])
    with pytest.raises(ValueError, match="needs a closed set"):
        Absorption.from_attractors(half, StateSet(all_states(8)[[3, 77]], 8, device=None))
    # judged before the graph: the members
    with pytest.raises(ValueError, match="1 member state\\(s\\) are no row of the graph"):
        Absorption.from_attractors(half, StateSet(all_states(8)[[5, 200]], 8, labels=[0, 1], device=None))
    with pytest.raises(ValueError, match="a state set of 9 nodes for a graph of 8"):
        Absorption.from_attractors(half, StateSet(all_states(8)[[5]], 9, device=None))
    with pytest.raises(ValueError, match="1 state\\(s\\) of attractor 1 are no row of the graph"):
        Absorption.from_attractors(half, [all_states(8)[[5]], all_states(8)[[6, 200]]])
    full = device_case("golden-N8")["graph"]
    atts = case_attractors(case_by(8, 2, 6))
    with pytest.raises(ValueError, match="attractor 1 shares a state with an earlier one"):
        Absorption.from_attractors(full, [atts[0], atts[0][:1]])
    half.close()


# ---------------------------------------------------------------- the closed loop
LOOP_SEED = 20


def test_env_step_matches_its_exact_law():
    """N10-p2-s0, ``TorchVecPBNTargetMultiSetEnv`` over the two golden attractors, ``update_cap = 16``, 65,536 envs: eight
    transient states ``t`` whose class-0 probability at horizon 16 lies in [0.2, 0.8] (chosen on the host), 8,192 envs
    each at ``t ^ bit(0)`` with the action ``[1]`` (flip node 0), so the state after the flip is ``t``. Per state the
    counts of ``label == 0``, ``label == 1`` and ``capped`` lie within ``6 sqrt(n p (1 - p)) + 1 + n * 16 * pmax * 2**-32``
    of ``n p`` (the last term: the 32-bit grid of the Philox choice word, one grid step per threshold, over 16
    updates) with ``p`` from ``env_step_law``, and the mean of ``n_updates`` within ``6 * 16 / sqrt(n)`` of
    ``mean_updates`` (``n_updates`` lies in [1, 16]: its standard deviation is below 16)."""
    import torch

    from gym_pbn_amd.absorption import Absorption, host_absorb_within
    from gym_pbn_amd.torch_env import TorchVecPBNTargetMultiSetEnv

    cap, n, n_states = 16, 8192, 8
    d = device_case("golden-N10")
    case = d["case"]
    net = case_network(case_by(10, 2, 0))
    atts = case_attractors(case_by(10, 2, 0))
    h = host_absorb_within(case["mass"], case["succ"], case["label"], case["n_movable"], n_updates=cap)
    ok = np.flatnonzero((d["label"] < 0) & (h["prob"][:, 0] >= 0.2) & (h["prob"][:, 0] <= 0.8))
    assert len(ok) >= n_states, "fewer than 8 states qualify"
    t = ok[:: len(ok) // n_states][:n_states].astype(np.uint64)
    env = TorchVecPBNTargetMultiSetEnv(net, atts, n_envs=n * n_states, update_cap=cap, seed=LOOP_SEED)
    env.batch.set_state(np.repeat(t ^ np.uint64(1), n).reshape(-1, 1))
    actions = torch.ones((n * n_states, 1), dtype=torch.int64, device="cuda:0")
    _, _, _, _, info = env.step(actions)
    label = info["label"].cpu().numpy().reshape(n_states, n)
    capped = info["capped"].cpu().numpy().reshape(n_states, n).astype(bool)
    nup = info["n_updates"].cpu().numpy().reshape(n_states, n)
    env.close()
    law = Absorption(d["graph"], d["label"]).within(cap)
    words = torch.from_numpy(t.astype(np.int64).reshape(-1, 1)).to("cuda:0")
    lp, cp, mu = (v.cpu().numpy() for v in law.env_step_law(words))
    assert np.abs(lp - h["prob"][t.astype(np.int64)]).max() <= summed_bound(10, cap)
    pmax = int(np.diff(net.pred_offsets).max())
    grid = n * cap * pmax * 2.0 ** -32
    worst = 0.0
    for s in range(n_states):
        assert ((label[s] == -1) == capped[s]).all() and nup[s].min() >= 1 and nup[s].max() <= cap
        for count, p in ((int((label[s] == 0).sum()), lp[s, 0]), (int((label[s] == 1).sum()), lp[s, 1]),
                         (int(capped[s].sum()), cp[s])):
            band = 6.0 * np.sqrt(n * p * (1.0 - p)) + 1.0 + grid
            worst = max(worst, abs(count - n * p) / band)
            assert abs(count - n * p) <= band, (s, count, n * p, band)
        band = 6.0 * cap / np.sqrt(n)
        worst = max(worst, abs(nup[s].mean() - mu[s]) / band)
        assert abs(nup[s].mean() - mu[s]) <= band, (s, nup[s].mean(), mu[s])
    print(f"closed loop: {len(ok)} states qualify; class-0 probabilities {np.round(lp[:, 0], 3).tolist()}, capped "
          f"{np.round(cp, 3).tolist()}, mean updates {np.round(mu, 2).tolist()}; largest fraction of a band {worst:.3f}")
    assert 0.0 < worst <= 1.0 and (cp > 0.01).any()
