#!/usr/bin/env python3
"""The max over multi-flip action sets: what one full max (A levels and the select) costs in the ``k_stg_flipset``
kernels, in the same top-two recursion written in torch ops, and in plain enumeration in torch. Measurement only; no
threshold.

Workload: ``bench_control.py``'s set -- ``synthetic_truth_table_pbn(21, 3, seed=0)`` under ``table_graph="step"``, all
2**20 states with node 0 clear -- with the 20 movable nodes allowed (the set is closed under their flips) and ``A = 3``:
20 + 190 + 1,140 = 1,350 sets per row against 20 * 3 gathers of a pair.

Legs, all on the same ``nbr`` and the same random worths ``m``, cost 1:
  kernel     ``A`` launches of ``k_stg_flipset`` and one of ``k_stg_flipset_select``;
  recursion  the same recursion in torch ops: per level and node one gather of the neighbour's pair and two inserts
             written with ``torch.where``, under the same order;
  enumerate  every set by gathers through composed ``nbr`` (``itertools.combinations``), a running best under the same
             order.
The three are checked once to give the same ``v`` bit for bit and the same policy before any number is written. REPS
rounds after a warm-up round; in each round every leg runs once, in turn, so drift hits all legs alike; device events
and a wall clock around the run and a device synchronise; median and spread (max - min). ``streamed_bytes`` of the kernel
leg = A * S * (4 N + 24 + 24) + S * (24 + 8 + 16): per level nbr and the row's own pair read and the pair written, the
select's reads and writes; ``gather_bytes`` = A * S * 20 * 24 (level 0 -> 1 gathers 8 bytes, not 24).

Then one whole backup of the MDP is split into its inner sweeps (``n - 2`` of ``k_stg_absorb``, three of
``k_stg_expect``) and its max, and ``solve`` is timed whole, at ``n_updates = 16`` and ``gamma = 0.9``. The classes are
the attractors ``find_attractors`` reaches under ``"step"``; where that gives no proper labelling (none found, or the
whole set is one attractor) there is no MDP to solve: the reason is recorded, ``solve`` is left out, and the split is
timed launch for launch with ``bench_absorb.py``'s first-hit classes instead. Results go to profiles/multiflip.json.
"""
import argparse
import itertools
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))

REPS = 10
N_NODES = 21
MAX_FLIPS = 3
N_UPDATES = 16
D_SHIFT = 24


def summary(values):
    return {"runs": values, "median": statistics.median(values), "spread": max(values) - min(values)}


def time_legs(legs, reps=REPS):
    """``{name: {"wall_s", "device_s"}}``: ``reps`` rounds after a warm-up round, every leg once per round, in turn."""
    import torch

    for run in legs.values():
        run()
    wall = {k: [] for k in legs}
    dev = {k: [] for k in legs}
    for _ in range(reps):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
            dev[name].append(e0.elapsed_time(e1) * 1e-3)
    return {k: {"wall_s": summary(wall[k]), "device_s": summary(dev[k])} for k in legs}


# ---------------------------------------------------------------- the recursion in torch ops
def t_value(base, tag, k):
    return base - k * (tag >> D_SHIFT).to(base.dtype)


def t_better(ab, at, bb, bt, k):
    va, vb = t_value(ab, at, k), t_value(bb, bt, k)
    return (at >= 0) & ((bt < 0) | (va > vb) | ((va == vb) & (at < bt)))


def t_insert(p, eb, et, k):
    """pbn_flipset_rule.hpp's flip_insert on tensors: ``p = (b0, t0, b1, t1)``."""
    import torch

    b0, t0, b1, t1 = p
    mask = (1 << D_SHIFT) - 1
    same0 = (et >= 0) & (t0 >= 0) & ((et & mask) == (t0 & mask))
    w0, w1 = t_better(eb, et, b0, t0, k), t_better(eb, et, b1, t1, k)
    nb0, nt0 = torch.where(w0, eb, b0), torch.where(w0, et, t0)
    sb = torch.where(w0, b0, torch.where(w1, eb, b1))
    st = torch.where(w0, t0, torch.where(w1, et, t1))
    return nb0, nt0, torch.where(same0, b1, sb), torch.where(same0, t1, st)


def torch_recursion(nbr_cols, m, A, k):
    import torch

    S = m.shape[0]
    own = torch.arange(S, dtype=torch.int32, device=m.device)
    none_b, none_t = torch.zeros_like(m), torch.full_like(own, -1)
    cur = (m, own, none_b, none_t)
    for _ in range(A):
        nxt = cur
        for col in nbr_cols:
            for eb, et in ((cur[0][col], cur[1][col]), (cur[2][col], cur[3][col])):
                et = torch.where(et >= 0, et + (1 << D_SHIFT), et)
                nxt = t_insert(nxt, eb, et, k)
        cur = nxt
    b0, t0, b1, t1 = cur
    first_is_s = (t0 & ((1 << D_SHIFT) - 1)) == own
    eb, et = torch.where(first_is_s, b1, b0), torch.where(first_is_s, t1, t0)
    return t_value(eb, et, k), et & ((1 << D_SHIFT) - 1), et >> D_SHIFT


def torch_enumeration(nbr_cols, m, A, k):
    import torch

    S = m.shape[0]
    v = torch.full_like(m, -float("inf"))
    end = torch.full((S,), -1, dtype=torch.int64, device=m.device)
    flips = torch.zeros(S, dtype=torch.int64, device=m.device)
    for d in range(1, A + 1):
        c = k * float(d)
        for F in itertools.combinations(range(len(nbr_cols)), d):
            y = nbr_cols[F[0]]
            for i in F[1:]:
                y = nbr_cols[i][y]
            q = m[y] - c
            better = (q > v) | ((q == v) & (flips == d) & (y < end))
            v, end = torch.where(better, q, v), torch.where(better, y, end)
            flips = torch.where(better, torch.full_like(flips, d), flips)
    return v, end, flips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multiflip.json"))
    ap.add_argument("--nodes", type=int, default=N_NODES, help="network size (the default is the measured workload)")
    ap.add_argument("--max-flips", type=int, default=MAX_FLIPS)
    args = ap.parse_args()
    import numpy as np
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.absorption import Absorption
    from gym_pbn_amd.attractors import find_attractors
    from gym_pbn_amd.multiflip import MultiFlipProblem
    from gym_pbn_amd.network import TruthTableNetwork, synthetic_truth_table_pbn
    from gym_pbn_amd.transition import TransitionGraph

    assert _lib.device_count() >= 1, "bench_multiflip.py measures on a GPU"
    N, A, k = args.nodes, args.max_flips, 1.0
    S = 1 << (N - 1)
    network = TruthTableNetwork.from_pbn_data(synthetic_truth_table_pbn(N, 3, 0))
    states = (np.arange(S, dtype=np.uint64) << np.uint64(1)).reshape(-1, 1)
    g = TransitionGraph(network, states, table_graph="step")
    assert g.closed
    dev = torch.device("cuda", 0)
    nodes = list(range(1, N))
    mask = np.array([sum(1 << i for i in nodes)], dtype=np.uint64)
    nbr = torch.empty((S, N), dtype=torch.int32, device=dev)
    with g._on_default_stream(dev):
        _lib.check(_lib.lib.pbn_stg_flip_rows_device(g.handle, 0, S, _lib.ptr(mask, _lib._u64p), nbr.data_ptr()))
    assert bool((nbr[:, 1:] >= 0).all()) and bool((nbr[:, 0] == -1).all())
    nbr_cols = [nbr[:, i].long().contiguous() for i in nodes]
    m = torch.from_numpy(np.random.default_rng(0).uniform(-1000.0, 1000.0, size=S)).to(dev)
    n_sets = sum(len(list(itertools.combinations(nodes, d))) for d in range(1, A + 1))

    base = [torch.empty((S, 2), dtype=torch.float64, device=dev) for _ in range(2)]
    tag = [torch.empty((S, 2), dtype=torch.int32, device=dev) for _ in range(2)]
    out_v = torch.empty(S, dtype=torch.float64, device=dev)
    out_end, out_flips = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(2))

    def kernel():
        with g._on_default_stream(dev):
            src = None
            for lev in range(A):
                _lib.check(_lib.lib.pbn_stg_flipset_level_device(
                    g.handle, nbr.data_ptr(), m.data_ptr(), k, None if src is None else src[0].data_ptr(),
                    None if src is None else src[1].data_ptr(), base[lev & 1].data_ptr(), tag[lev & 1].data_ptr()))
                src = (base[lev & 1], tag[lev & 1])
            _lib.check(_lib.lib.pbn_stg_flipset_select_device(g.handle, src[0].data_ptr(), src[1].data_ptr(), m.data_ptr(),
                                                              k, None, out_v.data_ptr(), out_end.data_ptr(),
                                                              out_flips.data_ptr()))

    # agreement, once, before any number is written
    kernel()
    rv, rend, rflips = torch_recursion(nbr_cols, m, A, k)
    ev, eend, eflips = torch_enumeration(nbr_cols, m, A, k)
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))  # noqa: E731
    assert same(out_v, rv) and same(out_v, ev), "the three legs disagree on v"
    assert torch.equal(out_end.long(), rend.long()) and torch.equal(out_end.long(), eend)
    assert torch.equal(out_flips.long(), rflips.long()) and torch.equal(out_flips.long(), eflips)
    del rv, rend, rflips, ev, eend, eflips

    t = time_legs({"kernel": kernel, "recursion": lambda: torch_recursion(nbr_cols, m, A, k),
                   "enumerate": lambda: torch_enumeration(nbr_cols, m, A, k)})
    streamed = A * S * (4 * N + 24 + 24) + S * (24 + 8 + 16)
    k_dev = t["kernel"]["device_s"]["median"]
    result = {
        "workload": {"network": f"synthetic_truth_table_pbn({N}, 3, 0)", "table_graph": "step", "n_states": S,
                     "n_nodes": N, "allowed_nodes": len(nodes), "max_flips": A, "sets_per_row": n_sets,
                     "pair_gathers_per_row": len(nodes) * A, "cost": k},
        "reps": REPS, "unit": "seconds per full max: A levels and the select",
        "agreement": "v bit-equal and policy equal across the three legs",
        "max": t,
        "kernel_over_recursion_device": k_dev / t["recursion"]["device_s"]["median"],
        "kernel_over_enumerate_device": k_dev / t["enumerate"]["device_s"]["median"],
        "kernel_over_recursion_wall": t["kernel"]["wall_s"]["median"] / t["recursion"]["wall_s"]["median"],
        "streamed_bytes_kernel": streamed, "gather_bytes_kernel": A * S * len(nodes) * 24,
        "kernel_streamed_bytes_per_s_device": streamed / k_dev,
    }

    # one whole backup, split; and solve
    res = find_attractors(network, n_seeds=1024, table_graph="step", max_states=1 << 21)
    sizes = [int(len(a)) for a in res.attractors]
    result["attractors"] = {"sizes": sizes[:16], "count": len(sizes), "incomplete": len(res.incomplete)}
    if len(sizes) < 1 or sum(sizes) >= S:
        # no MDP to solve here; a backup's launches are still the same launches: time them with bench_absorb.py's
        # first-hit classes (three times 16 random rows), one column, the same n
        result["solve"] = None
        result["solve_left_out"] = "no proper labelling: " + ("no attractor found" if not sizes else "the set is one attractor")
        labels = np.full(S, -1, dtype=np.int32)
        rows = np.random.default_rng(0).choice(S, size=48, replace=False)
        for c in range(3):
            labels[rows[c * 16:(c + 1) * 16]] = c
        ab = Absorption(g, labels)
        za = torch.from_numpy(np.random.default_rng(1).uniform(0.0, 1000.0, size=(S, 1))).to(dev)
        zb, e1, e2 = torch.empty_like(za), torch.empty(S, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev)

        def sweeps():
            a, b = za, zb
            with g._on_default_stream(dev):
                for _ in range(N_UPDATES - 2):
                    ab._launch(a, b, (0.0,))
                    a, b = b, a
                g._expect_into(m, e1)
                g._expect_into(a.reshape(-1), e2)
                g._expect_into(e2, e1)

        b = time_legs({"inner_sweeps": sweeps, "max": kernel})
        s_dev, m_dev = b["inner_sweeps"]["device_s"]["median"], b["max"]["device_s"]["median"]
        b["max_share_of_backup_device"] = m_dev / (s_dev + m_dev)
        b["n_updates"] = N_UPDATES
        b["classes"] = "first-hit classes, 3 x 16 random rows: the launches of a backup, not an MDP"
        result["backup"] = b
    else:
        ab = Absorption.from_attractors(g, res.attractors)
        p = MultiFlipProblem(ab, len(sizes) - 1, max_flips=A, n_updates=N_UPDATES, gamma=0.9, nodes=nodes)
        v = torch.from_numpy(np.random.default_rng(1).uniform(0.0, 1000.0, size=S)).to(dev)
        end, flips = p._policy_buffers()
        nxt = torch.empty_like(v)

        def sweeps():
            with g._on_default_stream(dev):
                p._arrival_into(v, p._m)

        def the_max():
            with g._on_default_stream(dev):
                p._max_into(p._m, nxt, end, flips)

        b = time_legs({"inner_sweeps": sweeps, "max": the_max})
        s_dev, m_dev = b["inner_sweeps"]["device_s"]["median"], b["max"]["device_s"]["median"]
        b["max_share_of_backup_device"] = m_dev / (s_dev + m_dev)
        b["n_updates"] = N_UPDATES
        result["backup"] = b
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = p.solve(tol=1e-9)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        result["solve"] = {"tol": 1e-9, "gamma": 0.9, "n_updates": N_UPDATES, "backups": sol.iters, "residual": sol.residual,
                           "inner_residual": sol.inner_residual, "seconds": secs, "seconds_per_backup": secs / max(sol.iters, 1),
                           "mean_v": float(sol.v.mean()), "rows_by_flips": torch.bincount(sol.policy_flips.long()).tolist()}
    print(json.dumps(result), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
