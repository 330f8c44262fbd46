#!/usr/bin/env python3
"""Absorption over a transition graph: what one sweep of all columns costs in one ``k_stg_absorb`` launch, in one
``k_stg_expect`` launch per column, and in torch ops. Measurement only; no threshold.

Workload: ``bench_control.py``'s set -- ``synthetic_truth_table_pbn(21, 3, seed=0)`` under ``table_graph="step"``, all
2**20 states with node 0 clear -- with three first-hit classes of 16 random rows each: K + 2 = 5 columns (class
probabilities, survival, time), and the same padded to 8 columns.

Legs, per column count C in (5, 8), all on the same ``mass`` / ``succ`` / labels and the same start:
  absorb  one ``k_stg_absorb`` launch over ``[S][C]`` (row-major): the graph is streamed once, labelled rows are held
          in the pass;
  expect  what the library could do before: per column one ``k_stg_expect`` launch on a contiguous ``[S]`` column, one
          ``torch.add`` of the source constant and one ``torch.where`` that holds the labelled rows (columns kept
          ``[C][S]``, the layout that suits it);
  pull    the torch formulation: ``TransitionGraph.pull`` per column (it recomputes ``probabilities()``), then the
          same add and where.
REPS rounds after a warm-up round; in each round every leg runs once (SWEEPS sweeps), in turn, so drift hits all legs
alike; device events and a wall clock around the run and a device synchronise; per-sweep time is the run's over SWEEPS;
median and spread (max - min). ``absorb`` and ``expect`` are checked once to agree within ``2 * sweep_bound`` per column
(``tests/test_absorb_host.py``) before any number is written. ``streamed_bytes`` = S * (12 N + 4 + 16 C): mass, succ,
labels, x read and out written once; ``gather_lines`` = S * N successor reads of C contiguous doubles (at most one
64-byte line for C = 8 when the row is line-aligned). One ``solve(tol=1e-12)`` is timed whole, capped at
``--max-updates`` sweeps; whether the tolerance was reached is part of the result. Results go to profiles/absorb.json.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))

REPS = 10
SWEEPS = 10
N_NODES = 21
N_CLASSES = 3
CLASS_ROWS = 16
COLUMN_COUNTS = (5, 8)
HBM_SPEC_BYTES_PER_S = 8e12
U53 = 2.0 ** -53


def summary(values):
    return {"runs": values, "median": statistics.median(values), "spread": max(values) - min(values)}


def time_legs(legs):
    """``{name: {"wall_s", "device_s"}}``: REPS rounds after a warm-up round, every leg once per round, in turn."""
    import torch

    for run in legs.values():
        run()
    wall = {k: [] for k in legs}
    dev = {k: [] for k in legs}
    for _ in range(REPS):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / SWEEPS)
            dev[name].append(e0.elapsed_time(e1) * 1e-3 / SWEEPS)
    return {k: {"wall_s": summary(wall[k]), "device_s": summary(dev[k])} for k in legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "absorb.json"))
    ap.add_argument("--nodes", type=int, default=N_NODES, help="network size (the default is the measured workload)")
    ap.add_argument("--max-updates", type=int, default=20000, help="sweeps the timed solve may make")
    args = ap.parse_args()
    import numpy as np
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.absorption import Absorption
    from gym_pbn_amd.network import TruthTableNetwork, synthetic_truth_table_pbn
    from gym_pbn_amd.transition import TransitionGraph

    assert _lib.device_count() >= 1, "bench_absorb.py measures on a GPU"
    N = args.nodes
    S = 1 << (N - 1)
    net = TruthTableNetwork.from_pbn_data(synthetic_truth_table_pbn(N, 3, 0))
    states = (np.arange(S, dtype=np.uint64) << np.uint64(1)).reshape(-1, 1)
    t0 = time.perf_counter()
    g = TransitionGraph(net, states, table_graph="step")
    assert g.closed
    labels = np.full(S, -1, dtype=np.int32)
    rows = np.random.default_rng(0).choice(S, size=N_CLASSES * CLASS_ROWS, replace=False)
    for k in range(N_CLASSES):
        labels[rows[k * CLASS_ROWS:(k + 1) * CLASS_ROWS]] = k
    ab = Absorption(g, labels)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    dev = ab.device
    held = ab.labels >= 0
    K = ab.n_classes

    def start(cols):
        """The standard five columns after three sweeps (no column is an indicator any more), padded with scaled
        copies; and the source constants."""
        a, _ = ab._start()
        x = a.clone()
        src = np.zeros(cols)
        src[K + 1] = 1.0
        for _ in range(3):
            x = ab.sweep(x, ab._src)
        if cols > K + 2:
            x = torch.cat([x, x[:, :cols - (K + 2)] * 0.5], dim=1).contiguous()
        return x, src

    result = {
        "workload": {"network": f"synthetic_truth_table_pbn({N}, 3, 0)", "table_graph": "step", "n_states": S,
                     "n_nodes": N, "classes": N_CLASSES, "rows_per_class": CLASS_ROWS, "setup_s": setup_s},
        "reps": REPS, "sweeps_per_rep": SWEEPS,
        "unit": "seconds per sweep of all columns: a run of sweeps_per_rep sweeps over sweeps_per_rep",
        "columns": {},
    }
    for cols in COLUMN_COUNTS:
        x0, src = start(cols)
        b_t = torch.from_numpy(src).to(dev)
        # agreement, once: absorb against expect per column
        got = ab.sweep(x0, src)
        tmp = torch.empty(S, dtype=torch.float64, device=dev)
        worst = 0.0
        for c in range(cols):
            xc = x0[:, c].contiguous()
            with g._on_default_stream(dev):
                g._expect_into(xc, tmp)
            want = torch.where(held, xc, tmp + b_t[c])
            bound = (2 * N + 8) * U53 * float(xc.abs().max()) + U53 * (float(xc.abs().max()) + abs(src[c]))
            d = float((got[:, c] - want).abs().max())
            assert d <= 2 * bound, (cols, c, d, bound)
            worst = max(worst, d / (2 * bound))

        a, b = x0.clone(), torch.empty_like(x0)
        ca = x0.t().contiguous()  # [C][S]: contiguous columns
        cb = torch.empty_like(ca)

        def absorb():
            nonlocal a, b
            with g._on_default_stream(dev):
                for _ in range(SWEEPS):
                    ab._launch(a, b, src)
                    a, b = b, a

        def expect():
            nonlocal ca, cb
            with g._on_default_stream(dev):
                for _ in range(SWEEPS):
                    for c in range(cols):
                        g._expect_into(ca[c], tmp)
                        if src[c]:
                            tmp.add_(src[c])
                        torch.where(held, ca[c], tmp, out=cb[c])
                    ca, cb = cb, ca

        def pull():
            nonlocal ca, cb
            for _ in range(SWEEPS):
                for c in range(cols):
                    e = g.pull(ca[c])
                    if src[c]:
                        e.add_(src[c])
                    torch.where(held, ca[c], e, out=cb[c])
                ca, cb = cb, ca

        t = time_legs({"absorb": absorb, "expect": expect, "pull": pull})
        streamed = S * (12 * N + 4 + 16 * cols)
        a_dev = t["absorb"]["device_s"]["median"]
        t.update({
            "agreement_absorb_vs_expect_over_allowed": worst,
            "absorb_over_expect_device": a_dev / t["expect"]["device_s"]["median"],
            "absorb_over_expect_wall": t["absorb"]["wall_s"]["median"] / t["expect"]["wall_s"]["median"],
            "absorb_over_pull_device": a_dev / t["pull"]["device_s"]["median"],
            "streamed_bytes_absorb": streamed,
            "streamed_bytes_expect": S * cols * (12 * N + 8 + 8 + 8 + 8 + 8 + 1),
            "gather_lines": S * N,
            "gather_bytes_used": S * N * 8 * cols,
            "absorb_streamed_bytes_per_s_device": streamed / a_dev,
            "absorb_share_of_hbm_spec": streamed / a_dev / HBM_SPEC_BYTES_PER_S,
        })
        result["columns"][str(cols)] = t
        del a, b, ca, cb, x0

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol = ab.solve(tol=1e-12, max_updates=args.max_updates)
    torch.cuda.synchronize()
    solve_s = time.perf_counter() - t0
    result["solve"] = {"tol": 1e-12, "max_updates": args.max_updates, "sweeps": sol.n_updates, "residual": sol.residual,
                       "reached_tol": sol.residual <= 1e-12, "seconds": solve_s,
                       "seconds_per_sweep": solve_s / max(sol.n_updates, 1),
                       "basin_weights": [float(v) for v in sol.basin_weights()],
                       "mean_unabsorbed": float(sol.unabsorbed.mean()), "max_time": float(sol.time.max())}
    print(json.dumps(result), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
