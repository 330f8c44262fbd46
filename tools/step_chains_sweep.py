#!/usr/bin/env python3
"""Step mode's launch chains: host wall time and HIP-event region per step, by chain count and launch form.

For every (network, batch) case and every (chains, graph) setting a fresh batch is created with
PBNSIM_STEP_CHAINS / PBNSIM_STEP_GRAPH set (the knobs are read at batch creation), warmed up, and
``step(K)`` is measured ``--reps`` times two ways: host wall clock around step(K) + device sync (what
bench.py's headline takes), and the timing-mode-2 event region on the batch's stream (start ahead of the
fork, stop behind the join). Where wall per step exceeds the region per step, the host does not keep up
with the launches. Prints one JSON object; ``--out`` also writes it.

A library without the knob (the parent commit's, selected with PBNSIM_LIB) ignores PBNSIM_STEP_CHAINS:
run it with ``--chains 1`` for the baseline rows.

Usage: step_chains_sweep.py [--cases bittner199:1048576,...] [--chains 1,2,4] [--graph d,0,1] [--steps K]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))


def measure(net, B, steps, warmup, reps):
    import torch

    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch(net, B, seed=0x5EED)
    info = b.info()
    b.randomize()
    b.step(warmup)
    b.prepare_steps(steps)
    b.sync()
    wall, region = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.step(steps)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6 / steps)
    for _ in range(reps):
        torch.cuda.synchronize()
        b.timing(2)
        b.step(steps)
        b.timing(0)
        ms, launches = b.timing_read()
        assert launches == steps, (launches, steps)
        region.append(ms * 1e3 / steps)
    b.close()
    return {"step_chains": info.get("step_chains"), "wall_us_per_step": wall, "region_us_per_step": region,
            "wall_us_median": statistics.median(wall), "region_us_median": statistics.median(region)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="bittner199:1048576,bittner199:2097152,bittner199:8388608,bittner28:65536")
    p.add_argument("--chains", default="1,2,4")
    p.add_argument("--graph", default="d,0,1", help="d = the default by size, 0 = plain launches, 1 = graphs")
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from gym_pbn_amd import _lib
    from gym_pbn_amd.network import load_network

    rows = []
    for case in a.cases.split(","):
        name, B = case.split(":")
        net = load_network(name)
        for chains in a.chains.split(","):
            for graph in a.graph.split(","):
                os.environ["PBNSIM_STEP_CHAINS"] = chains
                if graph == "d":
                    os.environ.pop("PBNSIM_STEP_GRAPH", None)
                else:
                    os.environ["PBNSIM_STEP_GRAPH"] = graph
                row = {"network": name, "n_envs": int(B), "chains_knob": int(chains), "graph_knob": graph,
                       "steps": a.steps, "warmup": a.warmup, **measure(net, int(B), a.steps, a.warmup, a.reps)}
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"library": str(_lib.LIB_PATH), "rows": rows}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
