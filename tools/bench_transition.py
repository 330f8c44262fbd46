#!/usr/bin/env python3
"""The exact transition graph of two enumerated sets: what ``rows()`` costs, and the host path it replaces.
Measurement only; no threshold.

Four sets, each closed:
  bittner28_49152  the 49,152-state attractor of Bittner-28 from find_attractors (N = 28, W = 1);
  tt64_cube20      a 2**20-state closure of a truth-table network made here: 64 nodes, nodes 0 .. 19 with three inputs
                   among themselves and table entries inside (0, 1), nodes 20 .. 63 copying themselves (frozen), graph
                   "stg": everything a state reaches is the cube over the 20 free nodes;
  tt24_cube20, tt128_cube20  the same 20 free nodes among 24 and 128: the same 2**20 x 20 probing cells beside 4 and
                   108 frozen nodes' cells, which make no probe -- what the probes cost and what a cell costs (W = 2 at 128).
Per set:
  rows        TransitionGraph.rows() over the whole set, outputs allocated by torch's caching allocator, wall clock
              around the call and a device synchronise, and device events around the same call; REPS runs after a
              warm-up, median and spread (max - min). bytes = S * N * 12 (the uint64 mass and the int32 succ written);
              the states and the table probes read are not counted.
  host        what a user had without the kernel: host_edge_mass over the rows, the neighbour of every cell with
              mass > 0 formed in numpy, and a host StateSet.lookup of those neighbours; each part timed, HOST_RUNS runs.
The device result is compared with the host result (mass bit for bit, succ where the host looked up) before any number
is written. Results go to profiles/transition.json.
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
HOST_RUNS = 2
FREE = 20
CUBE_NODES = (24, 64, 128)


def cube_network(n_nodes=64, free=FREE, seed=0):
    import numpy as np

    from gym_pbn_amd.network import TruthTableNetwork

    rng = np.random.default_rng(seed)
    data = []
    for i in range(n_nodes):
        mask = np.zeros(n_nodes, dtype=bool)
        if i < free:
            mask[np.sort(rng.choice([j for j in range(free) if j != i], size=3, replace=False))] = True
            tt = 0.05 + 0.9 * rng.random((2, 2, 2))
        else:
            mask[i] = True
            tt = np.array([0.0, 1.0])
        data.append((mask, tt, f"G{i}", False))
    return TruthTableNetwork.from_pbn_data(data, name=f"tt{n_nodes}_cube{free}")


def cube_states(free, frozen_bits):
    """The 2**free states over the free nodes 0 .. free - 1 (free <= 64), the other nodes at frozen_bits: [S][W]."""
    import numpy as np

    n_nodes = free + len(frozen_bits)
    base = sum(int(b) << (free + k) for k, b in enumerate(frozen_bits))
    words = [np.arange(1 << free, dtype=np.uint64) | np.uint64(base & (2 ** 64 - 1))]
    for k in range(1, (n_nodes + 63) // 64):
        words.append(np.full(1 << free, (base >> (64 * k)) & (2 ** 64 - 1), dtype=np.uint64))
    return np.stack(words, axis=1)


def summary(values):
    return {"runs": values, "median": statistics.median(values), "spread": max(values) - min(values)}


def host_path(net, states, graph):
    """(mass, (cell rows, cell nodes, labels), seconds per part) of the host path."""
    import numpy as np

    from gym_pbn_amd.stateset import StateSet
    from gym_pbn_amd.transition import host_edge_mass

    t0 = time.perf_counter()
    mass = host_edge_mass(net, states, graph)
    t1 = time.perf_counter()
    s_idx, i_idx = np.nonzero(mass)
    neigh = states[s_idx].copy()
    neigh[np.arange(len(s_idx)), i_idx // 64] ^= np.uint64(1) << (i_idx % 64).astype(np.uint64)
    t2 = time.perf_counter()
    table = StateSet(states, net.n_nodes, labels=np.arange(len(states), dtype=np.int32), device=None)
    t3 = time.perf_counter()
    labels = table.lookup(neigh)
    t4 = time.perf_counter()
    table.close()
    return mass, (s_idx, i_idx, labels), {"host_edge_mass": t1 - t0, "neighbours_numpy": t2 - t1,
                                          "stateset_build": t3 - t2, "stateset_lookup": t4 - t3, "total": t4 - t0}


def measure(name, net, states, graph):
    import numpy as np
    import torch

    from gym_pbn_amd.transition import TransitionGraph

    S, N = len(states), net.n_nodes
    g = TransitionGraph(net, states, table_graph=graph)
    mass, succ = g.rows()  # warm-up: code object, allocator
    torch.cuda.synchronize()
    host_runs = []
    for _ in range(HOST_RUNS):
        h_mass, (s_idx, i_idx, labels), secs = host_path(g.net, states, graph)
        host_runs.append(secs)
    m, t = mass.cpu().numpy(), succ.cpu().numpy()
    assert np.array_equal(m.astype(np.uint64), h_mass), "device mass differs from host_edge_mass"
    assert np.array_equal(t[s_idx, i_idx], labels), "device succ differs from the host lookup"
    assert np.array_equal(t[m == 0], np.nonzero(m == 0)[0].astype(np.int32)), "succ of a cell without mass is not its row"
    leaks = g.leaks
    del mass, succ, m, t
    wall, dev = [], []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = g.rows()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1) * 1e-3)
        del out
    g.close()
    row_bytes = S * N * 12
    r = {"set": name, "n_states": S, "n_nodes": N, "n_words": net.n_words, "table_graph": graph, "leaks": leaks,
         "cells_with_mass": int(len(s_idx)), "row_bytes": row_bytes,
         "rows_wall_s": summary(wall), "rows_device_s": summary(dev),
         "row_bytes_per_s_wall": row_bytes / statistics.median(wall),
         "row_bytes_per_s_device": row_bytes / statistics.median(dev),
         "host_s": {k: summary([x[k] for x in host_runs]) for k in host_runs[0]},
         "host_over_rows_wall": statistics.median([x["total"] for x in host_runs]) / statistics.median(wall)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "transition.json"))
    args = ap.parse_args()
    import numpy as np

    from gym_pbn_amd import _lib
    from gym_pbn_amd.attractors import find_attractors
    from gym_pbn_amd.network import load_network

    assert _lib.device_count() >= 1, "bench_transition.py measures on a GPU"
    result = {"reps": REPS, "host_runs": HOST_RUNS,
              "unit": "seconds per rows() call over the whole set; row_bytes = n_states * n_nodes * 12 written",
              "sets": []}
    res = find_attractors("bittner28", n_seeds=256, max_states=1 << 17, seed=1)
    big = [a for a in res.attractors if len(a) == 49152]
    assert big, f"the 49,152-state attractor was not reached: sizes {[len(a) for a in res.attractors]}"
    result["sets"].append(measure("bittner28_49152", load_network("bittner28"), big[0], None))
    for n_nodes in CUBE_NODES:
        net = cube_network(n_nodes)
        frozen = np.random.default_rng(1).integers(0, 2, size=n_nodes - FREE)
        result["sets"].append(measure(f"tt{n_nodes}_cube{FREE}", net, cube_states(FREE, frozen), "stg"))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
