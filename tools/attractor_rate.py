#!/usr/bin/env python3
"""Rate of on-device attractor discovery (gym_pbn_amd.attractors) next to a numpy restatement.

For each network: ``find_attractors`` end to end (seeds, burn-in, closures, backward marking), then
one closure from a settled state on the device set and the same closure by a numpy breadth-first
search on this host. States expanded per second = states of the closure / wall time. The numpy
search stops once it has seen ``--numpy-limit`` states (its rate is then over the states it
expanded), so a 2^21-state closure does not take minutes of host time.

    python tools/attractor_rate.py [--networks bittner28 bittner70 bittner100] [--n-seeds 256]

Networks under ``--large`` (Bittner-149, -199: closures that do not fit) only get the ``find_attractors``
report: how many states each closure had seen when it stopped and how many nodes vary among them.
Truth-table networks (``--tables``, support graph ``--table-graph``): a bundled name such as ``tt200``, or
``n,k,det,seed`` for a random network (every node ``k`` inputs, table entries 0.0 / 1.0 with probability
``det`` each, else uniform). They get the ``find_attractors`` report and the closure rate from one seed; a
closure that stops at ``--table-max-states`` still gives a rate (states seen per second).
Prints one JSON line per network.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))

TWO53 = 1 << 53


def random_table_network(n, k, det, seed):
    from gym_pbn_amd.network import TruthTableNetwork

    rng = np.random.default_rng(seed)
    data = []
    for i in range(n):
        inp = np.sort(rng.choice([j for j in range(n) if j != i], size=k, replace=False))
        u, v = rng.random(1 << k), rng.random(1 << k)
        mask = np.zeros(n, dtype=bool)
        mask[inp] = True
        data.append((mask, np.where(u < det, 0.0, np.where(u < 2 * det, 1.0, v)).reshape((2,) * k), f"n{i}", False))
    return TruthTableNetwork.from_pbn_data(data, name=f"random-{n}-{k}-{det}-{seed}")


def np_table_unstable(net, bits, graph):
    """Node i can flip iff its table entry p has p > 0 (from 0) or p < 1 (from 1); "step" freezes node 0."""
    bits = np.asarray(bits, dtype=np.int64)
    out = np.zeros(bits.shape, dtype=bool)
    for i in range(1 if graph == "step" else 0, net.n_nodes):
        code = np.zeros(len(bits), dtype=np.int64)
        for j in net.inputs[int(net.input_offsets[i]):int(net.input_offsets[i + 1])]:
            code = 2 * code + bits[:, int(j)]
        p = net.probs[int(net.thr_offsets[i]):int(net.thr_offsets[i + 1])][code]
        out[:, i] = ((p > 0.0) & (bits[:, i] == 0)) | ((p < 1.0) & (bits[:, i] == 1))
    return out


def np_unstable(net, bits, graph=None):
    """Node i can flip at a state iff a live predictor (non-empty 53-bit interval) outputs 1 - x_i."""
    if graph is not None:
        return np_table_unstable(net, bits, graph)
    bits = np.asarray(bits, dtype=np.int64)
    out = np.zeros(bits.shape, dtype=bool)
    for i in range(net.n_nodes):
        o0, o1 = int(net.pred_offsets[i]), int(net.pred_offsets[i + 1])
        prev, xi = 0, bits[:, i]
        for j in range(o0, o1):
            t = min(int(net.pred_thr[j]), TWO53) if j < o1 - 1 else TWO53
            live, prev = t > prev, max(prev, t)
            if not live:
                continue
            a, b, c = (int(v) for v in net.pred_inputs[j])
            p = (bits[:, a] << 3) | (bits[:, b] << 2) | (bits[:, c] << 1) | xi
            out[:, i] |= ((int(net.pred_tt[j]) >> p) & 1) != xi
    return out


def np_closure(net, seed, limit, graph=None):
    """Breadth-first closure; returns (states seen, states expanded)."""
    from gym_pbn_amd.attractors import rows_in
    from gym_pbn_amd.batch import unpack_bits

    seen = np.asarray(seed, np.uint64).reshape(1, -1)
    frontier, expanded = seen, 0
    while len(frontier) and len(seen) < limit:
        s_idx, i_idx = np.nonzero(np_unstable(net, unpack_bits(frontier, net.n_nodes), graph))
        succ = frontier[s_idx].copy()
        succ[np.arange(len(s_idx)), i_idx // 64] ^= np.uint64(1) << (i_idx % 64).astype(np.uint64)
        expanded += len(frontier)
        succ = np.unique(succ, axis=0)
        frontier = succ[~rows_in(succ, seen)]
        seen = np.concatenate([seen, frontier])
    return len(seen), expanded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--networks", nargs="+", default=["bittner28", "bittner70", "bittner100"])
    ap.add_argument("--large", nargs="*", default=["bittner149", "bittner199"])
    ap.add_argument("--large-seeds", type=int, default=16)
    ap.add_argument("--large-max-states", type=int, default=1 << 20)
    ap.add_argument("--n-seeds", type=int, default=256)
    ap.add_argument("--max-states", type=int, default=1 << 22)
    ap.add_argument("--numpy-limit", type=int, default=1 << 18)
    ap.add_argument("--tables", nargs="*", default=["tt200", "40,3,0.40,7"])
    ap.add_argument("--table-graph", choices=["stg", "step"], default="stg")
    ap.add_argument("--table-seeds", type=int, default=64)
    ap.add_argument("--table-max-states", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    from gym_pbn_amd.attractors import ReachSet, find_attractors, rows_in
    from gym_pbn_amd.network import load_network

    ReachSet("bittner28", 64, a.device).closure(np.zeros((1, 1), np.uint64))  # runtime and code object warm
    jobs = [(name, load_network(name), None, a.n_seeds, a.max_states) for name in a.networks]
    for name in a.tables:
        net = random_table_network(*(float(v) if "." in v else int(v) for v in name.split(","))) if "," in name \
            else load_network(name)
        jobs.append((net.name, net, a.table_graph, a.table_seeds, a.table_max_states))
    for name, net, graph, n_seeds, max_states in jobs:
        t0 = time.perf_counter()
        res = find_attractors(net, n_seeds=n_seeds, max_states=max_states, device=a.device, table_graph=graph or "stg")
        t_find = time.perf_counter() - t0
        out = {"network": name, "table_graph": graph, "n_seeds": n_seeds, "max_states": max_states,
               "attractor_sizes": [len(x) for x in res.attractors], "seed_counts": res.seed_counts,
               "attractors_disjoint": not any(rows_in(x[:1], y)[0] for k, x in enumerate(res.attractors)
                                              for y in res.attractors[k + 1:]),
               "incomplete": [{"n_seen": e["n_seen"], "n_seeds": e["n_seeds"], "free_nodes": e["hull"].count("*")}
                              for e in res.incomplete],
               "find_attractors_s": round(t_find, 4)}
        seed = res.attractors[-1][:1] if res.attractors else res.incomplete[0]["seed"][None]
        rs = ReachSet(net, max_states, a.device, table_graph=graph)
        t0 = time.perf_counter()
        n, complete = rs.closure(seed)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        n_back = rs.mark_backward(seed)
        t_back = time.perf_counter() - t0
        info = rs.info()
        out.update(closure_states=n, closure_complete=complete, closure_s=round(t_dev, 5),
                   device_states_per_s=round(n / t_dev), backward_marked=n_back, backward_s=round(t_back, 5),
                   dead_entries=int(info["n_entries"] - info["n_states"]))
        t0 = time.perf_counter()
        seen, expanded = np_closure(net, seed, a.numpy_limit, graph)
        t_np = time.perf_counter() - t0
        out.update(numpy_states_seen=seen, numpy_states_expanded=expanded, numpy_s=round(t_np, 3),
                   numpy_states_per_s=round(expanded / t_np), numpy_stopped_early=bool(seen < n))
        print(json.dumps(out), flush=True)
    for name in a.large:
        t0 = time.perf_counter()
        res = find_attractors(name, n_seeds=a.large_seeds, max_states=a.large_max_states, device=a.device)
        print(json.dumps({"network": name, "n_seeds": a.large_seeds, "max_states": a.large_max_states,
                          "attractor_sizes": [len(x) for x in res.attractors], "seed_counts": res.seed_counts,
                          "incomplete": [{"n_seen": e["n_seen"], "n_seeds": e["n_seeds"],
                                          "free_nodes": e["hull"].count("*")} for e in res.incomplete],
                          "find_attractors_s": round(time.perf_counter() - t0, 4)}), flush=True)


if __name__ == "__main__":
    main()
