#!/usr/bin/env python3
"""Per-step period and chain overlap of the step kernel from a rocprofv3 kernel trace.

Takes the last --steps launches of the step kernel on every queue that ran it (one queue per launch chain)
and prints one JSON object: per queue the launch count, mean kernel duration and mean start-to-start
period; ``period_us`` = the mean over queues (the time from one step's kernel start to the next step's on
the same chain); ``overlap_frac`` = the share of the window during which two or more step kernels were in
flight (0 for one chain: launches of one queue never overlap).

Usage: chain_trace.py <kernel_trace.csv> [--kernel SUBSTR] [--steps N]
"""
import argparse
import csv
import json
from collections import defaultdict


def main():
    p = argparse.ArgumentParser()
    p.add_argument("trace")
    p.add_argument("--kernel", default="k_step<4, 1, 1, 0, 1024>")
    p.add_argument("--steps", type=int, default=200)
    a = p.parse_args()
    by_queue = defaultdict(list)
    for r in csv.DictReader(open(a.trace)):
        if a.kernel in r["Kernel_Name"]:
            by_queue[r.get("Queue_Id", "0")].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    queues, spans = {}, []
    for q, rows in by_queue.items():
        rows.sort()
        rows = rows[-a.steps:]
        if len(rows) < 2:
            continue
        spans += rows
        queues[q] = {"launches": len(rows), "mean_kernel_us": sum(e - s for s, e in rows) / len(rows) / 1e3,
                     "period_us": (rows[-1][0] - rows[0][0]) / (len(rows) - 1) / 1e3}
    # time with >= 2 kernels in flight over the window from the first start to the last end
    edges = sorted([(s, 1) for s, _ in spans] + [(e, -1) for _, e in spans])
    depth, last, busy2, busy1 = 0, None, 0, 0
    for t, d in edges:
        if last is not None:
            busy2 += (t - last) if depth >= 2 else 0
            busy1 += (t - last) if depth >= 1 else 0
        depth += d
        last = t
    window = (edges[-1][0] - edges[0][0]) if edges else 0
    print(json.dumps({"kernel": a.kernel, "queues": queues,
                      "period_us": sum(q["period_us"] for q in queues.values()) / max(len(queues), 1),
                      "window_us": window / 1e3, "overlap_frac": busy2 / window if window else 0.0,
                      "busy_frac": busy1 / window if window else 0.0}, indent=1))


if __name__ == "__main__":
    main()
