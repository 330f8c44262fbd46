#!/usr/bin/env python3
"""State census at 1,048,576 envs, 64 updates, every state counted: what the table costs. Measurement only.

Per network (TT-200, Bittner-28) and start -- "settled": randomize + rollout(BURN_IN); "fair": randomize alone, every
bit a coin flip, so nearly every env sits on a state of its own -- wall time of one call (state and update counter put
back before each, one sync after it):
  census_cold   pbn_census_run_device(64, first 0, stride 1) into a cleared table: every distinct state is inserted;
  census_warm   the same call again without a clear: the same trajectories, so every key is found, none inserted;
  rollout       pbn_rollout(64) on the same batch: the floor -- the same updates with no table.
And once per network and start (the first round only: the sort takes most of a minute), what a user had to do before
the census existed:
  host_loop     64 x (step(1) + get_state()), the batch over PCIe once per sample, plus get_state() of the start;
  host_unique   np.unique(axis=0, return_counts=True) over the 65 x B rows.
Three rounds; a round is one child process per network that runs the legs in turn, so the legs alternate, and every
child runs under its own time limit. Medians and spreads (max - min over the rounds) go to profiles/census.json with
the ratio census / rollout, the distinct states, the dropped visits and the count adds issued per sample point (one
minus the share of sample points that only extended a lane's pending run).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))

B = 1 << 20
N_UPDATES = 64
BURN_IN = 16384
ROUNDS = 3
REPS = 5
CHILD_LIMIT_S = 600
NETWORKS = ("tt200", "bittner28")
STARTS = ("settled", "fair")
LEGS = ("census_cold", "census_warm", "rollout")


def child(network: str, n_envs: int, host_leg: bool) -> dict:
    import numpy as np
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.census import StateCensus

    b = PBNBatch(network, n_envs, seed=7)
    c = StateCensus(b.net, max_states=_lib.CENSUS_MAX_STATES)
    saved = torch.empty((n_envs, b.n_words), dtype=torch.int64, device="cuda:0")
    out = {"network": network, "n_envs": n_envs}

    def restore(u0):
        b.set_state_device(saved.data_ptr())
        b.seek(update_count=u0)
        b.sync()

    def timed(fn, u0, before=None):
        runs = []
        for _ in range(REPS + 1):  # the first run is a warm-up
            restore(u0)
            if before:
                before()
            t0 = time.perf_counter()
            fn()
            b.sync()
            runs.append(time.perf_counter() - t0)
        return statistics.median(runs[1:])

    for start in STARTS:
        b.randomize()
        if start == "settled":
            b.rollout(BURN_IN)
        b.get_state_device(saved.data_ptr())
        b.sync()
        u0 = b.counters()["update_count"]
        r = {}
        r["census_cold"] = timed(lambda: c.run(b, N_UPDATES), u0, before=c.clear)
        info, adds = c.info(), c.adds()  # of the last cold run alone
        r["distinct_states"] = info["n_states"]
        r["dropped"] = info["dropped"]
        r["visits"] = info["visits"]
        r["adds_per_sample_point"] = adds / info["visits"]
        r["census_warm"] = timed(lambda: c.run(b, N_UPDATES), u0)
        r["rollout"] = timed(lambda: b.rollout(N_UPDATES), u0)
        print(f"{network} {start}: {r}", file=sys.stderr, flush=True)
        if host_leg:
            restore(u0)
            t0 = time.perf_counter()
            rows = [b.get_state()]
            for _ in range(N_UPDATES):
                b.step(1)
                rows.append(b.get_state())
            t1 = time.perf_counter()
            print(f"{network}: host loop {t1 - t0:.3f} s; np.unique over {len(rows) * n_envs} rows ...", file=sys.stderr,
                  flush=True)
            uniq, _ = np.unique(np.concatenate(rows), axis=0, return_counts=True)
            t2 = time.perf_counter()
            r["host_loop"], r["host_unique"], r["host_distinct_states"] = t1 - t0, t2 - t1, int(len(uniq))
            del rows, uniq
        out[start] = r
    c.close()
    b.close()
    return out


def summary(values):
    return {"runs": values, "median": statistics.median(values), "spread": max(values) - min(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="", help="run one round of this network and print its JSON line")
    ap.add_argument("--envs", type=int, default=B)
    ap.add_argument("--host-leg", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "census.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.envs, bool(args.host_leg))))
        return 0
    result = {"n_envs": args.envs, "n_updates": N_UPDATES, "first": 0, "stride": 1, "burn_in": BURN_IN, "rounds": ROUNDS,
              "reps_per_round": REPS, "unit": "seconds per call over the whole batch, wall clock", "networks": []}
    for network in NETWORKS:
        rounds = []
        for r in range(ROUNDS):
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, __file__, "--child", network,
                   "--envs", str(args.envs), "--host-leg", str(int(r == 0))]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"round {r} of {network} ended with status {p.returncode}; stopping", file=sys.stderr)
                return p.returncode
            rounds.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(rounds[-1]), flush=True)
        entry = {"network": network}
        for start in STARTS:
            legs = {k: summary([x[start][k] for x in rounds]) for k in LEGS}
            first = rounds[0][start]
            entry[start] = {
                **legs,
                "census_cold_over_rollout": legs["census_cold"]["median"] / legs["rollout"]["median"],
                "census_warm_over_rollout": legs["census_warm"]["median"] / legs["rollout"]["median"],
                "distinct_states": first["distinct_states"], "dropped": first["dropped"], "visits": first["visits"],
                "adds_per_sample_point": first["adds_per_sample_point"],
            }
            if "host_loop" in first:
                host = first["host_loop"] + first["host_unique"]
                entry[start].update({"host_loop": first["host_loop"], "host_unique": first["host_unique"],
                                     "host_distinct_states": first["host_distinct_states"], "host_runs": 1,
                                     "host_over_census_cold": host / legs["census_cold"]["median"]})
        result["networks"].append(entry)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
