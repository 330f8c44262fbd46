#!/usr/bin/env python3
"""Until-attractor env step: the cube kernel k_env against the state-set kernel k_env_set. Measurement only.

Bittner-28 with the attractors ``find_attractors`` returns, 131,072 envs, the bench's ``env_actions`` (A = 4), update
cap 4,096, one launch per env step; wall time per env step (all launches queued, then one sync):
  (a) k_env over ``EnvConfig(net, res.all_attractors())``: the path the library offered before k_env_set;
  (b) k_env_set over ``res.state_set()``;
  (c) (b) without the hull pre-filter (PBNSIM_ENVSET_NO_HULL=1);
  (d) (b) without the unchanged-state skip (PBNSIM_ENVSET_NO_SKIP=1).
Also (a) and (b) on TT-200 with a state-list attractor set of TT200_STATES states: three attractors of 1, 15 and 240
states, the states envs reach after a burn-in (k_env gets their cube cover, which has to fit its LDS image).
Every leg starts from the same batch seed and state and steps the same action rows, so every leg computes the same
trajectory (the kernels are bit-exact against each other: tests/test_env_set_gpu.py). Five rounds; a round is one
child process that runs the legs in turn, so the legs alternate, and every child runs under its own time limit.
Medians and spreads (max - min over the rounds) go to profiles/env_set.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))

N_ENVS = 131072
CAP = 4096
A = 4
ROUNDS = 5
CHILD_LIMIT_S = 300
TT200_SIZES = (1, 15, 240)  # k_env keeps its cubes in LDS next to the 28.8 KiB image: a few hundred at most
TT200_STATES = sum(TT200_SIZES)
LEGS = {"a_k_env_cubes": {}, "b_k_env_set": {}, "c_no_hull": {"PBNSIM_ENVSET_NO_HULL": "1"},
        "d_no_skip": {"PBNSIM_ENVSET_NO_SKIP": "1"}}


def child(network: str, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch

    from gym_pbn_amd.actions import env_actions
    from gym_pbn_amd.attractors import AttractorResult, find_attractors
    from gym_pbn_amd.batch import EnvConfig, Net, PBNBatch

    net = Net(network)
    N, W = net.n_nodes, net.n_words
    dev = torch.device("cuda", 0)
    if network == "bittner28":
        res = find_attractors(network, n_seeds=4096)
        legs = list(LEGS)
    else:  # attractors as state lists: what envs hold after a burn-in, split into three attractors
        b = PBNBatch(net, 4 * TT200_STATES, seed=3)
        b.randomize()
        b.rollout(200 * N)
        rows = np.unique(b.get_state(), axis=0)[:TT200_STATES]
        b.close()
        assert len(rows) == TT200_STATES
        cuts = np.cumsum((0,) + TT200_SIZES)
        res = AttractorResult(N, attractors=[rows[cuts[k]:cuts[k + 1]] for k in range(3)])
        legs = ["a_k_env_cubes", "b_k_env_set"]
    cubes = res.all_attractors()
    cfg = EnvConfig(net, cubes)
    sset = res.state_set()
    K = len(res.attractors)
    acts = env_actions(warmup + steps, 0, N_ENVS, A, N, seed=0xAC7, device=dev)
    obs = torch.empty((N_ENVS, W), dtype=torch.int64, device=dev)
    rew = torch.empty(N_ENVS, dtype=torch.int32, device=dev)
    flags = torch.empty(N_ENVS, dtype=torch.uint8, device=dev)
    nup = torch.empty(N_ENVS, dtype=torch.int32, device=dev)
    lab = torch.empty(N_ENVS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out = {"network": network, "n_attractors": K, "n_states": len(sset), "n_cubes": sum(len(c) for c in cubes)}
    sums = {}
    for leg in legs:
        for k in ("PBNSIM_ENVSET_NO_HULL", "PBNSIM_ENVSET_NO_SKIP"):
            os.environ.pop(k, None)
        os.environ.update(LEGS[leg])  # read when the batch is created
        b = PBNBatch(net, N_ENVS, seed=7)
        b.env_reset_device(cfg)  # every leg: the cube reset, so the same start

        def step(t):
            a = acts[t]
            if leg == "a_k_env_cubes":
                b.env_step_multi_device(cfg, a.data_ptr(), A, obs.data_ptr(), rew.data_ptr(), flags.data_ptr(),
                                        nup.data_ptr(), update_cap=CAP)
            else:
                b.env_set_step_device(sset, a.data_ptr(), A, obs.data_ptr(), rew.data_ptr(), flags.data_ptr(),
                                      nup.data_ptr(), lab.data_ptr(), target_label=K - 1, update_cap=CAP)

        for t in range(warmup):
            step(t)
        b.sync()
        t0 = time.perf_counter()
        for t in range(warmup, warmup + steps):
            step(t)
        b.sync()
        out[leg] = (time.perf_counter() - t0) / steps
        torch.cuda.synchronize()
        # of the last step: the legs must agree (same trajectory), and how long the loops were
        sums[leg] = (int(nup.to(torch.int64).sum().item()), int(obs.sum().item()))
        out.setdefault("mean_updates_last_step", float(nup.to(torch.float64).mean().item()))
        out.setdefault("capped_last_step", int(((flags & 4) != 0).sum().item()))
        b.close()
    assert len(set(sums.values())) == 1, f"the legs computed different trajectories: {sums}"
    return out


def summary(values):
    med = statistics.median(values)
    return {"runs_ms": [1e3 * v for v in values], "median_ms": 1e3 * med, "spread_ms": 1e3 * (max(values) - min(values)),
            "env_steps_per_s": N_ENVS / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="", help="run one round on this network and print its JSON line")
    ap.add_argument("--steps", type=int, default=40, help="timed env steps per leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "env_set.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.steps, args.warmup)))
        return 0
    result = {"n_envs": N_ENVS, "update_cap": CAP, "actions_per_row": A, "rounds": ROUNDS, "steps": args.steps,
              "warmup": args.warmup, "unit": "wall clock per env step of the whole batch, one launch per step",
              "tt200_attractor_states": TT200_STATES, "networks": []}
    for network in ("bittner28", "tt200"):
        rounds = []
        for r in range(ROUNDS):
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, __file__, "--child", network,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"round {r} on {network} ended with status {p.returncode}; stopping", file=sys.stderr)
                return p.returncode
            rounds.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(rounds[-1]), flush=True)
        legs = {k: summary([x[k] for x in rounds]) for k in LEGS if k in rounds[0]}
        entry = {k: rounds[0][k] for k in ("network", "n_attractors", "n_states", "n_cubes", "mean_updates_last_step",
                                           "capped_last_step")}
        entry.update(legs)
        b = legs["b_k_env_set"]
        entry["b_over_a"] = b["median_ms"] / legs["a_k_env_cubes"]["median_ms"]
        for k in ("c_no_hull", "d_no_skip"):
            if k in legs:
                entry[f"{k}_slower_than_b_beyond_spread"] = legs[k]["median_ms"] - b["median_ms"] > b["spread_ms"]
        result["networks"].append(entry)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")  # after every network: a later one may be refused
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
