#!/usr/bin/env python3
"""Macro-action env step at tt200: k fused PBN-v0 steps against one macro launch. Measurement only.

Per macro step of the whole batch, wall time (all launches queued, then one sync), at 1,048,576 and 65,536 envs:
  (a) k = 8 calls of pbn_tenv_step_device: what the library offered before the macro kernel. It has no ragged form
      -- every call steps every env -- so an agent whose envs chose intervals in [1, 8] pays the k = 8 cost (and
      would still have to mask and sum the rewards itself, which is not timed here);
  (b) one pbn_tenv_macro_device call, interval mode, t_max = 8: every interval 8 ("uniform"), and intervals drawn
      uniformly from [1, 8] ("ragged": lanes of a wave leave the loop at different rounds);
  (c) the same call in trigger mode, stop probabilities drawn uniformly from [1, 10] tenths, t_max = 8.
Five rounds; a round is one child process that runs the legs in turn, so the legs alternate, and every child runs
under its own time limit. Medians and spreads (max - min over the rounds) go to profiles/macro_env.json, with the
time per inner update (the macro step's time over the mean number of rounds an env ran).

The envs are those of tools/bench_vec_pbn_env.py: one made-up attractor of 64 states with x_0 = 0, whose first
state is the target. Hits are rare, which does not change what a round costs: every env is looked up every round.
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

SIZES = (1 << 20, 1 << 16)
ROUNDS = 5
K = 8
CHILD_LIMIT_S = 300
LEGS = ("a_k_steps", "b_macro_uniform", "b_macro_ragged", "c_trigger")


def child(B: int, steps: int) -> dict:
    import numpy as np
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import pack_bits
    from gym_pbn_amd.macro_env import gamma_powers, stop_thresholds
    from gym_pbn_amd.network import synthetic_truth_table_pbn
    from gym_pbn_amd.torch_env import TorchVecPBNEnv

    data = synthetic_truth_table_pbn(200, 4, seed=0)  # the network of data/tt200.npz
    N = 200
    rng = np.random.default_rng(1)
    att = rng.integers(0, 2, size=(64, N), dtype=np.uint8)
    att[:, 0] = 0
    goal = {"target_nodes": {tuple(int(v) for v in att[0])}}
    acts = rng.integers(1, N, size=B).astype(np.int32)
    acts[rng.random(B) < 0.5] = 0
    ragged = rng.integers(1, K + 1, size=B).astype(np.int32)
    probs = rng.integers(1, 11, size=B).astype(np.int32)

    env = TorchVecPBNEnv(data, goal_config=goal, n_envs=B, all_attractors=[pack_bits(att)], seed=7)
    b = env.batch
    b.randomize()
    dev = env.device
    d_acts = torch.from_numpy(acts).to(dev)
    d_uniform = torch.full((B,), K, dtype=torch.int32, device=dev)
    d_ragged = torch.from_numpy(ragged).to(dev)
    d_probs = torch.from_numpy(probs).to(dev)
    d_gpow = torch.from_numpy(gamma_powers(0.99, K)).to(dev)
    d_thr = torch.from_numpy(stop_thresholds().view(np.int64)).to(dev)
    labels = torch.empty(B, dtype=torch.int32, device=dev)
    reward = torch.empty(B, dtype=torch.int32, device=dev)
    reward_f = torch.empty(B, dtype=torch.float64, device=dev)
    interval = torch.empty(B, dtype=torch.int32, device=dev)
    first_hit = torch.empty(B, dtype=torch.int32, device=dev)
    flags = torch.empty(B, dtype=torch.uint8, device=dev)
    words = torch.empty((B, env.W), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def k_steps():
        for _ in range(K):
            b.tenv_step_device(env.target, d_acts.data_ptr(), reward.data_ptr(), flags.data_ptr(),
                               d_obs=words.data_ptr(), d_labels=labels.data_ptr())

    def macro(mode, d_limit, **kw):
        b.tenv_macro_device(env.target, mode, K, d_acts.data_ptr(), d_limit.data_ptr(), flags.data_ptr(),
                            d_obs=words.data_ptr(), d_interval=interval.data_ptr(), d_first_hit=first_hit.data_ptr(),
                            d_labels=labels.data_ptr(), **kw)

    def interval_mode(d_limit):
        return lambda: macro(_lib.MACRO_INTERVAL, d_limit, d_reward_i32=reward.data_ptr())

    def trigger_mode():
        macro(_lib.MACRO_TRIGGER, d_probs, d_reward_f64=reward_f.data_ptr(), d_gpow=d_gpow.data_ptr(),
              d_stop_thr=d_thr.data_ptr())

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    out = {"B": B}
    out["a_k_steps"] = timed(k_steps)
    out["b_macro_uniform"] = timed(interval_mode(d_uniform))
    out["b_macro_ragged"] = timed(interval_mode(d_ragged))
    out["c_trigger"] = timed(trigger_mode)
    out["ragged_mean_rounds"] = float(ragged.mean())
    out["trigger_mean_rounds"] = float(interval.to(torch.float64).mean().item())  # of the last trigger call
    env.close()
    return out


def summary(values):
    return {"runs": values, "median": statistics.median(values), "spread": max(values) - min(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0, help="run one round at this many envs and print its JSON line")
    ap.add_argument("--steps", type=int, default=100, help="timed macro steps per leg")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "macro_env.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args.steps)))
        return 0
    result = {"network": "tt200", "rounds": ROUNDS, "steps": args.steps, "k": K,
              "unit": "seconds per macro step of the whole batch, wall clock", "sizes": []}
    for B in SIZES:
        rounds = []
        for r in range(ROUNDS):
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, __file__, "--child", str(B),
                   "--steps", str(args.steps)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"round {r} at {B} envs ended with status {p.returncode}; stopping", file=sys.stderr)
                return p.returncode
            rounds.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(rounds[-1]), flush=True)
        legs = {k: summary([x[k] for x in rounds]) for k in LEGS}
        mean_rounds = {"a_k_steps": K, "b_macro_uniform": K, "b_macro_ragged": rounds[0]["ragged_mean_rounds"],
                       "c_trigger": statistics.median([x["trigger_mean_rounds"] for x in rounds])}
        a, bu, br = legs["a_k_steps"], legs["b_macro_uniform"], legs["b_macro_ragged"]
        result["sizes"].append({
            "n_envs": B, **legs, "mean_rounds_per_env": mean_rounds,
            "s_per_inner_update": {k: legs[k]["median"] / mean_rounds[k] for k in LEGS},
            "speedup_b_uniform_over_a": a["median"] / bu["median"],
            "speedup_b_ragged_over_a": a["median"] / br["median"],
            "b_uniform_faster_than_a_beyond_a_spread": a["median"] - bu["median"] > a["spread"],
            "b_ragged_faster_than_a_beyond_a_spread": a["median"] - br["median"] > a["spread"],
            "ragged_over_uniform_per_macro_step": br["median"] / bu["median"],
            "ragged_over_uniform_per_inner_update": (br["median"] / mean_rounds["b_macro_ragged"]) / (bu["median"] / K),
        })
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
