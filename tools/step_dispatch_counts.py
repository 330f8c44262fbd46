#!/usr/bin/env python3
"""Which path each pbn_step call takes, read off a kernel trace: the acceptance check of a change to step
mode's host side that must not change the device work of any call.

Without arguments: 4,099 Bittner-200 envs, step(1, 2, 3, 20, 20, 64, 65, 130, 200) with prepare_steps(20) before
the second 20, then the state's digest. Run it under ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR
-o run -- python tools/step_dispatch_counts.py`` once per library (``PBNSIM_LIB``) and ``PBNSIM_STEP_CHAINS``.

``--count DIR``: dispatches of k_step, k_bump and k_set_counters in DIR's kernel trace. k_bump ends every
power-of-two replay, k_set_counters precedes every call that replays graphs, an exact-length replay has neither:
equal counts of the three mean every call took the same path.
"""
import csv
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CALLS = (1, 2, 3, 20, 20, 64, 65, 130, 200)
KERNELS = ("k_step", "k_bump", "k_set_counters")


def count(trace_dir):
    files = sorted(Path(trace_dir).rglob("*kernel_trace.csv"))
    assert files, f"no kernel trace under {trace_dir}"
    n = dict.fromkeys(KERNELS, 0)
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                for k in KERNELS:
                    if k in row["Kernel_Name"]:
                        n[k] += 1
    return n


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--count":
        print(json.dumps(count(sys.argv[2])))
        return
    sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))
    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch("bittner199", 4099, seed=3)
    b.randomize()
    for k, n in enumerate(CALLS):
        if k == 4:
            b.prepare_steps(20)
        b.step(n)
    state = b.get_state()
    print(json.dumps({"step_chains": b.info()["step_chains"], "updates": b.info()["update_count"],
                      "state_sha256": hashlib.sha256(state.tobytes()).hexdigest()[:16]}))
    b.close()


if __name__ == "__main__":
    main()
