#!/usr/bin/env python3
"""Benchmark: env-steps/s of the async PBN update on Bittner-200 at 1M envs per GPU.

Workload (BASELINE.json configs[2], metric "env-steps/sec (whole node), Bittner-200,
batch=1M; achieved HBM GB/s"): the exported ``predictor_sets_200_5_kmeans`` network
(N=199 nodes, 994 predictors, W=4 state words), 1,048,576 independent envs per GPU
resident in HBM as bit-packed uint64 words. One bench *step* = one R1 async
transition (``Graph.step``, base.py:306-312) for every env = one ``pbn_step`` launch
(state read from and written back to device memory). Philox4x32-10 RNG in-register.

Multi-GPU: ``python bench.py --gpus N`` starts ``torch.distributed.run`` with N ranks as a
child process (before anything touches a GPU) when ``WORLD_SIZE`` is not set, and exits with
its code; under ``torch.distributed.run`` ``--gpus`` must equal ``WORLD_SIZE``. Each rank owns
1,048,576 envs with global ids [rank*B, (rank+1)*B) -- weak scaling, no data-path collective
(envs are independent); barrier + max-over-ranks timing; ``n_gpus`` = the process group's size.

A plain run (``bench.py --gpus N --steps K --warmup W``) does only what the headline needs: it sets
up the batch, runs the W warm-up launches, times the K launches, writes the final state when
``--dump-outputs DIR`` is given and prints the line (``value``, ``ms_per_step``, ``config``, ``dist``).
Everything below -- the supplementary measurements, the roofline with its twin-batch kernel time and
changed fraction, the memory-floor probe, the copy bandwidth, the shard self-checks and the CPU
baseline -- runs only with ``--full`` and adds its keys to the same line.

``--dump-outputs DIR``: after the timed launches, the state the stepped batch holds (what ``get_state``
returns to a caller) is written as ``DIR/state.npy`` -- float32 0/1 node values, one row per env of a
fixed, seeded sample of the rank's envs -- with the rows' global env ids in ``DIR/env_ids.npy``
(float64). Same arguments, same inputs (seeded Philox), so two builds can be compared row for row.
At N > 1 every rank writes ``state_rank<r>.npy`` / ``env_ids_rank<r>.npy``.

Order with ``--full``: the supplementary measurements (rollout, BASELINE config 2, the past-MALL 8M-env
step run, config 5's R6 chunks with their all-gather) run first, the headline's W warm-up and K
timed launches after them. The per-launch time depends on where the trajectory is: from fair-bit
initial states about 40 % of envs change their updated bit per launch and are written back,
falling to about 9 % after ~1,000 launches -- not a clock ramp. The roofline's
bytes follow the window actually timed: the changed fraction over exactly the K timed launches
is measured on a twin batch (same seed: identical Philox trajectory) after the timing, and so is the
kernel time (a HIP-event region over the same K launches of a twin batch: the timed window itself
carries no instrumentation). ``peak`` is the fixed 8 TB/s HBM spec; the 1M line's state stays in
the Infinity Cache (MALL), so the measured ceiling of its access pattern (``tools/mall_probe.hip``:
the same launch shape and bytes, no compute) is reported beside it (``floor_GBs``,
``frac_of_floor`` = kernel floor / kernel time); the guide's MALL gather rate stays as a labelled,
read-only reference. The 8M-env run (256 MiB of state, past the MALL) carries the HBM-bound figure.

Self-checks (``--full``, any N): ``shard_check`` re-runs sampled global env ids as 2-env batches and compares
them with the sharded run (Philox keyed by global id: a one-GPU run gives those ids the same
trajectory), digesting every rank's rows in global-id order; ``dist`` names the process group's
backend and size and every rank's kernel time; config 5's actions are keyed by global env id.

Prints ONE JSON line (rank 0); with ``--full`` it carries ``roofline`` and ``cpu_baseline`` (the
oracle's C restatement on host cores, rank 0 at N = 1 only).
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "gym-pbn-stac_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# MI355X_MICROARCH.md "Indexed rows: gather into LDS": rows of a 38 MB table served from the Infinity
# Cache (MALL) read at 8.6 TB/s chip-wide -- the guide's only MALL rate, used as the 1M line's peak
MALL_PEAK_GBS = 8600.0
VALU_PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12  # 256 CUs x 4 SIMD32 x 32 lanes/clk x 2.4 GHz = 78.6 T lane-ops/s


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--network", default="bittner199")
    p.add_argument("--batch", type=int, default=1 << 20, help="envs per GPU")
    p.add_argument("--seed", type=int, default=0x5EED)
    p.add_argument("--full", action="store_true",
                   help="also run the supplements, the roofline's runs (twin-batch kernel time, changed fraction, "
                        "memory floor, copy bandwidth), the shard self-checks and the CPU baseline; the options "
                        "below that tune or skip those apply with --full only")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write the stepped batch's final state (a fixed, seeded sample of envs, "
                        "float32 node values) and the sampled global env ids as DIR/<name>.npy")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-seconds", type=float, default=10.0)
    p.add_argument("--rollout", type=int, default=64, help="updates per launch for the supplementary rollout line")
    p.add_argument("--pmc-file", default=str(ROOT / "profiles" / "pmc_traffic.json"))
    p.add_argument("--valu-file", default=str(ROOT / "profiles" / "r06_valu_pmc.json"))
    p.add_argument("--kernel-only", action="store_true", help="just run steps (for rocprofv3 child runs)")
    p.add_argument("--r6-chunks", type=int, default=2, help="config-5 supplement: timed T=100 chunks (0 = off)")
    p.add_argument("--r6-batch", type=int, default=131072, help="config-5 supplement: envs per GPU")
    p.add_argument("--no-r6-variants", dest="r6_variants", action="store_false",
                   help="config-5 supplement: skip the high-cap and SURVEY-spec-attractor figures")
    p.add_argument("--no-config2", dest="config2", action="store_false", help="skip the Bittner-28 supplement")
    p.add_argument("--no-beyond-mall", dest="beyond_mall", action="store_false",
                   help="skip the 8M-env (state past the MALL) step-mode supplement that carries the HBM roofline")
    p.add_argument("--no-probe", dest="probe", action="store_false", help="skip the memory-floor probe")
    p.add_argument("--no-mt", dest="mt", action="store_false", help="skip the MT-mode (reference RNG) supplement")
    p.add_argument("--dist-backend", default="nccl",
                   help="process group for the barrier / max-over-ranks timing (nccl = RCCL); gloo lets several "
                        "ranks share one GPU for rehearsals")
    p.add_argument("--dist-timeout", type=float, default=600.0,
                   help="seconds before a collective waiting on a dead peer fails (process-group timeout)")
    p.add_argument("--check-launch", action="store_true",
                   help="multi-rank plumbing only (process group, barrier, max over ranks, the JSON line): no GPU work")
    return p.parse_args()


# Device and process-group plumbing in one place: tests/test_bench_dist.py replaces these four with
# CPU stand-ins to rehearse the multi-rank bookkeeping (gloo, world 2) without a GPU.
def _dev(device):
    import torch

    return torch.device("cuda", device)


def _sync():
    import torch

    torch.cuda.synchronize()


def _set_device(local):
    """This rank's GPU (one process per GPU): LOCAL_RANK modulo the visible devices."""
    import torch

    n = max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local % n)
    return local % n


def _init_dist(backend, timeout_s):
    """The process group; a rank whose init fails raises (non-zero exit) and torch.distributed.run
    then stops the others; the timeout bounds every later collective (a peer that died mid-run)."""
    import datetime

    import torch.distributed as dist

    dist.init_process_group(backend, timeout=datetime.timedelta(seconds=timeout_s))
    return dist


def dist_env():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    return world, rank, local


def spawn_ranks(n: int) -> int:
    """``--gpus N`` without torch.distributed.run: start it as a CHILD process (nothing here has
    touched a GPU) with N ranks on this node and return its exit code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
    return subprocess.run(cmd).returncode


def cpu_baseline(net, seconds: float):
    """Oracle (C restatement, same semantics and Philox stream) timed on host cores; bounded sample."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O

    O.build()
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    o = O.Oracle(net)
    B = 65536
    st = o.init_philox(B, seed=1)
    T = 8
    t0 = time.perf_counter()
    o.step_philox(st, 1, 0, 0, T, n_threads=threads)
    dt = time.perf_counter() - t0
    T = max(8, int(T * seconds / max(dt, 1e-6)))
    t0 = time.perf_counter()
    o.step_philox(st, 1, 0, 0, T, n_threads=threads)
    dt = time.perf_counter() - t0
    return {"value": B * T / dt, "unit": "env-steps/s", "cores": threads, "kind": "port",
            "sample": f"oracle/pbn_oracle.c orc_step_philox, {net.name}, {B} envs x {T} updates "
                      f"({dt:.1f} s, OpenMP {threads} threads)",
            "reference_python_1core_measured_in_build_container": "20-28k env-steps/s (BASELINE.md)"}


def read_pmc(path: str, key: str):
    """Committed PMC results (profiles/): per-launch HBM-side bytes for network:batch, or None."""
    try:
        pmc = json.loads(Path(path).read_text())
    except (OSError, ValueError):
        return None, None
    return pmc.get("per_launch_bytes", {}).get(key), pmc.get("source")


def read_pmc_window(path: str, key: str):
    """The launch window [lo, hi) the committed PMC median was taken over (tools/pmc_traffic.py), or None."""
    try:
        return json.loads(Path(path).read_text()).get("detail", {}).get(key, {}).get("window")
    except (OSError, ValueError):
        return None


class MemFloor:
    """tools/libmallprobe.so: the step kernel's memory pattern without compute (see mall_probe.hip)."""

    def __init__(self):
        self.lib = ctypes.CDLL(str(ROOT / "tools" / "libmallprobe.so"))
        self.lib.mall_probe.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_double)]

    def us_per_launch(self, n_envs: int, write_pct: int, launches: int) -> float:
        us = ctypes.c_double()
        rc = self.lib.mall_probe(n_envs, write_pct, 1, launches, ctypes.byref(us))
        if rc:
            raise RuntimeError(f"mall_probe failed: {rc}")
        return us.value


def window_changed_fraction(net, B, device, seed, env_base, warmup, steps):
    """Mean fraction of envs whose updated node changed value per launch over launches
    [warmup, warmup + steps) of a batch -- the envs the dirty-store kernel writes back. Measured
    on a TWIN batch (same network, seed, env ids, fair-bit start: Philox makes its trajectory
    identical), one launch at a time with the state compared on the device, after the timed run."""
    import torch

    from gym_pbn_amd.batch import PBNBatch

    dev = torch.device("cuda", device)
    b = PBNBatch(net, B, device=device, seed=seed, env_id_base=env_base)
    b.set_stream(torch.cuda.current_stream(dev).cuda_stream)  # one stream: the copies and compares in order
    b.randomize()
    b.step(warmup)
    x = torch.empty((B, net.n_words), dtype=torch.int64, device=dev)
    y = torch.empty_like(x)
    n = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(steps):
        b.get_state_device(x.data_ptr())
        b.step(1)
        b.get_state_device(y.data_ptr())
        n += (x != y).any(dim=1).sum()
    torch.cuda.synchronize(dev)
    b.set_stream(None)
    b.close()
    return float(n.item()) / (B * steps)


def step_run(net, B, device, seed, warmup, steps, env_base=0):
    """W + K step launches on a fresh batch; K timed with HIP events on the batch stream (the K
    launches' graph captured beforehand, so the timed call is one graph replay)."""
    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch(net, B, device=device, seed=seed, env_id_base=env_base)
    b.randomize()
    b.step(warmup)
    b.prepare_steps(steps)
    b.sync()
    time.sleep(0.005)  # idle gap: the timed launches are a run of their own in a kernel trace
    b.timing(2)
    b.step(steps)
    b.timing(0)
    ms, launches = b.timing_read()
    return b, ms / 1e3 / max(launches, 1)


def min_bytes(n_words: int, B: int, q: float) -> float:
    """Bytes one step launch must move: every env's state read (8W B), the envs whose bit changed
    written back (8W B each). SURVEY §8(d) prices 16W B per update (every env written): the
    kernel writes an env only if its updated bit changed, so that figure exceeds what it moves."""
    return 8.0 * n_words * B * (1.0 + q)


def beyond_mall_supplement(net, device, seed, floor):
    """Step mode on 8,388,608 envs on ONE GPU (BASELINE config 4's whole batch): 256 MiB of
    state, as large as the 256 MiB MALL, so every launch streams the state from HBM. Algorithmic
    bytes (64 B per update) / HIP-event kernel time against the 8 TB/s HBM spec."""
    B, W_, K_ = 1 << 23, 50, 200
    b, s = step_run(net, B, device, seed, W_, K_)
    b.close()
    q = window_changed_fraction(net, B, device, seed, 0, W_, K_)
    alg = min_bytes(net.n_words, B, q)
    contract = 16 * net.n_words * B
    out = {"workload": "Bittner-200 step mode, 8,388,608 envs on one GPU (state 256 MiB, past the MALL)",
           "bound": "hbm", "achieved": alg / s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": alg / s / 1e9 / HBM_PEAK_GBS, "avg_kernel_us": s * 1e6, "launches_timed": K_,
           "warmup_launches": W_, "alg_bytes_per_launch": alg, "changed_env_frac": q,
           "contract_accounting": {
               "bytes_per_launch": contract, "GBs": contract / s / 1e9,
               "note": "SURVEY 8(d) prices 16W B per update (every env written back); the kernel writes only "
                       "the envs whose bit changed, so this is accounting, not moved bytes (it can exceed the "
                       "8 TB/s peak)"},
           "env_steps_per_s": B / s}
    traffic, src = read_pmc(str(ROOT / "profiles" / "pmc_traffic.json"), f"{net.name}:{B}")
    out["traffic"] = traffic
    if traffic:
        out["traffic_GBs"] = traffic / s / 1e9
        out["traffic_frac"] = traffic / s / 1e9 / HBM_PEAK_GBS
        out["traffic_over_alg"] = traffic / alg
        out["traffic_window"] = read_pmc_window(str(ROOT / "profiles" / "pmc_traffic.json"), f"{net.name}:{B}")
        out["timed_window"] = [W_, W_ + K_]
    if floor is not None:
        fl = floor.us_per_launch(B, round(100 * q), 50)
        out["floor_us"] = fl
        out["frac_of_floor"] = fl / (s * 1e6)
    return out


def copy_bandwidth(device, gib: float = 2.0, reps: int = 10):
    """Achievable HBM rate on this box: a device-to-device copy of a buffer far past the MALL,
    (read + write bytes) / time from CUDA events. Context for the roofline's fractions."""
    import torch

    n = int(gib * (1 << 30))
    src = torch.empty(n, dtype=torch.uint8, device=f"cuda:{device}")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        dst.copy_(src)
    t1.record()
    torch.cuda.synchronize()
    s = t0.elapsed_time(t1) / 1e3 / reps
    del src, dst
    torch.cuda.empty_cache()
    return 2 * n / s / 1e9


def config2_supplement(device):
    """BASELINE config 2 beside the main line: Bittner-28 (predictor_sets_28_15_median, N = 28,
    one state word), 65,536 envs on one GPU (512 KiB of state: launch-bound in step mode), step
    mode (one Graph.step per env per launch) and rollout (256 updates per launch)."""
    from gym_pbn_amd.network import load_network

    B = 65536
    b, s = step_run(load_network("bittner28"), B, device, 0x5EED, 500, 2000)
    b.rollout(256)
    b.sync()
    b.timing(2)
    for _ in range(5):
        b.rollout(256)
    b.timing(0)
    rms, rl = b.timing_read()
    lanes = b.info()["roll_lanes"]
    b.close()
    return {"workload": "Bittner-28, 65,536 envs, 1 GPU (BASELINE config 2)",
            "step_env_steps_per_s": B / s, "step_us_per_launch": s * 1e6,
            "rollout_updates_per_launch": 256, "rollout_node_updates_per_s": B * 256 * 5 / (rms / 1e3),
            "rollout_lanes_per_env": lanes}


MT_WORDS_PER_UPDATE = 256 / 199 + 2.0  # Bittner-199: randint(0, 198) takes 256/199 words on average, random() 2


def mt_supplement(net, device, B=1 << 20, T=256, reps=3):
    """MT mode: every env runs the reference's own CPython MT19937, seeded from the
    Python seed alone (random.seed(s); genRandState(); Graph.step() x T, base.py:7,94,306-312,368-370) --
    the path that reproduces the reference bit for bit from its seed. Bittner-199, 1,048,576 envs, T updates
    per pbn_mt_step launch. Algorithmic bytes: the MT words an update consumes (MT_WORDS_PER_UPDATE), each
    twisted once (read + written) and read once by the walk that draws from it (12 B per word: the 2,496-B
    table per 624 words three times; the walk comes hundreds of updates after the twist, so the word is
    re-read, not kept) + the packed state read and written once per launch; against the 8 TB/s HBM spec (the
    2.5 GiB of tables are past the MALL)."""
    import numpy as np

    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch(net, B, device=device, seed=1)
    b.mt_seed(np.arange(B, dtype=np.uint64) + 12345, init_state=True)
    b.mt_step(T)  # warm-up (also moves every env past its first twists)
    b.sync()
    b.timing(2)
    for _ in range(reps):
        b.mt_step(T)
    b.timing(0)
    ms, n = b.timing_read()
    b.close()
    s = ms / 1e3 / reps
    alg = B * T * MT_WORDS_PER_UPDATE * 12 + 16 * net.n_words * B
    return {"workload": f"MT mode (reference RNG streams on the device), Bittner-199, {B} envs, T = {T} updates "
                        "per launch", "node_updates_per_s": B * T / s, "ms_per_launch": s * 1e3,
            "roofline": {"bound": "hbm", "achieved": alg / s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": alg / s / 1e9 / HBM_PEAK_GBS, "alg_bytes_per_launch": alg,
                         "alg_bytes_rule": f"{MT_WORDS_PER_UPDATE:.3f} MT words per update x 12 B (twist read + write, walk "
                              "read) "
                                           "+ 16W B of packed state per env per launch"},
            "kernel": "pbn::k_mt_staged (LDS-DMA windows, draw ring, cooperative twists; csrc/pbn_mt.hip)"}


def rollout_supplement(net, B, device, seed, T, valu):
    """Rollout mode (T updates per launch, state in the LDS plane): VALU-bound."""
    from gym_pbn_amd.batch import PBNBatch

    b = PBNBatch(net, B, device=device, seed=seed)
    b.randomize()
    b.rollout(T)
    b.sync()
    b.timing(2)
    reps = 5
    for _ in range(reps):
        b.rollout(T)
    b.timing(0)
    rms, rl = b.timing_read()
    b.close()
    s = rms / 1e3 / max(rl, 1)
    out = {"updates_per_launch": T, "node_updates_per_s_per_gpu": B * T / s, "kernel_ms": s * 1e3}
    v = (valu or {}).get(f"k_rollout:{net.name}:{B}:{T}")
    if v:
        out["roofline"] = valu_roofline(v, s, B * T)
    return out


def valu_roofline(v, s, updates):
    """VALU roofline: VALU wave-instructions per node update from committed SQ counters
    (profiles/r03_valu_pmc.json, tools/valu_pmc.py: SQ_INSTS_VALU over a profiled launch of the
    same kernel, batch and seeds / its node updates) x this run's node updates / its kernel time,
    against the chip's VALU issue peak (64 lanes per wave-instruction)."""
    ipu = v["valu_wave_insts_per_update"]
    lane_ops = ipu * updates * 64
    out = {"bound": "valu", "achieved": lane_ops / s / 1e12, "peak": VALU_PEAK_TOPS, "unit": "T lane-ops/s",
           "frac": lane_ops / s / 1e12 / VALU_PEAK_TOPS, "valu_wave_insts_per_update": ipu,
           "frac_source": "issue slots: SQ_INSTS_VALU x 64 lane-ops per wave-instruction, masked lanes included",
           "valu_busy_frac": v.get("valu_busy_frac"), "kernel_s": s, "node_updates": updates,
           "source": v.get("source", "profiles/r06_valu_pmc.json")}
    alf = v.get("active_lane_frac")
    if alf is not None:  # useful work: lane-ops of enabled lanes only
        out["active_lane_frac"] = alf
        out["frac_active_lanes"] = out["frac"] * alf
        out["frac_active_lanes_source"] = ("frac x active_lane_frac, active_lane_frac = SQ_THREAD_CYCLES_VALU / "
                                           "(SQ_ACTIVE_INST_VALU x 64) from the same PMC pass (rocprofv3's VALUUtilization)")
    return out


def r6_figure(args, world, rank, device, dist, valu, spec, cap, n_chunks, gather=True, check=False):
    """One config-5 figure: the multi-flip until-attractor env (pbn_target_multi.py:119-154) on
    Bittner-200, ``--r6-batch`` envs per GPU (131,072: 1M over 8 GPUs), T = horizon = 100 env steps per
    chunk written to a device chunk and all-gathered across ranks (RCCL) while the next chunk runs;
    A = 4 action slots (0 w.p. 0.75) drawn by ``actions.env_actions`` from Philox seed 0xAC7 keyed by
    GLOBAL env id and env step, so the global batch is one workload at any GPU count;
    attractors ``spec`` (r6_attractors); update cap ``cap``. Timed twice: one launch per env step
    (closed loop), then one launch per chunk (actions known for it). Every timed chunk reports its
    kernel time (HIP events, read after the timed window) and the slowest env's updates; the last fused
    launch's tail hand-offs are reported once;
    with ``check`` the fused run's last chunk is checked on sampled global ids (r6_shard_check)."""
    import torch

    from gym_pbn_amd.actions import env_actions
    from gym_pbn_amd.batch import EnvConfig, Net, PBNBatch
    from gym_pbn_amd.network import load_network
    from gym_pbn_amd.rollout import TrajectoryCollector, gather_chunk
    from gym_pbn_amd.shard import max_over_ranks, shard_for

    T, B, A = 100, args.r6_batch, 4
    net = Net(load_network("bittner199"))
    atts, desc = r6_attractors(spec, net.n_nodes)
    cfg = EnvConfig(net, atts, horizon=T)
    sh = shard_for(rank, world, B)
    dev = _dev(device)
    acts = env_actions(T, sh.env_base, B, A, net.n_nodes, seed=0xAC7, device=dev)

    def chunk_stats(buf):
        # per env step: the slowest env (a per-step launch waits for it) and the mean; capped envs
        n = buf["n_updates"]
        return n.to(torch.int64).sum(), torch.stack([n.max(dim=1).values.to(torch.float64),
                                                     n.to(torch.float64).mean(dim=1),
                                                     ((buf["flags"] & 4) != 0).to(torch.float64).mean(dim=1)])

    def run(fused):
        b = PBNBatch(net, B, device=device, env_id_base=sh.env_base, seed=0xAC7)
        col = TrajectoryCollector(b, cfg, T, A, dev, update_cap=cap, dist=dist if gather else None, fused=fused)

        def chunks(diag=None):
            # nothing is read back to the host inside the loop: the per-chunk figures stay on
            # the device (slowest env) or in the batch's event pairs (kernel ms), read after the window
            ups = torch.zeros((), dtype=torch.int64, device=dev)
            stats = []
            for _ in range(n_chunks):
                buf, _ = col.step_chunk(acts)
                u, st = chunk_stats(buf)
                ups += u
                stats.append(st)
                if diag is not None:  # the env whose T env steps took the most updates: a fused chunk ends with it
                    diag.append(buf["n_updates"].to(torch.int64).sum(dim=0).max())
            return buf, ups, stats

        def diag_after(slowest):
            # every chunk issues the same launches: the per-launch kernel times split evenly into chunks
            each = b.timing_read_each()
            per = max(len(each) // max(n_chunks, 1), 1)
            return [{"kernel_ms": float(sum(each[k * per:(k + 1) * per])), "launches": per,
                     "slowest_env_updates": int(x.item())} for k, x in enumerate(slowest)]

        # warm-up: the timed loop itself, untimed, with the per-launch events on -- the first use
        # of the events (created on demand, then reused) and of torch's small kernels costs tens
        # of ms, which otherwise landed in the first timed per-step chunks (48-79 vs 97 M env-steps/s)
        b.timing(1)
        chunks()
        b.timing(0)
        col.finish()
        _sync()
        if dist is not None:
            dist.barrier()
        b.timing(1)  # an event pair around every launch on the batch stream: kernel time alone
        diag = []
        t0 = time.perf_counter()
        buf, ups, stats = chunks(diag)
        col.finish()
        _sync()
        if dist is not None:
            dist.barrier()
        dt = max_over_ranks(time.perf_counter() - t0, dist, device=dev)
        diag = diag_after(diag)
        b.timing(0)
        kms = sum(d["kernel_ms"] for d in diag)
        local_ups = float(ups.item())
        if dist is not None:
            dist.all_reduce(ups)
        st = torch.cat(stats, dim=1).cpu().numpy()
        tail = {"capped_frac": float(st[2].mean()), "mean_updates_per_env_step": float(st[1].mean()),
                "max_updates_per_env_step_mean_over_steps": float(st[0].mean()),
                "steps_whose_slowest_env_hit_the_cap": float((st[0] >= cap).mean())}
        return b, buf, dt, float(ups.item()), tail, (kms / 1e3, local_ups), diag

    # closed-loop shape first (one launch per env step, as an agent in the loop needs), then the
    # open-loop collector (actions known for the chunk: one launch walks each env through T steps)
    b, buf, dt_step, ups_step, tail_step, k_step, diag_step = run(False)
    b.close()
    b, buf, dt, ups, tail, k_fused, diag = run(True)
    lanes = b.info()["env_lanes"]
    handoffs = b.env_handoffs()  # the last fused launch's tail envs passed between the waves of a workgroup
    out = {"unit": "env-steps/s", "attractors": spec, "attractors_desc": desc, "update_cap": cap,
           "value": world * B * T * n_chunks / dt, "node_updates_per_s": ups / dt,
           "launch": "one per chunk (T env steps per env in one launch; actions known for the chunk)",
           "value_one_launch_per_env_step": world * B * T * n_chunks / dt_step,
           "node_updates_per_s_one_launch_per_env_step": ups_step / dt_step,
           "batch_per_gpu": B, "global_batch": world * B, "T": T, "A": A, "env_lanes": lanes,
           "actions": "actions.env_actions: Philox seed 0xAC7 keyed by global env id and env step (stream 9)",
           "chunks": n_chunks, "s_per_chunk": dt / n_chunks, "tail": tail,
           "tail_one_launch_per_env_step": tail_step,
           "chunk_diag": diag, "chunk_diag_one_launch_per_env_step": diag_step,
           "handoffs_last_fused_launch": handoffs,
           "chunk_bytes_per_gpu": sum(t.numel() * t.element_size() for t in buf.values())}
    for key, (ks, nu), name in ((f"k_env:bittner199:{B}:fused{T}", k_fused, "roofline"),
                                (f"k_env:bittner199:{B}:per_step", k_step, "roofline_one_launch_per_env_step")):
        vr = (valu or {}).get(key) if (spec == "fixture" and cap == 4096) else None
        if vr and ks > 0:  # this rank's env kernels: node updates / summed kernel time (HIP events)
            out[name] = valu_roofline(vr, ks, nu)
    if check:
        out["shard_check"] = guarded(r6_shard_check, net, cfg, buf, sh, T, A, cap, 2 * n_chunks, device, dist)
    if dist is not None and gather:  # the gather alone: bytes received per GPU / time
        _sync()
        dist.barrier()
        t0 = time.perf_counter()
        gather_chunk(buf, dist)
        _sync()
        tg = max_over_ranks(time.perf_counter() - t0, dist, device=dev)
        out["all_gather_GBs_per_gpu"] = out["chunk_bytes_per_gpu"] * (world - 1) / tg / 1e9
        out["all_gather_s"] = tg
    b.close()
    return out


def r6_shard_check(net, cfg, buf, sh, T, A, cap, n_chunks_run, device, dist, n_samples=16):
    """Config 5 at any N checks itself: for the sampled global env ids (shard.sampled_env_ids) in this
    rank's shard, a 2-env batch with the same global ids, seed, actions (keyed by global id), cap and
    chunk sequence -- what a one-GPU run gives those envs -- must reproduce the last chunk's obs,
    reward, flags and update counts bit for bit; rank 0 digests every rank's rows in global-id order."""
    import numpy as np
    import torch

    from gym_pbn_amd.actions import env_actions
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.rollout import FIELDS, TrajectoryCollector
    from gym_pbn_amd.shard import gather_rows, max_over_ranks, rows_digest, sampled_env_ids

    dev = _dev(device)
    rows, bad = [], 0
    for g in sampled_env_ids(sh.n_global, n_samples):
        if not sh.env_base <= g < sh.env_base + sh.n_local - 1:
            continue
        s = PBNBatch(net, 2, device=device, env_id_base=g, seed=0xAC7)
        col = TrajectoryCollector(s, cfg, T, A, dev, update_cap=cap, dist=None, fused=True)
        a2 = env_actions(T, g, 2, A, net.n_nodes, seed=0xAC7, device=dev)
        for _ in range(n_chunks_run):
            sbuf, _ = col.step_chunk(a2)
        col.finish()
        j = g - sh.env_base
        ref = {k: buf[k][:, j:j + 2].contiguous() for k in FIELDS}
        bad += 0 if all(torch.equal(sbuf[k], ref[k]) for k in FIELDS) else 1
        rows.append((g, b"".join(np.ascontiguousarray(ref[k].cpu().numpy()).tobytes() for k in FIELDS)))
        s.close()
    all_rows = gather_rows(rows, dist)
    bad = max_over_ranks(float(bad), dist, device=dev)
    return {"sampled_env_pairs": len(all_rows), "match": bad == 0, "digest": rows_digest(all_rows),
            "ranks": dist.get_world_size() if dist is not None else 1,
            "method": "per rank, the sampled global ids in its shard re-run as 2-env batches (same ids, seed, "
                      "actions, cap, chunk sequence); last chunk's obs/reward/flags/n_updates compared bit for bit; "
                      "digest = blake2b-64 over every rank's rows in global-id order (shard.rows_digest)"}


def step_shard_check(net, state, device, seed, env_base, n_local, n_global, n_launches, dist, n_samples=32):
    """The headline at any N checks itself: for the sampled global env ids in this rank's shard, a
    2-env batch with the same global ids and seed, randomized and stepped the same number of launches
    (what a one-GPU run gives those ids: Philox keyed by global id), must equal the sharded batch's
    final state; rank 0 digests every rank's rows in global-id order."""
    import numpy as np

    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.shard import gather_rows, max_over_ranks, rows_digest, sampled_env_ids

    rows, bad = [], 0
    for g in sampled_env_ids(n_global, n_samples):
        if not env_base <= g < env_base + n_local - 1:
            continue
        s = PBNBatch(net, 2, device=device, env_id_base=g, seed=seed)
        s.randomize()
        s.step(n_launches)
        mine = s.get_state()
        s.close()
        ref = np.ascontiguousarray(state[g - env_base:g - env_base + 2])
        bad += 0 if np.array_equal(mine, ref) else 1
        rows.append((g, ref.tobytes()))
    all_rows = gather_rows(rows, dist)
    bad = max_over_ranks(float(bad), dist, device=_dev(device))
    return {"sampled_env_pairs": len(all_rows), "match": bad == 0, "digest": rows_digest(all_rows),
            "ranks": dist.get_world_size() if dist is not None else 1,
            "method": "per rank, the sampled global ids in its shard re-run as 2-env batches (same ids and seed, "
                      "randomize + the same launches); final states compared bit for bit; digest = blake2b-64 over "
                      "every rank's rows in global-id order (shard.rows_digest)"}


R6_HIGH_CAP = 1 << 20  # the longest loop measured at config 5 ran 78,057 updates (profiles/r03_r6_cap_sweep.json)


def r6_supplement(args, world, rank, device, dist, valu):
    """BASELINE config 5 beside the main line (r6_figure): the fixture's attractors with the 4,096
    update cap (the headline figure, ``args.r6_chunks`` chunks), plus, one chunk each and with a cap
    the loop never reached in measurement (so comparable to the reference's unbounded loop,
    pbn_target_multi.py:135-146): the same attractors, and SURVEY §8(d)'s attractor spec."""
    out = {"metric": "R6 env-steps/s (whole node) incl. per-chunk trajectory all-gather",
           **r6_figure(args, world, rank, device, dist, valu, "fixture", 4096, args.r6_chunks, check=True)}
    if args.r6_variants:
        out["high_cap"] = guarded(r6_figure, args, world, rank, device, dist, valu, "fixture", R6_HIGH_CAP, 1)
        out["spec_attractors"] = guarded(r6_figure, args, world, rank, device, dist, valu, "spec", R6_HIGH_CAP, 1)
    return out


# SURVEY §8(d)'s config-5 attractor spec: H = 4 hypercubes over the 7 target genes of
# BittnerMulti7/200 (pbn_target_multi.py:354,415: 234237, 324901, 759948, 25485, 266361, 108208, 130057 =
# nodes 0-6 of the exported Bittner-200 network), other bits '*'. The cubes are the reference's own
# sample cabean output (get_attractors_from_cabean.py:57-81, parsed by parse_attractors :14-36); its
# last attractor (1,1,1,1,1,1,0) is BittnerMulti200's target_node_values (:416).
SPEC_ATTRACTORS_7 = [[(1, 0, 1, 0, "*", "*", 1)], [(1, 0, 1, 1, 1, 1, 0)], [(1, 0, 1, 1, 1, 1, 1)],
                     [(1, 1, 1, 1, 1, 1, 0)]]


def r6_attractors(spec, n_nodes):
    """all_attractors for config 5: "fixture" = the r6_bittner199 fixture's cubes (cabean-like: they
    fix 165 of 199 bits); "spec" = SURVEY §8(d) (SPEC_ATTRACTORS_7 on nodes 0-6, the rest '*')."""
    import numpy as np

    from gym_pbn_amd.batch import attractors_from_cubes

    if spec == "fixture":
        z = np.load(ROOT / "tests" / "golden" / "r6_bittner199.npz", allow_pickle=False)
        return (attractors_from_cubes(z["cube_care"], z["cube_value"], z["cube_attractor"], n_nodes),
                "r6_bittner199 fixture: 4 attractors' cubes fixing 165 of 199 bits (tests/golden/make_golden.py)")
    atts = [[tuple(c) + ("*",) * (n_nodes - 7) for c in a] for a in SPEC_ATTRACTORS_7]
    return atts, ("SURVEY 8(d): 4 cubes over the 7 target genes (nodes 0-6), the reference's sample cabean "
                  "attractors (get_attractors_from_cabean.py:57-81), other bits '*'")


def per_rank(values: dict, dist):
    """Every rank's ``values`` on every rank (rank order), e.g. per-rank kernel time at N > 1."""
    if dist is None:
        return [values]
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, values)
    return parts


def process_census():
    """This process's live child processes (recursive) and thread count when the line is printed, and
    again at exit on stderr -- to name whatever the driver counts after the run (BENCH procs_at_end)."""
    try:
        import psutil

        me = psutil.Process()
        kids = []
        for c in me.children(recursive=True):
            try:
                kids.append({"pid": c.pid, "name": c.name(), "cmdline": " ".join(c.cmdline())[:160]})
            except psutil.Error:
                kids.append({"pid": c.pid, "name": "?"})
        return {"children": kids, "threads": me.num_threads()}
    except Exception as exc:  # diagnostics only
        return {"error": f"{type(exc).__name__}: {exc}"}


def _census_at_exit():
    print("bench.py exit census: " + json.dumps(process_census()), file=sys.stderr, flush=True)


def guarded(fn, *a):
    try:
        return fn(*a)
    except Exception as exc:  # a supplement must not cost the main line
        return {"error": f"{type(exc).__name__}: {exc}"}


def supplements(args, sup, net, B, world, rank, device, dist):
    """``--full``: the supplementary measurements into ``sup`` (every rank); returns the memory-floor
    probe (or None) and rank 0's copy bandwidth."""
    try:
        valu = json.loads(Path(args.valu_file).read_text()).get("kernels", {})
    except (OSError, ValueError):
        valu = {}
    floor = None
    if args.probe:
        try:
            floor = MemFloor()
        except OSError:
            floor = None
    if args.rollout > 1:
        sup["rollout"] = guarded(rollout_supplement, net, B, device, args.seed, args.rollout, valu)
    if args.config2:
        sup["config2_bittner28"] = guarded(config2_supplement, device)
    if args.beyond_mall and B == 1 << 20:
        sup["beyond_mall_8m"] = guarded(beyond_mall_supplement, net, device, args.seed, floor)
    if args.r6_chunks > 0:
        sup["config5_r6"] = guarded(r6_supplement, args, world, rank, device, dist, valu)
    if args.mt and args.network == "bittner199":
        sup["mt_mode"] = guarded(mt_supplement, net, device)
    return floor, (guarded(copy_bandwidth, device) if rank == 0 else None)


DUMP_SAMPLE_SEED = 0xD0A5EED  # the sampled envs depend on the batch size alone
DUMP_MAX_ENVS = 65536         # 65,536 envs x 199 nodes x 4 B = 52 MB (the dump stays under 64 MB)
DUMP_MAX_BYTES = 60_000_000


def dump_outputs(out_dir, state, n_nodes, env_base, rank, world):
    """``--dump-outputs``: the timed batch's final state (``get_state``'s packed words, unpacked to
    float32 0/1 node values) for a fixed, seeded sample of this rank's envs (all of them when they
    fit), and the rows' global env ids (float64: exact below 2^53)."""
    import numpy as np

    from gym_pbn_amd.batch import unpack_bits

    B = state.shape[0]
    n = max(1, min(B, DUMP_MAX_ENVS, DUMP_MAX_BYTES // (4 * n_nodes + 8)))
    rows = np.arange(B) if n == B else np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(B, n, replace=False))
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    tag = "" if world == 1 else f"_rank{rank}"
    np.save(d / f"state{tag}.npy", unpack_bits(state[rows], n_nodes).astype(np.float32))
    np.save(d / f"env_ids{tag}.npy", (rows + env_base).astype(np.float64))


def headline_line(args, net, world, dist, value, elapsed):
    """The line's fields every run prints: the headline figure and the workload it was measured on."""
    return {
        "metric": "env-steps/sec (whole node), Bittner-200, batch=1M; achieved HBM GB/s",
        "value": value,
        "unit": "env-steps/s",
        "n_gpus": dist.get_world_size() if dist is not None else 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u64",
        "data": "synthetic (Philox fair-bit initial states; network exported from the reference's "
                "predictor_sets_200_5_kmeans.pkl)",
        "config": {
            "workload": "Bittner-200 async node update (R1 Graph.step), step mode: one update per env per "
                        "launch, state resident in device memory",
            "network": args.network, "n_nodes": net.n_nodes, "state_words": net.n_words,
            "batch_per_gpu": args.batch, "global_batch": world * args.batch, "updates_per_step": 1,
            "parallelism": f"dp{world} (env shards, no collective)", "rng": "philox4x32-10",
        },
    }


def main():
    args = parse()
    import atexit

    atexit.register(_census_at_exit)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    world, rank, local = dist_env()
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    import torch

    from gym_pbn_amd.shard import max_over_ranks, shard_for

    dist = None
    if world > 1:
        if not args.check_launch:
            _set_device(local)
        dist = _init_dist(args.dist_backend, args.dist_timeout)
    if args.check_launch:  # plumbing only: the N-rank path without GPU work
        if dist is not None:
            dist.barrier()
        t = max_over_ranks(float(rank), dist)
        if rank == 0:
            print(json.dumps({"check_launch": True, "n_gpus": dist.get_world_size() if dist else 1,
                              "max_over_ranks_of_rank": t, "value": None}), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    from gym_pbn_amd import _lib  # noqa: F401  (fails loudly when libpbnsim.so is missing)
    from gym_pbn_amd.batch import PBNBatch
    from gym_pbn_amd.network import load_network

    device = _set_device(local if world > 1 else 0)
    net = load_network(args.network)
    B = args.batch
    shard = shard_for(rank, world, B)  # contiguous global env ids; Philox keyed by global id

    if args.kernel_only:
        batch = PBNBatch(net, B, device=device, env_id_base=shard.env_base, seed=args.seed)
        batch.randomize()
        batch.step(args.warmup + args.steps)
        batch.sync()
        return

    # ---- --full: supplements first (every rank, so every GPU enters the headline in the same clock state)
    sup, floor, copy = {}, None, None
    if args.full:
        floor, copy = supplements(args, sup, net, B, world, rank, device, dist)

    # ---- the headline: W warm-up launches, then exactly K timed launches
    def barrier():
        if dist is not None:
            dist.barrier()

    batch = PBNBatch(net, B, device=device, env_id_base=shard.env_base, seed=args.seed)
    batch.randomize()
    batch.step(args.warmup)
    batch.prepare_steps(args.steps)  # setup, nothing runs (graph capture where the batch uses graphs)
    batch.sync()
    # no idle gap before the timed launches: a 5 ms sleep added ~0.4 us per timed launch to the wall
    # clock, a 0.2 ms busy wait ~0.2 us (tools/timing_window.py); the host syncs below still leave the
    # timed run a gap of its own in a kernel trace (tools/trace_split.py). No instrumentation inside
    # the window: the kernel time comes from an identical twin window right after it (below)
    _sync()
    barrier()
    _sync()
    t0 = time.perf_counter()
    batch.step(args.steps)
    _sync()  # device-wide: covers the batch's own stream (a stream sync first cost ~0.25 us/launch)
    t1 = time.perf_counter()
    barrier()
    elapsed = max_over_ranks(t1 - t0, dist, device=_dev(device))
    # host copy (after the window) for --dump-outputs and --full's shard self-check below
    final_state = batch.get_state() if (args.full or args.dump_outputs) else None
    batch.close()
    total_steps = world * B * args.steps
    value = total_steps / elapsed
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, final_state, net.n_nodes, shard.env_base, rank, world)
    if not args.full:  # the plain run ends here: the headline alone
        ranks = per_rank({"rank": rank, "elapsed_s": t1 - t0, "device": device}, dist)
        if rank == 0:
            print(json.dumps({
                **headline_line(args, net, world, dist, value, elapsed),
                "node_updates_per_s": value,
                "dist": {"backend": dist.get_backend() if dist is not None else None,
                         "world_size": dist.get_world_size() if dist is not None else 1, "per_rank": ranks},
                "process_census": process_census()}), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    # kernel time of the same window: a twin batch (same network, seed and env ids: the identical
    # Philox trajectory, so the same envs change and are written back per launch) runs the same W
    # warm-up launches, then the same K launches inside one HIP-event region on its stream
    twin = PBNBatch(net, B, device=device, env_id_base=shard.env_base, seed=args.seed)
    twin.randomize()
    twin.step(args.warmup)
    twin.prepare_steps(args.steps)
    twin.sync()
    _sync()
    twin.timing(2)
    twin.step(args.steps)
    twin.timing(0)
    _sync()
    local_kernel_ms, launches = twin.timing_read()
    kernel_ms = max_over_ranks(local_kernel_ms, dist, device=_dev(device))
    twin.close()

    # the bytes the timed launches had to move: the fraction of envs written back per launch over
    # exactly the timed window (twin batch), then the memory floor of that pattern in the same
    # clock state (32 B read per env, the changed envs' 32 B written back, no compute)
    q = window_changed_fraction(net, B, device, args.seed, shard.env_base, args.warmup, args.steps) \
        if rank == 0 else None
    # sharded-run self-check (every rank; collectives inside): sampled global ids re-run on their own
    check = guarded(step_shard_check, net, final_state, device, args.seed, shard.env_base, B, world * B,
                    args.warmup + args.steps, dist)
    del final_state
    ranks = per_rank({"rank": rank, "kernel_us": local_kernel_ms * 1e3 / max(launches, 1),
                      "elapsed_s": t1 - t0, "device": device}, dist)
    floor_us = None
    if floor is not None and q is not None:
        try:
            floor_us = floor.us_per_launch(B, round(100 * q), max(args.steps, 200))
        except RuntimeError:
            floor_us = None

    W = net.n_words
    contract_bytes = 16 * W * B  # read + write the packed state of every env
    avg_kernel_s = kernel_ms / 1e3 / max(launches, 1)
    traffic, pmc_src = read_pmc(args.pmc_file, f"{args.network}:{B}")
    if rank == 0:
        alg_bytes = min_bytes(W, B, q)
        achieved = alg_bytes / avg_kernel_s / 1e9 if launches else None
        kernel_us = avg_kernel_s * 1e6 if launches else None
        floor_GBs = alg_bytes / (floor_us / 1e6) / 1e9 if floor_us else None
        rf = {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": (achieved / HBM_PEAK_GBS) if achieved else None,
            "traffic": traffic,
            "kernel": f"pbn::k_step<{W},1,1,0,1024> (predictor mix, dirty store, Philox, 1024-thread groups)",
            "alg_bytes_per_launch": alg_bytes,
            "alg_bytes_rule": "8W B read per env + 8W B written per env whose updated bit changed "
                              "(changed_env_frac, measured over the timed window on a twin batch)",
            "changed_env_frac": q,
            "avg_kernel_us": kernel_us,
            "timing": "HIP events over the same K launches of a twin batch (same seed and env ids: the identical "
                      "trajectory) right after the timed window; the timed window itself carries no events",
            "residency": "the 32 MiB state stays in the 256 MiB Infinity Cache (MALL) and the XCDs' L2 between "
                         "launches; the HBM-bound figure is hbm_8m",
            "peak_source": "MI355X HBM3E spec, 8 TB/s (MI355X_MICROARCH.md): a fixed hardware ceiling; the 32 MiB "
                           "state is MALL-resident, and the measured ceiling of this access pattern is floor_GBs",
            "floor_us": floor_us,
            "floor_GBs": floor_GBs,
            "frac_of_floor": (floor_us / kernel_us) if (floor_us and kernel_us) else None,
            "frac_of_floor_note": "kernel floor / kernel time: the probe-relative figure (changes with the probe's "
                                  "run); frac is against the fixed 8 TB/s spec",
            "floor_source": "tools/mall_probe.hip run live after the timed launches: the same launch shape "
                            "(1024-thread groups, 2 per CU, env pairs), 32 B read per env, changed_env_frac of the "
                            "envs (drawn afresh per launch) written back, no compute",
            "reference_rates": {
                "guide_mall_gather_GBs": MALL_PEAK_GBS,
                "guide_mall_gather_note": "MI355X_MICROARCH.md Indexed rows: a READ-ONLY random-row gather into LDS "
                                          "from the Infinity Cache -- not a read+write ceiling (writes measure ~4 TB/s)",
                "frac_of_guide_mall_gather": (achieved / MALL_PEAK_GBS) if achieved else None,
                "hbm_spec_GBs": HBM_PEAK_GBS},
            "contract_accounting": {
                "bytes_per_launch": contract_bytes,
                "GBs": contract_bytes / avg_kernel_s / 1e9 if launches else None,
                "note": "SURVEY 8(d) prices 16W B per update (every env written back); the kernel writes only the "
                        "envs whose bit changed, so this is accounting, not moved bytes"},
            "traffic_source": pmc_src,
            "traffic_GBs": (traffic / avg_kernel_s / 1e9) if (traffic and launches) else None,
            "traffic_over_alg": (traffic / alg_bytes) if traffic else None,
            "traffic_window": read_pmc_window(args.pmc_file, f"{args.network}:{B}"),
            "timed_window": [args.warmup, args.warmup + args.steps],
        }
        bm = sup.get("beyond_mall_8m")
        if bm and "error" not in bm:
            rf["hbm_8m"] = {k: bm.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic",
                                                   "traffic_frac", "avg_kernel_us", "changed_env_frac",
                                                   "alg_bytes_per_launch", "floor_us", "frac_of_floor",
                                                   "traffic_over_alg", "traffic_window", "timed_window")}
        if isinstance(copy, float):
            rf["achievable_copy_GBs"] = copy
            rf["achievable_copy_source"] = "torch device-to-device copy of 2 GiB (past the MALL), read + write bytes"
        out = {
            **headline_line(args, net, world, dist, value, elapsed),
            "roofline": rf,
            "node_updates_per_s": value,
            "dist": {"backend": dist.get_backend() if dist is not None else None,
                     "world_size": dist.get_world_size() if dist is not None else 1, "per_rank": ranks},
            "shard_check": check,
            "order": "supplements (rollout, config 2, 8M past-MALL, config 5, MT mode) ran before the headline",
            **sup,
        }
        if world == 1 and not args.no_cpu_baseline:  # the host-core baseline: rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(net, args.cpu_seconds)
        out["process_census"] = process_census()
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
