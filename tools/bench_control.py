#!/usr/bin/env python3
"""Value iteration over a transition graph: what one Bellman sweep costs fused, in torch ops and on the host.
Measurement only; no threshold.

Workload: ``synthetic_truth_table_pbn(21, 3, seed=0)`` under ``table_graph="step"``, all 2**20 states with node 0
clear, 16 random target states, ``gamma = 0.99``, the literals 20 / 4 / 1 of ``PBN-v0``.

Three ways to make one sweep ``V -> V'`` on the same arrays (``mass``, ``succ``, ``nbr``, ``nT``), each checked against
the others before any number is written:
  fused   ``ControlProblem``'s sweep: three small torch ops on ``[S]`` for ``h``, ``k_stg_expect``, ``k_stg_backup``;
  torch   the same sweep in torch ops, as a user could write it without the kernels: ``TransitionGraph.pull(h)`` (which
          recomputes ``probabilities()``), ``Ua = U - k nT``, a gather of ``Ua`` through ``nbr``, a masked row max;
  host    ``host_backup`` in numpy.
Per device variant: REPS runs of SWEEPS sweeps after a warm-up run, timed with device events and with a wall clock
around the run and a device synchronise; the per-sweep time is the run's over SWEEPS; median and spread (max - min).
bytes_per_sweep = S * N * (8 + 4 + 4): ``mass``, ``succ`` and ``nbr`` streamed once; the two 8-byte gathers per cell
into ``[S]`` arrays (8 MiB, cache-resident) are not counted. ``share_of_hbm_spec`` is those bytes over the device time
over 8 TB/s (the datasheet rate), a lower bound on what the fused sweep moves, not a kernel's share of peak.
``fused_parts`` times the fused sweep's three parts alone, the same way (``h``'s three torch ops, ``k_stg_expect``,
``k_stg_backup``). One ``solve(tol=1e-9)`` is timed whole. Results go to profiles/control.json.
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
HOST_RUNS = 3
N_NODES = 21
N_TARGET = 16
GAMMA = 0.99
HBM_SPEC_BYTES_PER_S = 8e12


def summary(values):
    return {"runs": values, "median": statistics.median(values), "spread": max(values) - min(values)}


def torch_sweep(p, v):
    """One sweep in torch ops on the problem's arrays: ``(v_new, policy)``."""
    import torch

    h = torch.where(p.target, p._r, v * p.gamma - p.step_cost)
    u = p.graph.pull(h)
    ua = u - p.action_cost * p.n_t
    q = torch.where(p.nbr >= 0, ua[p.nbr.clamp(min=0).long()], torch.full((), float("-inf"), dtype=torch.float64,
                                                                          device=v.device))
    best, node = q.max(dim=1)
    flip = best > u
    return torch.where(flip, best, u), torch.where(flip, node, torch.full_like(node, -1)).to(torch.int32)


def time_runs(run):
    """REPS timed calls of ``run()`` (SWEEPS sweeps each) after one warm-up call: per-sweep seconds."""
    import torch

    run()
    wall, dev = [], []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / SWEEPS)
        dev.append(e0.elapsed_time(e1) * 1e-3 / SWEEPS)
    return {"wall_s": summary(wall), "device_s": summary(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "control.json"))
    ap.add_argument("--nodes", type=int, default=N_NODES, help="network size (the default is the measured workload)")
    args = ap.parse_args()
    import numpy as np
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.control import ControlProblem, host_backup
    from gym_pbn_amd.network import TruthTableNetwork, synthetic_truth_table_pbn
    from gym_pbn_amd.transition import TransitionGraph

    assert _lib.device_count() >= 1, "bench_control.py measures on a GPU"
    N = args.nodes
    S = 1 << (N - 1)
    net = TruthTableNetwork.from_pbn_data(synthetic_truth_table_pbn(N, 3, 0))
    states = (np.arange(S, dtype=np.uint64) << np.uint64(1)).reshape(-1, 1)
    t0 = time.perf_counter()
    g = TransitionGraph(net, states, table_graph="step")
    assert g.closed
    target = np.zeros(S, dtype=bool)
    target[np.random.default_rng(0).choice(S, size=N_TARGET, replace=False)] = True
    p = ControlProblem(g, target, gamma=GAMMA, strict=True)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0

    # the three sweeps agree, from a start that is no fixed point
    v0 = torch.from_numpy(np.random.default_rng(1).uniform(-50.0, 20.0, size=S)).to(p.device)
    vf, pf = p.backup(v0)
    vt, pt = torch_sweep(p, v0)
    mass, succ, nbr = g.mass.cpu().numpy(), g.succ.cpu().numpy(), p.nbr.cpu().numpy()
    n_t = p.n_t.cpu().numpy()
    host = []
    for _ in range(HOST_RUNS):
        t0 = time.perf_counter()
        vh, ph = host_backup(mass, succ, nbr, g.n_movable, target, v0.cpu().numpy(), gamma=GAMMA, n_t=n_t)
        host.append(time.perf_counter() - t0)
    bound = (2 * N + 8) * 2.0 ** -53 * 80.0 * 2  # two expectations of |h| <= 80, first order (tests/test_control_host.py)
    dev_t = float((vf - vt).abs().max())
    dev_h = float(np.abs(vf.cpu().numpy() - vh).max())
    assert dev_t <= 4 * bound and dev_h <= 4 * bound, (dev_t, dev_h, bound)
    agree_t = float((pf == pt).double().mean())
    agree_h = float((pf.cpu().numpy() == ph).mean())
    del mass, succ, nbr, vh, ph, vt, pt

    a, b = v0.clone(), torch.empty_like(v0)
    pol = torch.empty(S, dtype=torch.int32, device=p.device)

    def fused():
        nonlocal a, b
        with g._on_default_stream(p.device):
            for _ in range(SWEEPS):
                p._backup_into(a, b, pol)
                a, b = b, a

    def in_torch():
        nonlocal a
        for _ in range(SWEEPS):
            a = torch_sweep(p, a)[0]

    def h_ops():
        for _ in range(SWEEPS):
            torch.mul(a, p.gamma, out=p._h)
            p._h.sub_(p.step_cost)
            torch.where(p.target, p._r, p._h, out=p._h)

    def expect_only():
        with g._on_default_stream(p.device):
            for _ in range(SWEEPS):
                g._expect_into(p._h, p._u, p.n_t, p.action_cost, p._ua)

    def backup_only():
        with g._on_default_stream(p.device):
            for _ in range(SWEEPS):
                _lib.check(_lib.lib.pbn_stg_backup_device(g.handle, p.nbr.data_ptr(), p._u.data_ptr(), p._ua.data_ptr(),
                                                          b.data_ptr(), pol.data_ptr()))

    fused_t = time_runs(fused)
    parts = {"h_torch_ops": time_runs(h_ops), "k_stg_expect": time_runs(expect_only),
             "k_stg_backup": time_runs(backup_only)}
    a = v0.clone()
    torch_t = time_runs(in_torch)
    del a, b

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol = p.solve(tol=1e-9)
    torch.cuda.synchronize()
    solve_s = time.perf_counter() - t0
    bytes_per_sweep = S * N * (8 + 4 + 4)
    fused_dev = fused_t["device_s"]["median"]
    result = {
        "workload": {"network": f"synthetic_truth_table_pbn({N}, 3, 0)", "table_graph": "step", "n_states": S,
                     "n_nodes": N, "n_target": N_TARGET, "gamma": GAMMA, "setup_s": setup_s},
        "reps": REPS, "sweeps_per_rep": SWEEPS, "host_runs": HOST_RUNS,
        "unit": "seconds per sweep: a run of sweeps_per_rep sweeps over sweeps_per_rep",
        "fused": fused_t, "fused_parts": parts, "torch": torch_t, "host_backup_s": summary(host),
        "torch_over_fused_device": torch_t["device_s"]["median"] / fused_dev,
        "torch_over_fused_wall": torch_t["wall_s"]["median"] / fused_t["wall_s"]["median"],
        "host_over_fused_wall": statistics.median(host) / fused_t["wall_s"]["median"],
        "bytes_per_sweep": bytes_per_sweep,
        "fused_bytes_per_s_device": bytes_per_sweep / fused_dev,
        "share_of_hbm_spec": bytes_per_sweep / fused_dev / HBM_SPEC_BYTES_PER_S,
        "agreement": {"max_abs_fused_minus_torch": dev_t, "max_abs_fused_minus_host": dev_h, "allowed": 4 * bound,
                      "policy_equal_torch": agree_t, "policy_equal_host": agree_h},
        "solve": {"tol": 1e-9, "sweeps": sol.iters, "residual": sol.residual, "seconds": solve_s,
                  "seconds_per_sweep": solve_s / sol.iters, "states_that_flip": int((sol.policy >= 0).sum()),
                  "v_min": float(sol.v.min()), "v_max": float(sol.v.max())},
    }
    print(json.dumps(result), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
