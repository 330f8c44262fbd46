"""Case tables of the R6 env-step tests, shared by the test modules that run them (a plain module, not a
conftest: ``from r6_cases import ...``).

* ``ENV_VARIANT_CASES`` / ``env_variant_setup``: every k_env variant (kernel images 0, 1, 2 and 4, group mode,
  tail thresholds, lanes per wave) -- the table of ``test_env_kernel_variants_match_oracle``.
* ``FORCED_TAIL_CASES`` / ``forced_tail_knobs`` / ``long_first_step_actions``: the shapes in which the tail
  hand-off, the tail helpers and the grid pool must happen -- ``test_tail_handoff_forced_happens_and_matches_oracle``.
"""

import zlib
from types import SimpleNamespace

import numpy as np

from gym_pbn_amd.network import load_network

ENV_VARIANT_CASES = ["b28_gen_cap", "b28_h8_gen", "b199_h6_gen_first_tested", "b28_h12_general",
                     "b199_nogen", "tt200_fast", "syn500_gen",
                     "syn300_wide_cube", "b28_first_tested", "b28_h12_first_tested",
                     "tt200_first_tested", "b199_grp2", "b199_grp4", "b199_grp8", "b28_grp4_cap",
                     "b28_grp8_first_tested", "b28_grp2_h8", "b199_grp4_long",
                     "b28_gen_cap41", "b199_gen_long", "b199_gen_long_first_tested",
                     "b28_gen_cap41_tail32", "b199_gen_long_tail32", "b199_gen_long_tail16",
                     "b199_gen_long_tail8", "b199_gen_long_tail1", "b199_gen_long_first_tested_tail32",
                     "b28_first_tested_tail32", "b28_gen_cap41_tail3", "b199_gen_long_tail0",
                     "b199_gen_long_lanes16", "b199_gen_long_lanes1", "b28_gen_cap41_lanes4",
                     "b199_gen_long_first_tested_lanes8"]


def random_cubes(rng, N, H, n_care):
    cubes = []
    for _ in range(H):
        c = ["*"] * N
        for j in rng.choice(N, size=n_care, replace=False):
            c[int(j)] = int(rng.integers(0, 2))
        cubes.append(tuple(c))
    return cubes


def env_variant_setup(case, monkeypatch):
    """Sets the case's PBNSIM_ENV_* knobs and returns its inputs: ``case`` (the base case, knob suffixes
    stripped), ``net``, ``attractors``, ``cap``, ``first`` (first_update_tested), ``A``, ``B`` and ``rng`` (the
    case's generator, already advanced past the cubes: the test draws its actions from it).

    ``_tailK``: the cooperative-draw kernel's tail mode (a wave whose queue ran dry resolves its envs one at a
    time, 64 updates per block) from K live envs per wave (32: early, many envs queued behind the one resolved;
    1: the last env only; 0: never; the default is ENV_TAIL_DEFAULT)."""
    from gym_pbn_amd.network import PredictorNetwork, synthetic_predictor_sets

    if "_tail" in case:  # the same inputs as the base case, another tail-mode threshold
        monkeypatch.setenv("PBNSIM_ENV_TAIL", case.split("_tail")[1])
        case = case.split("_tail")[0]
    # lane mode proper (every lane takes envs) unless the case names K lanes per wave taking envs
    # (tail mode from the first env; batches this small default to K = 1)
    monkeypatch.setenv("PBNSIM_ENV_LANES", "64")
    if "_lanes" in case:
        monkeypatch.setenv("PBNSIM_ENV_LANES", case.split("_lanes")[1])
        case = case.split("_lanes")[0]
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    cap, A, B = 3000, 3, 1024
    first = case.endswith("first_tested")  # PBNTargetEnv.step(force=False) semantics
    # k_env_grp (G lanes per env, blocks of G updates resolved in parallel) or lane mode (1)
    monkeypatch.setenv("PBNSIM_ENV_GROUP", case.split("_grp")[1][0] if "_grp" in case else "1")
    if case.startswith("b199_grp") or case.startswith("b199_gen_long"):
        net = load_network("bittner199")
    elif case.startswith("b28"):
        net = load_network("bittner28")
    elif case == "b199_h6_gen_first_tested":
        net = load_network("bittner199")
    elif case == "b199_nogen":
        net = load_network("bittner199")
        monkeypatch.setenv("PBNSIM_ENV_NO_GEN", "1")
    elif case.startswith("tt200"):
        net = load_network("tt200")
    else:
        n = 500 if case == "syn500_gen" else 300
        net = PredictorNetwork.from_predictor_sets(*synthetic_predictor_sets(n, 4, seed=n), name=f"syn{n}")
    N = net.n_nodes
    if case in ("b28_gen_cap", "b28_grp4_cap", "b28_gen_cap41"):
        cap = 41 if ("grp" in case or "cap41" in case) else 40  # not a multiple of the group size
        attractors = [random_cubes(rng, N, 2, 5), random_cubes(rng, N, 2, 5)]
    elif case.startswith("b199_gen_long"):  # long loops: thousands of updates per env step
        cap = 2001
        attractors = [random_cubes(rng, N, 2, 12), random_cubes(rng, N, 2, 4)]
    elif case == "b199_grp4_long":  # long until-attractor loops, many capped envs
        cap = 2001
        attractors = [random_cubes(rng, N, 4, 12), random_cubes(rng, N, 2, 4)]
    elif case in ("b28_grp2_h8", "b28_h8_gen"):  # 8 cubes: the most the byte counters hold
        attractors = [random_cubes(rng, N, 4, 4), random_cubes(rng, N, 4, 4)]
    elif case == "b199_h6_gen_first_tested":  # 5..8 cubes: both packed counter words
        attractors = [random_cubes(rng, N, 3, 3), random_cubes(rng, N, 3, 3)]
    elif case.startswith("b28_h12"):
        attractors = [random_cubes(rng, N, 6, 4), random_cubes(rng, N, 6, 4)]
    elif case == "syn300_wide_cube":  # one cube caring about 260 > 255 nodes: general matching
        attractors = [random_cubes(rng, N, 1, 260) + random_cubes(rng, N, 2, 3), random_cubes(rng, N, 1, 3)]
    else:
        attractors = [random_cubes(rng, N, 2, 4), random_cubes(rng, N, 2, 4)]
    return SimpleNamespace(case=case, net=net, attractors=attractors, cap=cap, first=first, A=A, B=B, rng=rng)


FORCED_TAIL_CASES = ["handoff", "helpers", "helpers_off", "grid", "grid_off"]


def forced_tail_knobs(case, monkeypatch):
    """The knobs of one forced tail case; returns its batch size (see the test's docstring for the shapes)."""
    grid_case = case.startswith("grid")
    monkeypatch.setenv("PBNSIM_ENV_LANES", "16" if grid_case else "2")
    monkeypatch.setenv("PBNSIM_ENV_GRID", "2" if grid_case else "1")
    if case == "helpers_off":
        monkeypatch.setenv("PBNSIM_ENV_HELPERS", "0")
    if case == "grid_off":
        monkeypatch.setenv("PBNSIM_ENV_GRID_STEAL", "0")
    return {"handoff": 6, "grid": 16, "grid_off": 16}.get(case, 2)


def tail_actions(rng, shape, N):
    a = rng.integers(1, N + 1, size=shape).astype(np.int32)
    a[rng.random(shape) < 0.75] = 0
    return a


def long_first_step_actions(o, cfgd, st, ns, N, shape, seed, base, cap, call_idx=0):
    """Action rows ``shape`` = (T, B, A) whose first env step is long for every env: per env, the first
    candidate row (tried on the oracle, Philox call index ``call_idx``) that runs >= 2,048 updates."""
    T, B, A = shape
    acts = tail_actions(np.random.default_rng(77), (T, B, A), N)
    rng = np.random.default_rng(78)
    need = np.ones(B, bool)
    for _ in range(400):
        cand = tail_actions(rng, (B, A), N)
        r = o.env_step_multi(cfgd, st, ns, cand, seed=seed, env_base=base, call_idx=call_idx, update_cap=cap)
        ok = need & (r["n_updates"] >= 2048)
        acts[0][ok] = cand[ok]
        need &= ~ok
        if not need.any():
            break
    assert not need.any()
    return acts
