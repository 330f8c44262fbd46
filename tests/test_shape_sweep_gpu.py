"""Every kernel family at every state width ``W = 1 .. 8`` and every ``N % 64 == 0`` edge (GPU).

The families are compiled once per ``W`` (``by_words<8>``; the group kernels ``by_words<4>`` and ``N <= 256``)
and the rest of the suite reaches them only through the networks it happens to have. Here each family runs on
the 22 networks of ``shape_cases.py`` (predictor mix ``pm`` and truth table ``tt`` at
``N = 63 64 65 128 192 256 257 320 384 448 512``), bit-exact against the oracle -- which
``test_shape_sweep_host.py`` pins at these widths to an unpacked model and ``test_oracle.py`` to the reference.

Batches are small and odd (a partial wave and a second workgroup), update counts a few dozen. The trajectory
tests assert on the oracle's result that node ``N - 1`` and both sides of every word boundary move. A family
that refuses a shape is listed in ``shape_cases.EXPECTED_REFUSALS`` and asserted to refuse; none is skipped.
"""

import numpy as np
import pytest

from shape_cases import (EXPECTED_REFUSALS, KINDS, SHAPES, assert_edges_move, boundary_node, edge_actions,
                         edge_attractors, shape_net)

pytestmark = pytest.mark.gpu

CASES = [(k, n) for k in KINDS for n in SHAPES]
KNOBS = ("PBNSIM_STORE_MODE", "PBNSIM_ENVS_PER_THREAD", "PBNSIM_STEP_BLOCK", "PBNSIM_STEP_GRAPH",
         "PBNSIM_STEP_CHAINS", "PBNSIM_ROLL_GROUP", "PBNSIM_ENV_GROUP", "PBNSIM_ENV_NO_GEN", "PBNSIM_ENV_LANES",
         "PBNSIM_ENV_TAIL", "PBNSIM_MT_LANES", "PBNSIM_SSD_WAVE", "PBNSIM_SSD_SHARED", "PBNSIM_SSD_SERIAL")
B = 321  # 5 waves + 1 lane: a partial wave, a second 256-thread workgroup, an odd last lane pair
SEED = (3 << 32) | 17


@pytest.fixture(scope="module")
def G():
    from gym_pbn_amd import _lib, batch

    assert _lib.device_count() >= 1, "gpu tests need a HIP device"
    return batch


@pytest.fixture
def knobs(monkeypatch):
    """Sets exactly the given PBNSIM_* knobs (read once per batch, at its creation); the others are unset."""

    def set_(**kv):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kv.items():
            monkeypatch.setenv("PBNSIM_" + k, str(v))

    set_()
    return set_


_ORC = {}


def orc(oracle_mod, kind, N):
    if (kind, N) not in _ORC:
        _ORC[kind, N] = oracle_mod.Oracle(shape_net(kind, N))
    return _ORC[kind, N]


def refused(family, kind, N, call):
    """False for a shape the family takes (``call`` is not made). A shape listed in ``EXPECTED_REFUSALS`` is
    asserted to be refused by ``call`` with exactly the listed code; then True."""
    from gym_pbn_amd import _lib

    want = EXPECTED_REFUSALS.get((family, kind, N))
    if want is None:
        return False
    with pytest.raises(_lib.PbnError) as ei:
        call()
    assert ei.value.code == want[0], want
    return True


def flip_expected(oracle_mod, init, acts, offset, dedup):
    """Flips on unpacked rows with Python list indexing: (packed states, nodes changed in some env)."""
    want = init.copy()
    for e in range(len(acts)):
        row = acts[e].tolist()
        for a in (sorted(set(row)) if dedup else row):
            if a != 0:
                want[e, a - offset] ^= 1
    return oracle_mod.pack_bits(want), {int(i) for i in np.nonzero((want != init).any(axis=0))[0]}


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _sync():
    import torch

    torch.cuda.synchronize()


def _bit(i):
    return np.uint64(1) << np.uint64(i % 64)


# ------------------------------------------------------------------------------------------------ state I/O
@pytest.mark.parametrize("kind,N", CASES)
def test_state_io(G, oracle_mod, knobs, kind, N):
    """k_init, pbn_set_state's range check, k_unpack and k_flip (host and device actions)."""
    import torch

    net = shape_net(kind, N)
    o = orc(oracle_mod, kind, N)
    base = 2**33 + 5
    b = G.PBNBatch(net, B, seed=SEED, env_id_base=base)
    for rc in range(2):  # the reset counter is part of the draw
        b.randomize()
        init = b.get_state()
        assert np.array_equal(init, o.init_philox(B, seed=SEED, env_base=base, reset_count=rc)), rc
    top = (init[:, -1] >> np.uint64((N - 1) % 64)) & np.uint64(1)
    assert 0 < int(top.sum()) < B  # node N - 1 is drawn, both values
    # set_state: node N - 1 set is a state; bit N (N % 64 != 0) is not, and nothing is written
    st = init.copy()
    st[:, -1] |= _bit(N - 1)
    b.set_state(st)
    assert np.array_equal(b.get_state(), st)
    if N % 64:
        bad = st.copy()
        bad[B - 1, -1] |= _bit(N)
        with pytest.raises(ValueError):
            b.set_state(bad)
        assert np.array_equal(b.get_state(), st)
    # unpack on the device: the batch's state, and caller's words
    bits = torch.full((B, N), 7, dtype=torch.uint8, device="cuda:0")
    _sync()
    b.unpack_bits_device(bits.data_ptr())
    b.sync()
    want = ((st[:, np.arange(N) // 64] >> (np.arange(N) % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    assert np.array_equal(bits.cpu().numpy(), want)
    assert want[:, N - 1].all()
    words = _dev(init)
    _sync()
    b.unpack_bits_device(bits.data_ptr(), words.data_ptr())
    b.sync()
    assert np.array_equal(bits.cpu().numpy(), oracle_mod.unpack_bits(init, N))
    # flips: nodes 0, 63, 64 and N - 1 by both offsets, duplicates with and without dedup
    rng = np.random.default_rng(N)
    for offset in (1, 0):
        for dedup in (True, False):
            for device in (False, True):
                acts = edge_actions(rng, B, 3, N, offset)
                b.set_state(init)
                if device:
                    d = _dev(acts)
                    _sync()
                    b.flip_device(d.data_ptr(), 3, offset=offset, dedup=dedup)
                else:
                    b.flip(acts, offset=offset, dedup=dedup)
                want, hit = flip_expected(oracle_mod, oracle_mod.unpack_bits(init, N), acts, offset, dedup)
                assert np.array_equal(b.get_state(), want), (offset, dedup, device)
                if dedup:  # (without it the duplicated actions flip twice)
                    assert {n for n in (0, 63, 64, N - 1) if 1 - offset <= n < N} <= hit, (offset, hit)
    # the first value out of range on either side: the host call changes nothing, the device call skips the row
    for offset in (1, 0):
        for v in (N + offset, -N - 1 + offset):
            acts = np.zeros((B, 3), np.int32)
            acts[:, 0] = N - 1 + offset  # every other row flips node N - 1
            acts[B - 2, 2] = v
            b.set_state(init)
            with pytest.raises(ValueError):
                b.flip(acts, offset=offset)
            assert np.array_equal(b.get_state(), init)
            d = _dev(acts)
            _sync()
            with pytest.raises(ValueError):
                b.flip_device(d.data_ptr(), 3, offset=offset)
            want = init.copy()
            want[:, -1] ^= _bit(N - 1)
            want[B - 2] = init[B - 2]
            assert np.array_equal(b.get_state(), want), (offset, v)
            acts[B - 2, 2] = v - 1 if v > 0 else v + 1  # the last value in range: node N - 1 again / node 0
            b.set_state(init)
            b.flip(acts, offset=offset)
            assert np.array_equal(b.get_state(), flip_expected(oracle_mod, oracle_mod.unpack_bits(init, N), acts,
                                                               offset, True)[0]), (offset, v)
    b.close()


# ---------------------------------------------------------------------------------------------- step family
# A covering set: every value of every knob meets every W (each row runs on all 22 networks, with an even and an
# odd env id base: lane pairs sharing a Philox call / one call per env); not every combination.
STEP_KNOBS = {
    "default": {},
    "full-ept1-256-plain": dict(STORE_MODE=0, ENVS_PER_THREAD=1, STEP_BLOCK=256, STEP_GRAPH=0),
    "dirty-ept2-1024-graph": dict(STORE_MODE=1, ENVS_PER_THREAD=2, STEP_BLOCK=1024, STEP_GRAPH=1),
    "half-ept1-1024-plain": dict(STORE_MODE=2, ENVS_PER_THREAD=1, STEP_BLOCK=1024, STEP_GRAPH=0),
    "half-ept2-1024-graph": dict(STORE_MODE=2, ENVS_PER_THREAD=2, STEP_BLOCK=1024, STEP_GRAPH=1),
    "dirty-ept2-256-graph": dict(STORE_MODE=1, ENVS_PER_THREAD=2, STEP_BLOCK=256, STEP_GRAPH=1),
}
T = 48
_STEP_REF = {}


def step_reference(oracle_mod, kind, N, base):
    """Computed once per (network, base), read-only: init, forced nodes, replay draws and the oracle's states after
    step(T), rollout(T), step_forced(5) and step_replay(6)."""
    key = (kind, N, base)
    if key not in _STEP_REF:
        o = orc(oracle_mod, kind, N)
        rng = np.random.default_rng(N + base)
        lo = 1 if kind == "tt" else 0
        init = o.init_philox(B, seed=SEED, env_base=base)
        s1 = o.step_philox(init, SEED, base, 0, T)
        s2 = o.step_philox(s1, SEED, base, T, T)
        forced = rng.integers(lo, N, size=(5, B)).astype(np.uint32)
        forced[0, :3] = [N - 1, min(64, N - 1), 63 if N > 63 else N - 2]
        s3 = o.step_forced(s2, forced, SEED, base, 2 * T)
        ni = rng.integers(lo, N, size=(6, B)).astype(np.uint32)
        ni[0, :3] = [N - 1, min(64, N - 1), 63 if N > 63 else N - 2]
        k53 = rng.integers(0, 1 << 53, size=(6, B), dtype=np.uint64)
        s4 = o.step_replay(s3, ni, k53)
        assert_edges_move(init, s1, N, kind)
        assert_edges_move(s1, s2, N, kind)
        for a in (init, s1, s2, s3, s4, forced, ni, k53):
            a.setflags(write=False)
        _STEP_REF[key] = (init, s1, s2, forced, s3, ni, k53, s4)
    return _STEP_REF[key]


@pytest.mark.parametrize("kind,N", CASES)
@pytest.mark.parametrize("knob", list(STEP_KNOBS))
def test_step_family(G, oracle_mod, knobs, knob, kind, N):
    """k_step (T launches of one update: the write-back under test), k_rollout, the forced and the replay
    kernels on one update counter. ``half``: the changed 16-B half of an env (W even and >= 4: N = 256, 384, 512
    take store_changed's granule select; the others its whole-env branch)."""
    knobs(**STEP_KNOBS[knob])
    net = shape_net(kind, N)
    for base in (77, 64):
        init, s1, s2, forced, s3, ni, k53, s4 = step_reference(oracle_mod, kind, N, base)
        b = G.PBNBatch(net, B, seed=SEED, env_id_base=base)
        b.set_state(init)
        b.step(T)
        assert np.array_equal(b.get_state(), s1), base
        b.rollout(T)
        assert np.array_equal(b.get_state(), s2), base
        b.step_forced(forced)
        assert np.array_equal(b.get_state(), s3), base
        b.step_replay(ni, k53)
        assert np.array_equal(b.get_state(), s4), base
        assert b.info()["update_count"] == 2 * T + 5  # (replayed draws are the caller's: no counter)
        b.close()


# --------------------------------------------------------------------------------------------- R6 env pieces
def env_setup(N, first=False):
    """Host side of an env case: attractors, the oracle's config (cubes packed here) and three action rows."""
    from gym_pbn_amd.batch import cube_arrays

    rng = np.random.default_rng(2000 + N)
    attractors = edge_attractors(rng, N)
    care, value = cube_arrays([c for a in attractors for c in a], N)
    rcare, rvalue = cube_arrays(attractors[0], N)
    cfgd = dict(care=care, value=value, target_care=care[2], target_value=value[2], reset_care=rcare,
                reset_value=rvalue, horizon=2, first_tested=first)
    for f in (N - 1, boundary_node(N), boundary_node(N) + 1):  # the cubes care about the edges
        assert (int(np.bitwise_or.reduce(care, axis=0)[f // 64]) >> (f % 64)) & 1
    acts = np.stack([edge_actions(rng, B, 3, N) for _ in range(3)])
    return attractors, cfgd, acts


CAP = 300
_ENV_REF = {}


def env_reference(oracle_mod, kind, N, cfgd, acts, first, base):
    """The oracle's reset and three env steps, computed once per case, read-only."""
    key = (kind, N, first, base)
    if key not in _ENV_REF:
        o = orc(oracle_mod, kind, N)
        st, ns = o.env_reset_philox(np.zeros((B, o.W), np.uint64), np.ones(B, np.int64), cfgd["reset_care"],
                                    cfgd["reset_value"], seed=SEED, env_base=base, reset_count=0)
        refs = []
        for call in range(3):
            r = o.env_step_multi(cfgd, refs[-1]["state"] if refs else st, refs[-1]["n_steps"] if refs else ns,
                                 acts[call], seed=SEED, env_base=base, call_idx=call, update_cap=CAP)
            refs.append(r)
        assert_edges_move(st, refs[-1]["state"], N, kind)
        flags = np.concatenate([r["flags"] for r in refs])
        assert (flags & 2).any() and (flags & 4).any() and not (flags & 4).all()  # truncated; capped and not
        assert (refs[0]["n_updates"] > 1).any()  # real until-attractor loops
        _ENV_REF[key] = (st, ns, refs)
    return _ENV_REF[key]


def run_env_steps(G, oracle_mod, kind, N, first=False, base=1001, fused=False):
    """env_reset and three env steps of a fresh batch against the oracle; returns the batch's info()."""
    import torch

    attractors, cfgd, acts = env_setup(N, first)
    st, ns, refs = env_reference(oracle_mod, kind, N, cfgd, acts, first, base)
    gnet = G.Net(shape_net(kind, N))
    cfg = G.EnvConfig(gnet, attractors, horizon=2, first_update_tested=first)
    assert np.array_equal(cfg.cube_care, cfgd["care"]) and np.array_equal(cfg.target_value, cfgd["target_value"])
    W = gnet.n_words
    b = G.PBNBatch(gnet, B, seed=SEED, env_id_base=base)
    b.env_reset(cfg)
    assert np.array_equal(b.get_state(), st) and np.array_equal(b.get_n_steps(), ns)
    if fused:  # one launch for the three env steps
        d_acts = _dev(acts)
        o_ = torch.zeros((3, B, W), dtype=torch.int64, device="cuda:0")
        r_ = torch.zeros((3, B), dtype=torch.int32, device="cuda:0")
        f_ = torch.zeros((3, B), dtype=torch.uint8, device="cuda:0")
        n_ = torch.zeros((3, B), dtype=torch.int32, device="cuda:0")
        _sync()
        b.env_rollout_multi_device(cfg, 3, d_acts.data_ptr(), 3, o_.data_ptr(), r_.data_ptr(), f_.data_ptr(),
                                   n_.data_ptr(), update_cap=CAP)
        b.sync()
        outs = [(o_[t].cpu().numpy().view(np.uint64), r_[t].cpu().numpy(), f_[t].cpu().numpy(),
                 n_[t].cpu().numpy().view(np.uint32)) for t in range(3)]
    for call in range(3):
        obs, rew, flags, nup = outs[call] if fused else b.env_step_multi(cfg, acts[call], update_cap=CAP)
        ref = refs[call]
        assert np.array_equal(nup, ref["n_updates"]), call
        assert np.array_equal(obs, ref["obs"]) and np.array_equal(rew, ref["reward"]), call
        assert np.array_equal(flags, ref["flags"]), call
        if not fused:
            assert np.array_equal(b.get_state(), ref["state"]), call
            assert np.array_equal(b.get_n_steps(), ref["n_steps"]), call
    assert np.array_equal(b.get_state(), refs[-1]["state"]) and np.array_equal(b.get_n_steps(), refs[-1]["n_steps"])
    info = b.info()
    b.close()
    return info


ENV_VARIANTS = {"default": {}, "nogen": dict(ENV_NO_GEN=1), "lanes64": dict(ENV_LANES=64),
                "first-tested": {}, "fused": {}}


@pytest.mark.parametrize("kind,N", CASES)
@pytest.mark.parametrize("variant", list(ENV_VARIANTS))
def test_env_reset_and_step(G, oracle_mod, knobs, variant, kind, N):
    """k_init's reset path and k_env: the default image, without cooperative draws, lane mode proper, with the
    first update tested, and the three env steps as one fused launch."""
    knobs(**ENV_VARIANTS[variant])
    info = run_env_steps(G, oracle_mod, kind, N, first=variant == "first-tested", fused=variant == "fused")
    assert info["env_call_count"] == 3
    if variant == "lanes64" and kind == "pm" and info["env_kernel"] == 4:
        assert info["env_lane_limit"] == 64


# -------------------------------------------------------------------------------------------- group kernels
@pytest.mark.parametrize("kind,N", CASES)
@pytest.mark.parametrize("group", [2, 4, 8])
def test_group_kernels(G, oracle_mod, knobs, group, kind, N):
    """k_rollout_grp and k_env_grp (G lanes per env): predictor mix with N <= 256 (byte-packed node lists,
    ``by_words<4>``) really runs them; N = 257 and up, and every truth-table shape, reports lane mode and still
    matches. Update counts that are no multiple of G."""
    knobs(ROLL_GROUP=group, ENV_GROUP=group, ENV_LANES=64)
    lanes = group if kind == "pm" and N <= 256 else 1
    init, s1, s2 = step_reference(oracle_mod, kind, N, 77)[:3]
    b = G.PBNBatch(shape_net(kind, N), B, seed=SEED, env_id_base=77)
    assert b.info()["roll_lanes"] == lanes
    b.set_state(init)
    b.rollout(T - 11)
    b.rollout(11)
    assert np.array_equal(b.get_state(), s1)
    b.rollout(T)
    assert np.array_equal(b.get_state(), s2)
    b.close()
    assert run_env_steps(G, oracle_mod, kind, N)["env_lanes"] == lanes


# -------------------------------------------------------------------------------------------------- MT mode
@pytest.mark.parametrize("kind,N,walk", [("pm", n, w) for n in SHAPES for w in ("staged", "lanes")]
                         + [("tt", n, "tt") for n in SHAPES])
def test_mt_mode(G, oracle_mod, knobs, kind, N, walk):
    """k_mt_staged / k_mt_step / the truth-table walk: genRandState / reset from the seed, then 40 + 9 updates."""
    knobs(MT_LANES=1 if walk == "lanes" else 0)
    net = shape_net(kind, N)
    o = orc(oracle_mod, kind, N)
    seeds = np.random.default_rng(N).integers(0, 2**32 if kind == "tt" else 2**63, size=B, dtype=np.uint64)
    b = G.PBNBatch(net, B)
    if refused("mt", kind, N, lambda: b.mt_seed(seeds, init_state=True)):
        return
    b.mt_seed(seeds, init_state=True)
    init = o.run_mt(seeds, 0)
    assert np.array_equal(b.get_state(), init)
    b.mt_step(40)
    b.mt_step(9)
    want = o.run_mt(seeds, 49)
    assert_edges_move(init, want, N, kind)
    assert np.array_equal(b.get_state(), want)
    b.close()


# ----------------------------------------------------------------------------------------- synchronous step
@pytest.mark.parametrize("kind,N", CASES)
def test_sync_step(G, oracle_mod, knobs, kind, N):
    """k_sync without perturbations and with p = 0.7 / N, where a step perturbs in about half of the envs and
    updates in the others (both asserted on the oracle: with and without perturbations it agrees on some envs'
    first step and differs on others)."""
    net = shape_net(kind, N)
    o = orc(oracle_mod, kind, N)
    init = o.init_philox(B, seed=SEED, env_base=11)
    for p in (0.0, 0.7 / N):
        gap = G.flip_gap_table(N, p)
        b = G.PBNBatch(net, B, seed=SEED, env_id_base=11)
        b.set_state(init)
        if refused("sync", kind, N, lambda: b.synch_step(1, p)):
            return
        b.synch_step(5, p)
        b.synch_step(2, p)  # the step counter continues
        ref = oracle_mod.sync_philox(o, init, SEED, 11, 0, 5, gap)
        ref = oracle_mod.sync_philox(o, ref, SEED, 11, 5, 2, gap)
        if p:
            one, plain = (oracle_mod.sync_philox(o, init, SEED, 11, 0, 1, g) for g in (gap, None))
            same = (one == plain).all(axis=1)
            assert 0 < int(same.sum()) < B
        else:
            assert_edges_move(init, ref, N, "pm")  # the synchronous step updates node 0 of tables too
        assert np.array_equal(b.get_state(), ref), p
        b.close()


# ------------------------------------------------------------------------------------------------------ SSD
@pytest.mark.parametrize("kind,N", CASES)
@pytest.mark.parametrize("mode", ["lane", "wave", "shared"])
def test_ssd(G, oracle_mod, knobs, mode, kind, N):
    """k_ssd in lane, wave and shared (four waves per env) mode: targets on node 0, a word-boundary node and
    node N - 1, flips with p = 0.01."""
    knobs(SSD_WAVE=0 if mode == "lane" else 1, SSD_SHARED=4 if mode == "shared" else 0, SSD_SERIAL=0)
    net = shape_net(kind, N)
    o = orc(oracle_mod, kind, N)
    targets, iters, p = [0, boundary_node(N), N - 1], 70, 0.01
    Bs = 129
    b = G.PBNBatch(net, Bs, seed=SEED, env_id_base=5)
    b.randomize()
    s0 = b.get_state()
    if refused("ssd_" + mode, kind, N, lambda: b.ssd_counts(targets, 1, p)):
        return
    h1 = b.ssd_counts(targets, iters, p)
    h2 = b.ssd_counts(targets, 33, p)  # continues the iteration counter
    gap = G.flip_gap_table(N, p)
    st, r1 = oracle_mod.ssd_philox(o, s0, targets, gap, SEED, 5, 0, iters)
    st, r2 = oracle_mod.ssd_philox(o, st, targets, gap, SEED, 5, iters, 33)
    assert_edges_move(s0, st, N, kind)
    assert np.array_equal(h1, r1) and np.array_equal(h2, r2)
    assert np.array_equal(b.get_state(), st)
    assert int(h1.sum()) == Bs * iters and (r1 > 0).sum() >= 4  # the targets take both values
    b.close()


# ---------------------------------------------------------------------- state set and PBN-v0 env (tables)
def _classify(batch, s, words=None):
    import torch

    out = torch.full((batch.n_envs,), -7, dtype=torch.int32, device="cuda:0")
    t = None if words is None else _dev(words)
    _sync()
    batch.classify(s, out.data_ptr(), 0 if t is None else t.data_ptr())
    batch.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", SHAPES)
def test_stateset_classify(G, oracle_mod, knobs, N):
    """k_set_lookup vs the host ``StateSet.lookup`` (and that vs a Python dict): members, and decoys that
    differ from a member in node N - 1 or in one bit of the last word only."""
    from gym_pbn_amd.stateset import StateSet

    net = shape_net("tt", N)
    W = net.n_words
    b = G.PBNBatch(net, B, seed=SEED)
    b.randomize()
    state = b.get_state()
    rng = np.random.default_rng(N)
    members = np.unique(state[::2], axis=0)
    labels = np.arange(len(members)) % 7
    lo = 64 * (W - 1) + (1 if W == 1 else 0)  # the last word's nodes (node 0 of a table is always 0)
    decoy_top, decoy_last = members.copy(), members.copy()
    decoy_top[:, -1] ^= _bit(N - 1)
    bit = rng.integers(lo, N, size=len(members))
    decoy_last[:, -1] ^= np.uint64(1) << (bit % 64).astype(np.uint64)
    s = StateSet(members, N, labels=labels, device=0)
    table = {tuple(r.tolist()): int(l) for r, l in zip(members, labels)}
    pool = np.concatenate([members, decoy_top, decoy_last, state])
    q = pool[rng.integers(0, len(pool), size=B)]
    q[0], q[1], q[2] = members[-1], decoy_top[-1], decoy_last[0]
    want = np.array([table.get(tuple(r.tolist()), -1) for r in q], np.int32)
    assert want[0] >= 0 and want[1] == -1 and (want == -1).sum() > B // 4 and (want >= 0).sum() > B // 8
    assert np.array_equal(s.lookup(q), want)
    assert np.array_equal(_classify(b, s, q), want)
    own = np.array([table.get(tuple(r.tolist()), -1) for r in state], np.int32)
    assert np.array_equal(_classify(b, s), own) and (own[::2] >= 0).all()
    assert np.array_equal(b.get_state(), state)
    s.close()
    b.close()


@pytest.mark.parametrize("N", SHAPES)
def test_tenv_step_and_reset(G, oracle_mod, knobs, N):
    """k_tenv_step == flip + step(1) + host lookup (and the oracle's update of the flipped state), with actions
    on nodes 63, 64 and N - 1; k_tenv_reset vs the documented draw (stream 9, mulhi(word 0, n_states))."""
    import torch

    from gym_pbn_amd.stateset import StateSet

    network = shape_net("tt", N)
    net = G.Net(network)
    W, base, steps = net.n_words, 2**33 + 1, 6
    o = orc(oracle_mod, "tt", N)
    rng = np.random.default_rng(N)
    acts = rng.integers(1, N, size=(steps, B)).astype(np.int32)
    acts[rng.random((steps, B)) < 0.5] = 0
    acts[0, :3] = [N - 1, min(64, N - 1), 63 if N > 63 else 1]
    twin = G.PBNBatch(net, B, env_id_base=base, seed=SEED)
    twin.randomize()
    s0 = twin.get_state()
    want, prev = [], s0
    for t in range(steps):
        twin.flip(acts[t][:, None], offset=0, dedup=True)
        twin.step(1)
        flipped = prev.copy()
        for e in np.nonzero(acts[t])[0]:
            flipped[e, acts[t, e] // 64] ^= _bit(int(acts[t, e]))
        now = o.step_philox(flipped, SEED, base, t, 1)
        assert np.array_equal(twin.get_state(), now), t
        want.append(now)
        prev = now
    twin.close()
    assert_edges_move(s0, want[-1], N, "tt")
    pool = np.unique(np.concatenate(want), axis=0)
    members = pool[rng.random(len(pool)) < 0.5]
    target = StateSet(members, N, labels=np.arange(len(members)) % 5, device=0)
    f = G.PBNBatch(net, B, env_id_base=base, seed=SEED)
    f.randomize()
    obs = torch.full((B, W), -77, dtype=torch.int64, device="cuda:0")
    reward = torch.full((B,), -77, dtype=torch.int32, device="cuda:0")
    flags = torch.full((B,), 99, dtype=torch.uint8, device="cuda:0")
    label = torch.full((B,), -77, dtype=torch.int32, device="cuda:0")
    seen = set()
    for t in range(steps):
        a = _dev(acts[t])
        _sync()
        f.tenv_step_device(target, a.data_ptr(), reward.data_ptr(), flags.data_ptr(), d_obs=obs.data_ptr(),
                           d_labels=label.data_ptr())
        f.sync()
        lab = target.lookup(want[t])
        assert np.array_equal(f.get_state(), want[t]) and np.array_equal(obs.cpu().numpy().view(np.uint64), want[t]), t
        assert np.array_equal(label.cpu().numpy(), lab), t
        assert np.array_equal(flags.cpu().numpy(), (lab >= 0).astype(np.uint8)), t
        assert np.array_equal(reward.cpu().numpy(), np.where(lab >= 0, 20, -4 - (acts[t] != 0)).astype(np.int32)), t
        seen |= set((lab >= 0).tolist())
    assert seen == {True, False}
    # reset: rows with node 0 and node N - 1 set; the documented pick; node 0 cleared; masked envs keep theirs
    n_states = 3
    table = rng.integers(0, 2**63, size=(n_states, W), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    if N % 64:
        table[:, -1] &= np.uint64((1 << (N % 64)) - 1)
    table[:, -1] |= _bit(N - 1)
    d_table, mask = _dev(table), rng.random(B) < 0.5
    d_mask = _dev(mask.astype(np.uint8))
    before, rc = f.get_state(), f.counters()["reset_count"]
    _sync()
    f.tenv_reset_device(d_table.data_ptr(), n_states, d_mask.data_ptr())
    f.sync()
    picks = np.array([(oracle_mod.philox4x32_10([0, rc, g & 0xFFFFFFFF, ((g >> 32) & 0xFFFFFF) | (9 << 24)],
                                                [SEED & 0xFFFFFFFF, SEED >> 32])[0] * n_states) >> 32
                      for g in range(base, base + B)])
    cleared = table.copy()
    cleared[:, 0] &= ~np.uint64(1)
    assert len(set(picks.tolist())) == n_states
    assert np.array_equal(f.get_state(), np.where(mask[:, None], cleared[picks], before))
    assert f.counters()["reset_count"] == rc + 1
    f.close()
    target.close()


# ---------------------------------------------------------------------------------------------------- reach
@pytest.mark.parametrize("kind,N,graph", [("pm", n, None) for n in SHAPES]
                         + [("tt", n, g) for n in SHAPES for g in ("stg", "step")])
def test_reach_unstable(G, knobs, kind, N, graph):
    """``ReachSet.unstable`` (the edge-rule kernel, both kinds and both table graphs) on 257 random states
    against the numpy statement of the rule."""
    from gym_pbn_amd.attractors import ReachSet
    from test_attractors_host import np_unstable_words
    from test_attractors_tt_host import np_tt_unstable_words

    net = shape_net(kind, N)
    bits = np.random.default_rng(N).integers(0, 2, size=(257, N), dtype=np.uint8)
    bits[0, N - 1], bits[1, N - 1] = 0, 1
    states = G.pack_bits(bits)
    if kind == "pm":
        rs, want = ReachSet(net, 64), np_unstable_words(net, states)
    else:
        rs, want = ReachSet(net, 64, table_graph=graph), np_tt_unstable_words(net, states, graph)
    got = rs.unstable(states)
    assert got.shape == (257, net.n_words)
    assert np.array_equal(got, want)
    moved = np.bitwise_or.reduce(want, axis=0)
    assert (int(moved[-1]) >> ((N - 1) % 64)) & 1  # node N - 1 is unstable in some state: the top bit is computed
