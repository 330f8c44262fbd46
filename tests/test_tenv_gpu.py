"""The ``PBN-v0`` env on the device: the fused step (k_tenv_step), the reset over a table of states (k_env_set_reset)
and ``TorchVecPBNEnv`` on top of them. Every comparison is bit-exact.

The fused step is held against the calls it replaces (``PBNBatch.flip`` + ``step(1)`` + host ``StateSet.lookup``)
on a twin batch of the same seed, and -- independently of the product's own step path -- against
``oracle.Oracle.step_philox`` applied to the flipped state.
"""

import json

import numpy as np
import pytest

from conftest import GOLDEN
from shape_cases import tt_net

pytestmark = pytest.mark.gpu

KAT = json.loads((GOLDEN / "mdp_kat.json").read_text())
SENTINEL = -77


def _tt6_source():
    net = KAT["networks"]["tt6"]
    return [(np.array(d["mask"], dtype=bool), np.array(d["table"]).reshape((2,) * sum(d["mask"])), d["name"],
             d["control"]) for d in net["PBN_data"]]


def _network(name):
    from gym_pbn_amd.network import TruthTableNetwork, load_network

    return TruthTableNetwork.from_pbn_data(_tt6_source()) if name == "tt6" else load_network(name)


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to("cuda:0")


class _Out:
    """Device output buffers of one fused step, prefilled so that an untouched row shows."""

    def __init__(self, B, W):
        import torch

        self.obs = torch.full((B, W), SENTINEL, dtype=torch.int64, device="cuda:0")
        self.reward = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda:0")
        self.flags = torch.full((B,), 99, dtype=torch.uint8, device="cuda:0")
        self.label = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def step(self, batch, target, actions, check=False):
        a = _dev(np.asarray(actions, dtype=np.int32))
        import torch

        torch.cuda.synchronize()
        batch.tenv_step_device(target, a.data_ptr(), self.reward.data_ptr(), self.flags.data_ptr(),
                               d_obs=self.obs.data_ptr(), d_labels=self.label.data_ptr(), check=check)
        batch.sync()
        return (self.obs.cpu().numpy().view(np.uint64), self.reward.cpu().numpy(), self.flags.cpu().numpy(),
                self.label.cpu().numpy())


def _flip_rows(words, actions):
    out = words.copy()
    for e in np.nonzero(actions)[0]:
        a = int(actions[e])
        out[e, a // 64] ^= np.uint64(1) << np.uint64(a % 64)
    return out


def _actions(rng, B, N, steps):
    a = rng.integers(1, N, size=(steps, B))
    a[rng.random((steps, B)) < 0.5] = 0  # half of the actions are 0
    return a.astype(np.int32)


@pytest.mark.parametrize("name,B,base", [("tt6", 257, 0), ("tt6", 2, 1), ("tt200", 257, 0), ("tt200", 2, 1)])
def test_fused_step_equals_flip_step_lookup(name, B, base, oracle_mod):
    """20 steps. env_id_base 1 with B = 2 puts envs 1 and 2 in one batch: they take words of two different
    Philox calls ({u, 0} words 2-3 and {u, 1} words 0-1)."""
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    network = _network(name)
    net = Net(network)
    N, W, seed, steps = net.n_nodes, net.n_words, 5, 20
    orc = oracle_mod.Oracle(network)
    rng = np.random.default_rng(B + base)
    acts = _actions(rng, B, N, steps)
    # the existing calls first, on the twin: their states are the expected ones and supply the target's members
    twin = PBNBatch(net, B, env_id_base=base, seed=seed)
    twin.randomize()
    s0 = twin.get_state()
    want = []
    prev = s0
    for t in range(steps):
        if acts[t].any():
            twin.flip(acts[t][:, None], offset=0, dedup=True)
        twin.step(1)
        now = twin.get_state()
        # independent of the product's step path: the oracle's update t of the flipped state
        assert np.array_equal(now, orc.step_philox(_flip_rows(prev, acts[t]), seed, base, t, 1)), t
        want.append(now)
        prev = now
    twin.close()
    pool = np.unique(np.concatenate(want), axis=0)
    members = pool[rng.random(len(pool)) < 0.5]
    target = StateSet(members, N, labels=np.arange(len(members)) % 5, device=0)

    f = PBNBatch(net, B, env_id_base=base, seed=seed)
    f.randomize()
    assert np.array_equal(f.get_state(), s0)
    out = _Out(B, W)
    seen_term = seen_not = False
    for t in range(steps):
        obs, reward, flags, label = out.step(f, target, acts[t])
        assert np.array_equal(f.get_state(), want[t]), t
        assert np.array_equal(obs, want[t]), t
        lab = target.lookup(want[t])
        assert np.array_equal(label, lab), t
        term = lab >= 0
        assert np.array_equal(flags, term.astype(np.uint8)), t
        assert np.array_equal(reward, np.where(term, 20, -4 - (acts[t] != 0)).astype(np.int32)), t
        assert f.counters()["update_count"] == t + 1
        seen_term |= bool(term.any())
        seen_not |= bool((~term).any())
    assert seen_term and seen_not
    f.close()
    target.close()


@pytest.mark.parametrize("name", ["tt6", 65])
def test_one_workgroup_walks_every_env(name, monkeypatch, oracle_mod):
    """B = 600 with the grid capped at one workgroup (PBNSIM_ENVSET_GRID=1): every lane takes two or three envs in
    the grid-stride loop, and on the third trip only 88 lanes are live -- one full wave, one partly live, two that
    have left. tt6: W = 1; ttk3_65: W = 2, node 64 alone in the second word. Expected values: the oracle's update of
    the flipped state and the host lookup. Env 520 (third trip) holds an invalid action in step 1: skipped whole."""
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    network = tt_net(name) if isinstance(name, int) else _network(name)
    net = Net(network)
    N, W, B, seed, base, steps = net.n_nodes, net.n_words, 600, 11, 3, 3
    orc = oracle_mod.Oracle(network)
    rng = np.random.default_rng(N)
    acts = _actions(rng, B, N, steps)
    acts[0, :3], acts[2, -1] = [1, N - 1, 0], N - 1  # node N - 1 on the first trip and on the last live lane
    acts[1, 520] = N
    monkeypatch.setenv("PBNSIM_ENVSET_GRID", "1")
    f = PBNBatch(net, B, env_id_base=base, seed=seed)
    f.randomize()
    prev = f.get_state()
    want = []
    for t in range(steps):
        ok = np.where(acts[t] < N, acts[t], 0)
        now = orc.step_philox(_flip_rows(prev, ok), seed, base, t, 1)
        now[acts[t] >= N] = prev[acts[t] >= N]
        want.append(now)
        prev = now
    pool = np.unique(np.concatenate(want), axis=0)
    members = pool[rng.random(len(pool)) < 0.5]
    target = StateSet(members, N, labels=np.arange(len(members)) % 5, device=0)
    out = _Out(B, W)
    for t in range(steps):
        out.obs.fill_(SENTINEL)
        out.reward.fill_(SENTINEL)
        obs, reward, flags, label = out.step(f, target, acts[t])
        bad = acts[t] >= N
        assert bad.sum() == (t == 1)
        assert np.array_equal(f.get_state(), want[t]), t
        assert np.array_equal(obs[~bad], want[t][~bad]), t
        lab = target.lookup(want[t])
        term = lab >= 0
        assert term[512:].any() and (~term[512:]).any() and term[:256].any()
        assert np.array_equal(label[~bad], lab[~bad]), t
        assert np.array_equal(flags[~bad], term[~bad].astype(np.uint8)), t
        assert np.array_equal(reward[~bad], np.where(term, 20, -4 - (acts[t] != 0)).astype(np.int32)[~bad]), t
        assert (obs[bad].view(np.int64) == SENTINEL).all() and (reward[bad] == SENTINEL).all()
    with pytest.raises(ValueError, match="Invalid action"):
        out.step(f, target, np.zeros(B, np.int32), check=True)  # env 520's skip, noted on the third trip
    f.close()
    target.close()


def test_fused_step_mixes_with_step_and_rollout(oracle_mod):
    """step(3), one fused step, rollout(2) == six oracle updates with the flip in place."""
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    network = _network("tt200")
    net = Net(network)
    B, seed = 257, 9
    orc = oracle_mod.Oracle(network)
    b = PBNBatch(net, B, seed=seed)
    b.randomize()
    s0 = b.get_state()
    acts = _actions(np.random.default_rng(2), B, net.n_nodes, 1)[0]
    target = StateSet(np.zeros((0, net.n_words), np.uint64), net.n_nodes, device=0)
    b.step(3)
    obs, reward, flags, label = _Out(B, net.n_words).step(b, target, acts)
    b.rollout(2)
    s3 = orc.step_philox(s0, seed, 0, 0, 3)
    s4 = orc.step_philox(_flip_rows(s3, acts), seed, 0, 3, 1)
    assert np.array_equal(obs, s4)
    assert np.array_equal(b.get_state(), orc.step_philox(s4, seed, 0, 4, 2))
    assert b.counters()["update_count"] == 6
    assert (label == -1).all() and (flags == 0).all() and np.array_equal(reward, -4 - (acts != 0))
    b.close()


@pytest.mark.parametrize("name", ["tt6", "tt200"])
def test_a_bad_action_skips_its_env_and_is_reported_once(name, oracle_mod):
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    network = _network(name)
    net = Net(network)
    N, W, B, seed = net.n_nodes, net.n_words, 70, 4
    orc = oracle_mod.Oracle(network)
    b = PBNBatch(net, B, seed=seed)
    b.randomize()
    s0 = b.get_state()
    acts = _actions(np.random.default_rng(3), B, N, 1)[0]
    acts[3], acts[66] = -1, N
    bad = np.zeros(B, bool)
    bad[[3, 66]] = True
    target = StateSet(s0, N, device=0)  # every start state: the skipped rows would terminate if they were looked up
    out = _Out(B, W)
    obs, reward, flags, label = out.step(b, target, acts, check=False)  # asynchronous: no report yet
    ok = np.where(bad, 0, acts)
    s1 = orc.step_philox(_flip_rows(s0, ok), seed, 0, 0, 1)
    got = b.get_state()
    assert np.array_equal(got[bad], s0[bad]) and np.array_equal(got[~bad], s1[~bad])
    assert (obs[bad].view(np.int64) == SENTINEL).all() and np.array_equal(obs[~bad], s1[~bad])
    assert (reward[bad] == SENTINEL).all() and (flags[bad] == 99).all() and (label[bad] == SENTINEL).all()
    assert np.array_equal(label[~bad], target.lookup(s1[~bad]))
    assert b.counters()["update_count"] == 1  # the launch happened
    zeros = np.zeros(B, np.int32)
    with pytest.raises(ValueError, match="Invalid action"):
        out.step(b, target, zeros, check=True)  # the sticky flag, raised once ...
    assert b.counters()["update_count"] == 2
    out.step(b, target, zeros, check=True)  # ... and cleared
    with pytest.raises(ValueError, match="Invalid action"):
        acts[:] = 0
        acts[0] = N + 5
        out.step(b, target, acts, check=True)
    assert b.counters()["update_count"] == 4
    b.close()


def test_refusals_launch_nothing():
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    b = PBNBatch(Net(_network("tt6")), 8, seed=1)
    b.randomize()
    s0 = b.get_state()
    out = _Out(8, 1)
    a = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def step(batch, target):
        batch.tenv_step_device(target, a.data_ptr(), out.reward.data_ptr(), out.flags.data_ptr())

    with pytest.raises(ValueError, match="7 nodes"):
        step(b, StateSet(np.array([[1]], np.uint64), 7, device=0))
    with pytest.raises(_lib.PbnError) as ei:
        step(b, StateSet(np.array([[1]], np.uint64), 6, device=None))
    assert ei.value.code == _lib.PBN_E_STATE
    table = _dev(np.array([[1]], np.uint64))
    for n in (0, 1 << 32):
        with pytest.raises(ValueError, match="n_states"):
            b.tenv_reset_device(table.data_ptr(), n)
    mix = PBNBatch("bittner28", 8, seed=1)
    for call in (lambda: step(mix, StateSet(np.array([[1]], np.uint64), 28, device=0)),
                 lambda: mix.tenv_reset_device(table.data_ptr(), 1)):
        with pytest.raises(_lib.PbnError) as ei:
            call()
        assert ei.value.code == _lib.PBN_E_UNSUPPORTED
    b.sync()
    assert np.array_equal(b.get_state(), s0) and (out.reward.cpu().numpy() == SENTINEL).all()
    assert b.counters()["update_count"] == 0 and b.counters()["reset_count"] == 1  # randomize alone
    b.close()
    mix.close()


def _reset_picks(oracle_mod, seed, base, reset_count, B, n):
    """mulhi(philox4x32_10(ctr {0, reset_count, gid_lo, gid_hi & 0xFFFFFF | 9 << 24}, key seed)[0], n)."""
    picks = []
    for e in range(B):
        g = base + e
        w = oracle_mod.philox4x32_10([0, reset_count, g & 0xFFFFFFFF, ((g >> 32) & 0xFFFFFF) | (9 << 24)],
                                     [seed & 0xFFFFFFFF, seed >> 32])
        picks.append((w[0] * n) >> 32)
    return np.array(picks)


@pytest.mark.parametrize("name,n_states", [("tt6", 1), ("tt6", 3), ("tt200", 3)])
def test_reset_draws_rows_by_the_documented_counter(name, n_states, oracle_mod):
    from gym_pbn_amd.batch import Net, PBNBatch

    net = Net(_network(name))
    N, W, B = net.n_nodes, net.n_words, 257
    seed, base = (7 << 32) | 12345, (1 << 33) + 3  # both words of the key and of the env id in use
    rng = np.random.default_rng(n_states)
    table = rng.integers(0, 1 << 64, size=(n_states, W), dtype=np.uint64)
    table[:, -1] &= np.uint64((1 << (N - 64 * (W - 1))) - 1)
    table[:, 0] |= np.uint64(1)  # node 0 set in every row: the reset clears it
    d_table = _dev(table)
    b = PBNBatch(net, B, env_id_base=base, seed=seed)
    b.randomize()
    before = b.get_state()
    rc = b.counters()["reset_count"]
    mask = rng.random(B) < 0.5
    d_mask = _dev(mask.astype(np.uint8))
    import torch

    torch.cuda.synchronize()
    b.tenv_reset_device(d_table.data_ptr(), n_states, d_mask.data_ptr())
    b.sync()
    cleared = table.copy()
    cleared[:, 0] &= ~np.uint64(1)
    picks = _reset_picks(oracle_mod, seed, base, rc, B, n_states)
    assert n_states == 1 or len(set(picks.tolist())) == n_states
    want = np.where(mask[:, None], cleared[picks], before)
    assert np.array_equal(b.get_state(), want)
    assert b.counters()["reset_count"] == rc + 1
    b.tenv_reset_device(d_table.data_ptr(), n_states)  # no mask: every env, the next counter
    b.sync()
    assert np.array_equal(b.get_state(), cleared[_reset_picks(oracle_mod, seed, base, rc + 1, B, n_states)])
    assert b.counters()["reset_count"] == rc + 2
    b.close()


def test_torch_env_equals_vec_env_on_tt6(oracle_mod):
    import torch

    from gym_pbn_amd.envs import VecPBNEnv
    from gym_pbn_amd.torch_env import TorchVecPBNEnv

    case = next(c for c in KAT["cases"] if c["network"] == "tt6" and c["kind"] == "PBNEnv")
    target = {tuple(t) for t in case["target"]}
    B, seed = 257, 3
    v = VecPBNEnv(_tt6_source(), goal_config={"target_nodes": target}, n_envs=B, seed=seed)
    env = TorchVecPBNEnv(_tt6_source(), goal_config={"target_nodes": target}, n_envs=B, seed=seed)
    assert set(env.target_words[:, 0].tolist()) == {sum(int(x) << i for i, x in enumerate(s)) for s in v.target_nodes}
    env.batch.set_bits(v.reset())
    rng = np.random.default_rng(0)
    any_term = False
    for t in range(20):
        a = rng.integers(0, v.N, size=B)
        a[rng.random(B) < 0.5] = 0
        o, r, term, trunc, _ = v.step(a)
        to, tr, tterm, ttrunc, info = env.step(torch.from_numpy(a).to("cuda:0"))
        assert to.dtype == torch.uint8 and tr.dtype == torch.int32 and tterm.dtype == torch.bool
        assert np.array_equal(to.cpu().numpy(), o), t
        assert np.array_equal(tr.cpu().numpy(), r), t
        assert np.array_equal(tterm.cpu().numpy(), term) and not ttrunc.any().item(), t
        assert np.array_equal(info["obs_words"].cpu().numpy().view(np.uint64), v.batch.get_state())
        assert np.array_equal(info["label"].cpu().numpy() >= 0, term)
        any_term |= bool(term.any())
    assert any_term and not term.all()
    with pytest.raises(ValueError, match="Invalid action"):
        env.step(torch.full((B,), v.N, dtype=torch.int64, device="cuda:0"), check=True)
    env.close()

    # auto-reset: an env that ended holds the attracting state the documented draw names, node 0 cleared
    env = TorchVecPBNEnv(_tt6_source(), goal_config={"target_nodes": target}, n_envs=B, seed=seed, auto_reset=True)
    attracting = env._attracting.cpu().numpy().view(np.uint64)
    assert env.info()["n_attracting"] == len(attracting) == len(set.union(*v.all_attractors))
    env.batch.set_bits(v.batch.get_bits())
    ended = 0
    for t in range(5):
        rc = env.batch.counters()["reset_count"]
        a = rng.integers(0, v.N, size=B)
        _, _, term, _, info = env.step(torch.from_numpy(a).to("cuda:0"))
        term = term.cpu().numpy()
        after = env.observation_words().cpu().numpy().view(np.uint64)
        picks = _reset_picks(oracle_mod, seed, 0, rc, B, len(attracting))
        want = np.where(term[:, None], attracting[picks] & ~np.uint64(1), info["obs_words"].cpu().numpy().view(np.uint64))
        assert np.array_equal(after, want), t
        assert env.batch.counters()["reset_count"] == rc + 1
        ended += int(term.sum())
    assert ended > 0
    obs = env.reset()  # every env, on the device
    assert env.target.lookup(env.observation_words().cpu().numpy().view(np.uint64)).shape == (B,)
    assert obs.shape == (B, v.N) and not obs[:, 0].any().item()
    env.close()


def test_attractors_past_65536_states():
    """18 nodes: node 0 can only fall (p = 0 everywhere), nodes 1-17 move freely (p = 0.5): the one "stg"
    attractor is the 2^17 states with x_0 = 0 -- twice what the host envs' Python sets take."""
    import torch

    from gym_pbn_amd.attractors import MAX_ENV_STATES, find_state_attractors
    from gym_pbn_amd.network import TruthTableNetwork
    from gym_pbn_amd.torch_env import TorchVecPBNEnv

    N = 18
    data = []
    for i in range(N):
        mask = np.zeros(N, dtype=bool)
        mask[i] = True  # one input each: the node itself
        data.append((mask, np.full((2,), 0.0 if i == 0 else 0.5), f"n{i}", False))
    with pytest.raises(ValueError, match=str(1 << 17)):  # unchanged: the host envs stop at 2^16 states
        find_state_attractors(TruthTableNetwork.from_pbn_data(data), seed=1)
    assert MAX_ENV_STATES == 1 << 16
    B = 257
    env = TorchVecPBNEnv(data, goal_config={"target_nodes": {(0,) * N}}, n_envs=B, all_attractors="find", seed=1)
    info = env.info()
    assert info["n_states"] == 2 ** 17 and info["n_attracting"] == 2 ** 17 and info["table_slots"] == 2 ** 18
    assert len(env.attractors) == 1
    env.batch.randomize()  # node 0 cleared: every state is in the attractor, so in the expanded target
    a = torch.from_numpy(np.random.default_rng(0).integers(0, N, size=B)).to("cuda:0")
    obs, reward, term, trunc, out = env.step(a)
    assert term.all().item() and (reward == 20).all().item() and (out["label"] == 0).all().item()
    assert not obs[:, 0].any().item()
    env.close()
