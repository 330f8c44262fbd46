"""Step mode's launch chains (pbn_step over contiguous env ranges on separate streams) against the oracle.

``PBNSIM_STEP_CHAINS`` forces 1, 2 or 4 chains; every env of every case is compared with the oracle's Philox
step (bit-exact: the path is integer-only) after every call, with plain launches and with graph replays.
Batch sizes are odd or just past a multiple of the block so the last slice is ragged; env id bases 7 and 10
take the unpaired and the paired Philox path; tt200 is the truth-table kind (k_step_single); B = 5 with four
chains is clamped to three.
"""

import numpy as np
import pytest

from gym_pbn_amd.network import load_network

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 3, 20, 20, 64, 65, 130)
SHAPES = [("bittner199", 4099, 7), ("bittner199", 4099, 10), ("bittner28", 8193, 0), ("tt200", 4100, 3)]
CASES = [(*s, c) for s in SHAPES for c in ("1", "2", "4")] + [("bittner199", 5, 2, "4")]


@pytest.fixture(scope="module")
def G():
    from gym_pbn_amd import _lib, batch

    assert _lib.device_count() >= 1, "gpu tests need a HIP device"
    return batch


_ORACLES = {}


def oracle_for(oracle_mod, name):
    if name not in _ORACLES:
        net = load_network(name)
        _ORACLES[name] = (net, oracle_mod.Oracle(net))
    return _ORACLES[name]


def expected_chains(B, chains):
    return min(int(chains), (B + 1) // 2)


@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("name,B,base,chains", CASES)
def test_forced_chains_match_oracle(G, oracle_mod, monkeypatch, name, B, base, chains, graph):
    monkeypatch.setenv("PBNSIM_STEP_CHAINS", chains)
    monkeypatch.setenv("PBNSIM_STEP_GRAPH", graph)
    net, o = oracle_for(oracle_mod, name)
    seed = 41
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    assert b.info()["step_chains"] == expected_chains(B, chains)
    b.randomize()
    st = b.get_state()
    u = 0
    lo = 1 if net.kind == 2 else 0
    ni = np.random.default_rng(B).integers(lo, net.n_nodes, size=(2, B)).astype(np.uint32)
    for k, n in enumerate(STEPS):
        b.step(n)
        st = o.step_philox(st, seed, base, u, n)
        u += n
        if k == 0:
            b.rollout(5)
            st = o.step_philox(st, seed, base, u, 5)
            u += 5
        elif k == 1:
            b.step_forced(ni)
            st = o.step_forced(st, ni, seed, base, u)
            u += 2
        elif k == 3:  # no read since the last call: set_state is ordered behind the chains
            st = o.init_philox(B, 123, env_base=base)
            b.set_state(st)
            continue
        elif k == 4:  # the reset kernel is queued right behind the chains' join
            b.randomize()
            st = b.get_state()
            continue
        assert np.array_equal(b.get_state(), st), (k, n)
    assert b.info()["update_count"] == u
    b.close()


@pytest.mark.parametrize("chains", ["1", "2", "4"])
def test_timing_counts_steps_not_chain_launches(G, monkeypatch, chains):
    monkeypatch.setenv("PBNSIM_STEP_CHAINS", chains)
    b = G.PBNBatch("bittner199", 4099, seed=3)
    b.randomize()
    b.timing(2)
    b.step(20)
    b.step(1)
    b.step(20)
    b.step(65)  # a 64-replay and a plain launch
    b.step(130)  # two 64-replays and a 2-replay
    b.timing(0)
    ms, launches = b.timing_read()
    assert launches == 236 and ms > 0
    b.timing(1)  # an event pair per launch: one whole-batch launch per step
    b.step(5)
    b.step(1)
    each = b.timing_read_each()
    b.timing(0)
    assert len(each) == 6 and all(x > 0 for x in each)
    b.close()


@pytest.mark.parametrize("chains", ["1", "2", "4"])
def test_capture_on_a_handed_over_stream(G, oracle_mod, monkeypatch, chains):
    """Inside the caller's capture pbn_step stays one chain on the caller's stream (the caller's graph gets a
    linear run of launches); afterwards the batch's own chains continue from the host counter."""
    import torch

    monkeypatch.setenv("PBNSIM_STEP_CHAINS", chains)
    net, o = oracle_for(oracle_mod, "bittner199")
    seed, base, B = 5, 10, 4099
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    b.randomize()
    b.step(4)  # the chains have run before the hand-over
    st = b.get_state()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.set_stream(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            b.step(8)
        s.synchronize()
        b.step(2)  # chain 0 on the caller's stream, the others on the batch's own
        s.synchronize()
        b.set_stream(None)
    st = o.step_philox(st, seed, base, 12, 2)  # the capture moved the host counter on by 8 and ran nothing
    assert np.array_equal(b.get_state(), st)
    for _ in range(2):  # a replay repeats the captured launches: updates 4 .. 11 again
        g.replay()
        torch.cuda.synchronize()
        st = o.step_philox(st, seed, base, 4, 8)
        assert np.array_equal(b.get_state(), st)
    b.step(20)
    assert np.array_equal(b.get_state(), o.step_philox(st, seed, base, 14, 20))
    b.close()


def test_default_is_one_chain_for_a_small_batch(G, monkeypatch):
    monkeypatch.delenv("PBNSIM_STEP_CHAINS", raising=False)
    b = G.PBNBatch("bittner199", 4099)
    assert b.info()["step_chains"] == 1
    b.close()


def test_default_chains_at_a_batch_that_fills_the_gpu_twice(G, oracle_mod, monkeypatch):
    """No knob, 1M Bittner-200 envs (the bench shape): two chains where each half fills every CU with
    1024-thread groups, split calls from 128 updates on (shorter ones run unsplit), graphs per chain. Envs
    at both ends of the batch and either side of the slice boundary are checked against the oracle."""
    import torch

    monkeypatch.delenv("PBNSIM_STEP_CHAINS", raising=False)
    monkeypatch.delenv("PBNSIM_STEP_GRAPH", raising=False)
    net, o = oracle_for(oracle_mod, "bittner199")
    B, seed, base = 1 << 20, 0x5EED, 6
    b = G.PBNBatch(net, B, seed=seed, env_id_base=base)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert b.info()["step_chains"] == (2 if B >= 2 * n_cu * 2048 else 1)
    b.randomize()
    st0 = b.get_state()
    for n in (130, 20, 200, 1):
        b.step(n)
    st = b.get_state()
    half = B // 2
    for k0, k1 in ((0, 2048), (half - 2048, half + 2048), (B - 2048, B)):
        assert np.array_equal(st[k0:k1], o.step_philox(st0[k0:k1], seed, base + k0, 0, 351)), (k0, k1)
    b.close()


def test_create_and_close_many_chained_batches(G, monkeypatch):
    """pbn_batch_destroy after chained steps gives back the chains' streams and events."""
    monkeypatch.setenv("PBNSIM_STEP_CHAINS", "4")
    net = G.Net(load_network("bittner28"))
    for k in range(64):
        b = G.PBNBatch(net, 4099, seed=k)
        assert b.info()["step_chains"] == 4
        b.randomize()
        b.step(4)
        b.close()
