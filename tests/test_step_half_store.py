"""The step kernel's dirty write-back (store_changed, pbn_device.hpp) against the oracle, bit for bit.

In the 1024-thread step kernels of a batch that is resident at once (every batch here) a changed env of W = 4
words is written back as the 16-B half that holds the updated node, by one store whose address varies by lane
(STORE_HALF); larger batches and 256-thread kernels write the whole changed env (STORE_DIRTY), and
``PBNSIM_STORE_MODE`` = 0 / 1 / 2 forces full / whole changed envs / changed halves. Every env and every word is compared with the oracle's Philox step after every call:
40 single-update calls from ``init_philox(B, 123)``, then calls of 2, 3, 20 and 64 updates. The shapes are the
smallest at which each path of k_step can go wrong (the knobs force the path):

* bittner199, B = 2500, block 1024, env id bases 10 and 7: k_step_pair with paired and unpaired Philox; grid 2,
  stride 2048, so threads 452 .. 2047 have a partner env past B (clamped load, no store). With chains 1 and 2
  and with plain launches and graph replays.
* bittner199, B = 2049, block 1024: exactly one thread has a partner.
* bittner199, B = 20000, block 1024, 8 envs per thread: ceil(20000 / 8) = 2500 lanes make a grid of 3
  workgroups, and 2 x 3 x 1024 = 6144 < 20000, so every thread walks several pairs: k_step_single behind
  k_step's own staging (PRE).
* bittner199, B = 4099, block 256: k_step_single, staged in the kernel.
* tt200 (truth tables, W = 4), B = 4100, base 3, blocks 256 and 1024.
* bittner149 (W = 3), bittner100 (W = 2), bittner28 (W = 1), B = 1500: the whole env as before.
* bittner199 with PBNSIM_STORE_MODE 0, 1 and 2: the full store, and k_step_pair and the PRE k_step_single with
  the whole-env write-back that larger batches take.

For the bittner199 shapes the oracle's states must show every node 0 .. 198 flipping in at least one env over
the 40 single-update calls, so both halves, both words of each half and the bits at the word and half
boundaries (63/64, 127/128, 198) are written by the store under test whatever the seed.
"""

import numpy as np
import pytest

from gym_pbn_amd.network import load_network

pytestmark = pytest.mark.gpu

SEED = 41
CALLS = (1,) * 40 + (2, 3, 20, 64)
KNOBS = ("PBNSIM_STEP_BLOCK", "PBNSIM_ENVS_PER_THREAD", "PBNSIM_STORE_MODE", "PBNSIM_STEP_CHAINS", "PBNSIM_STEP_GRAPH")

# (network, B, env id base, knobs)
PAIR = [("bittner199", 2500, base, {"PBNSIM_STEP_BLOCK": "1024", "PBNSIM_STEP_CHAINS": c, "PBNSIM_STEP_GRAPH": g})
        for base in (10, 7) for c in ("1", "2") for g in ("0", "1")]
CASES = PAIR + [
    ("bittner199", 2049, 0, {"PBNSIM_STEP_BLOCK": "1024"}),
    ("bittner199", 20000, 0, {"PBNSIM_STEP_BLOCK": "1024", "PBNSIM_ENVS_PER_THREAD": "8"}),
    ("bittner199", 4099, 0, {"PBNSIM_STEP_BLOCK": "256"}),
    ("tt200", 4100, 3, {"PBNSIM_STEP_BLOCK": "256"}),
    ("tt200", 4100, 3, {"PBNSIM_STEP_BLOCK": "1024"}),
    ("bittner149", 1500, 0, {"PBNSIM_STEP_BLOCK": "1024"}),
    ("bittner149", 1500, 0, {"PBNSIM_STEP_BLOCK": "256"}),
    ("bittner100", 1500, 0, {"PBNSIM_STEP_BLOCK": "1024"}),
    ("bittner100", 1500, 0, {"PBNSIM_STEP_BLOCK": "256"}),
    ("bittner28", 1500, 0, {"PBNSIM_STEP_BLOCK": "1024"}),
    ("bittner28", 1500, 0, {"PBNSIM_STEP_BLOCK": "256"}),
    ("bittner199", 2500, 10, {"PBNSIM_STEP_BLOCK": "1024", "PBNSIM_STORE_MODE": "0"}),
    ("bittner199", 2500, 10, {"PBNSIM_STEP_BLOCK": "1024", "PBNSIM_STORE_MODE": "1"}),
    ("bittner199", 2500, 7, {"PBNSIM_STEP_BLOCK": "1024", "PBNSIM_STORE_MODE": "2"}),
    ("bittner199", 20000, 0, {"PBNSIM_STEP_BLOCK": "1024", "PBNSIM_ENVS_PER_THREAD": "8", "PBNSIM_STORE_MODE": "1"}),
]


@pytest.fixture(scope="module")
def G():
    from gym_pbn_amd import _lib, batch

    assert _lib.device_count() >= 1, "gpu tests need a HIP device"
    return batch


_REF = {}


def reference(oracle_mod, name, B, base):
    """(network, the initial state, the oracle's state after every call): computed once per shape, read-only."""
    key = (name, B, base)
    if key not in _REF:
        net = load_network(name)
        o = oracle_mod.Oracle(net)
        st = o.init_philox(B, 123, env_base=base)
        st.setflags(write=False)
        states, u = [], 0
        for n in CALLS:
            nx = o.step_philox(states[-1] if states else st, SEED, base, u, n)
            nx.setflags(write=False)
            states.append(nx)
            u += n
        _REF[key] = (net, st, states)
    return _REF[key]


def flipped_nodes(st0, states, n_nodes):
    """Nodes that flip in at least one env over the given consecutive states (from the oracle alone)."""
    acc = np.zeros(st0.shape[1], dtype=np.uint64)
    prev = st0
    for s in states:
        acc |= np.bitwise_or.reduce(prev ^ s, axis=0)
        prev = s
    return {i for i in range(n_nodes) if (int(acc[i >> 6]) >> (i & 63)) & 1}


@pytest.mark.parametrize("name,B,base,knobs", CASES, ids=lambda v: "-".join(v.values()) if isinstance(v, dict) else str(v))
def test_every_env_matches_the_oracle_after_every_call(G, oracle_mod, monkeypatch, name, B, base, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    net, st0, states = reference(oracle_mod, name, B, base)
    if name == "bittner199":
        assert flipped_nodes(st0, states[:40], 199) == set(range(199)), "the inputs do not flip every node"
    b = G.PBNBatch(net, B, seed=SEED, env_id_base=base)
    b.set_state(st0)
    for k, n in enumerate(CALLS):
        b.step(n)
        got = b.get_state()
        assert np.array_equal(got, states[k]), (k, n, int(np.count_nonzero((got != states[k]).any(axis=1))))
    assert b.info()["update_count"] == sum(CALLS)
    b.close()
