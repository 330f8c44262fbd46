"""``PBNBatch.classify`` (k_set_lookup) equals the host ``StateSet.lookup`` -- the same walk, one definition.

Shapes: B = 257 (a second workgroup with one live lane) and B = 1; W = 1 (``tt8``) and W = 4 (``tt200``, nodes
across word boundaries). ``tt8`` has 2^8 states, of which only 4 share home slot 63 of a 64-slot table, so the
12-state wrapped walk cannot be built over it: there the colliding set is those 4 (walks that wrap, 4 long) and the
full 12-state set runs on a 40-node synthetic network, still W = 1. Every other width (W = 1 .. 8, ``N % 64 == 0``,
decoys in the last word) is in ``test_shape_sweep_gpu.py::test_stateset_classify``.
"""

import numpy as np
import pytest

from test_stateset_host import colliding_rows, py_home

pytestmark = pytest.mark.gpu


def _network(name):
    from gym_pbn_amd.network import TruthTableNetwork, load_network, synthetic_truth_table_pbn

    if name == "tt40":
        return TruthTableNetwork.from_pbn_data(synthetic_truth_table_pbn(40, 3, seed=5), name=name)
    return load_network(name)


def _same_home_rows(n_nodes):
    if n_nodes >= 40:
        return colliding_rows(n_nodes)
    rows = np.array([[v] for v in range(1 << n_nodes) if py_home([v], 64) == 63], dtype=np.uint64)
    assert len(rows) >= 3
    return rows


def _classify(batch, s, words=None):
    import torch

    dev = torch.device("cuda", 0)
    out = torch.full((batch.n_envs,), -7, dtype=torch.int32, device=dev)
    d_words = 0
    if words is not None:
        t = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev)
        d_words = t.data_ptr()
    torch.cuda.synchronize(dev)
    batch.classify(s, out.data_ptr(), d_words)
    batch.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("B", [257, 1])
@pytest.mark.parametrize("name", ["tt8", "tt200", "tt40"])
def test_classify_equals_host_lookup(name, B):
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    net = Net(_network(name))
    N, W = net.n_nodes, net.n_words
    b = PBNBatch(net, B, seed=11)
    b.randomize()
    state = b.get_state()
    rng = np.random.default_rng(B)
    half = np.unique(state[::2], axis=0)
    decoys = half.copy()  # members with one bit flipped: most are non-members, the host lookup says which
    bit = rng.integers(0, N, size=len(half))
    decoys[np.arange(len(half)), bit // 64] ^= np.uint64(1) << (bit % 64).astype(np.uint64)
    same_home = _same_home_rows(N)
    sets = {
        "empty": (np.zeros((0, W), np.uint64), None),
        "one": (state[:1], [5]),
        "same-home": (same_home, np.arange(len(same_home)) + 1),
        "half": (half, np.arange(len(half)) % 9),
    }
    for tag, (rows, labels) in sets.items():
        s = StateSet(rows, N, labels=labels, device=0)
        if tag == "same-home":
            assert s.info()["max_probe"] == len(same_home) and (name == "tt8" or len(same_home) == 12)
        # the batch's own state (d_words NULL)
        got = _classify(b, s)
        assert np.array_equal(got, s.lookup(state)), (tag, "state")
        assert np.array_equal(b.classify_host(s), got), (tag, "classify_host")
        # the caller's words: members, decoys and the colliding rows, cycled to B rows
        pool = np.concatenate([rows.reshape(-1, W), decoys, same_home, state])
        q = pool[rng.integers(0, len(pool), size=B)]
        if len(rows):
            q[0] = rows[-1]  # a member in every batch, B = 1 included (same-home: the longest walk)
        want = s.lookup(q)
        assert np.array_equal(_classify(b, s, q), want), (tag, "words")
        assert len(rows) == 0 or want[0] >= 0, tag
        if B > 1 and tag in ("same-home", "half"):
            assert (want == -1).any(), tag
        s.close()
    assert np.array_equal(b.get_state(), state)  # a lookup writes nothing
    b.close()


def test_mismatched_set_or_batch_is_refused():
    import torch

    from gym_pbn_amd import _lib
    from gym_pbn_amd.batch import Net, PBNBatch
    from gym_pbn_amd.stateset import StateSet

    b = PBNBatch(Net(_network("tt8")), 4, seed=1)
    out = torch.full((4,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    wrong_n = StateSet(np.array([[1]], np.uint64), 9, device=0)
    with pytest.raises(ValueError, match="9 nodes"):
        b.classify(wrong_n, out.data_ptr())
    host_only = StateSet(np.array([[1]], np.uint64), 8, device=None)
    with pytest.raises(_lib.PbnError) as ei:
        b.classify(host_only, out.data_ptr())
    assert ei.value.code == _lib.PBN_E_STATE
    if _lib.device_count() > 1:
        other = StateSet(np.array([[1]], np.uint64), 8, device=1)
        with pytest.raises(ValueError, match="device"):
            b.classify(other, out.data_ptr())
    b.sync()
    assert (out.cpu().numpy() == -7).all()  # nothing was launched
    b.close()
