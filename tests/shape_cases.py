"""The shape table of the words-per-env sweep (a plain module, not a conftest: ``from shape_cases import ...``).

Every kernel family is compiled once per state-word count ``W = ceil(N / 64)`` for ``W = 1 .. 8``
(``by_words<8>`` in ``csrc/pbn_launch.hpp``; the group kernels ``by_words<4>`` and ``N <= 256``). ``SHAPES``
reaches every ``W``, every ``N % 64 == 0`` up to the maximum ``N = 512`` (the tail mask is skipped there) and
both sides of 64 and of 256. Used by ``test_shape_sweep_host.py`` (oracle == unpacked model),
``test_shape_sweep_gpu.py`` (kernel == oracle) and, for the shapes with a reference golden
(``GOLDEN_R1`` / ``GOLDEN_R4``, made by ``tests/golden/make_golden.py shapes``), ``test_oracle.py`` and
``test_gpu_parity.py`` (oracle / kernel == reference).
"""

import functools

import numpy as np

SHAPES = [63, 64, 65, 128, 192, 256, 257, 320, 384, 448, 512]  # W = 1 1 2 2 3 4 5 5 6 7 8
KINDS = ["pm", "tt"]  # predictor mix (4 predictors at most per node), truth table (k = 3 inputs per node)
PM_MAX_PREDS = 4
TT_K = 3  # k = 4 at N = 512 would need 64 KiB of thresholds, past the 48 KiB kernel image

GOLDEN_R1 = [64, 192, 257, 384, 448, 512]  # r1_syn{N}.npz: the reference's Graph.step on pm_net(N)
GOLDEN_R4 = [64, 192, 320, 384, 448, 512]  # r4_ttk3_{N}.npz: the reference's PBN.step on tt_net(N)

# (family, kind, N) -> (error code, reason). A family that refuses a shape is asserted to refuse it with
# exactly this code; every entry cites the source line that imposes the limit. Nothing else is left out.
EXPECTED_REFUSALS = {}


def n_words(N):
    return (N + 63) // 64


@functools.lru_cache(maxsize=None)
def pm_net(N):
    from gym_pbn_amd.network import PredictorNetwork, synthetic_predictor_sets

    return PredictorNetwork.from_predictor_sets(*synthetic_predictor_sets(N, PM_MAX_PREDS, seed=N), name=f"syn{N}")


@functools.lru_cache(maxsize=None)
def tt_net(N):
    from gym_pbn_amd.network import TruthTableNetwork, synthetic_truth_table_pbn

    return TruthTableNetwork.from_pbn_data(synthetic_truth_table_pbn(N, TT_K, seed=N), name=f"ttk3_{N}")


def shape_net(kind, N):
    return pm_net(N) if kind == "pm" else tt_net(N)


def edge_nodes(N):
    """Node ``N - 1`` and the node on each side of every 64-bit boundary inside the state."""
    e = {N - 1}
    for b in range(64, N, 64):
        e.update((b - 1, b))
    return sorted(e)


def boundary_node(N):
    """The top bit of the last full word below node ``N - 1`` (node ``N // 2`` for a one-word state)."""
    return 64 * ((N - 1) // 64) - 1 if N > 64 else N // 2


def assert_edges_move(first, last, N, kind):
    """The coverage condition of a trajectory test, on the *oracle's* packed result: node ``N - 1`` and
    the nodes on both sides of every word boundary differ between ``first`` and ``last`` in some env."""
    d = np.asarray(first, np.uint64) ^ np.asarray(last, np.uint64)
    moved = np.bitwise_or.reduce(d.reshape(-1, d.shape[-1]), axis=0)
    for i in edge_nodes(N):
        if i == 0 and kind == "tt":
            continue
        assert (int(moved[i // 64]) >> (i % 64)) & 1, f"node {i} never changes: the case does not reach the edge"


def edge_attractors(rng, N, n_care=8):
    """``all_attractors`` of two attractors with two cubes each, like ``r6_cases.random_cubes`` but with a
    care bit forced onto node ``N - 1`` (cube 0) and onto the node on each side of a word boundary (cubes 1
    and 2; mid-word nodes for a one-word state); the other ``n_care - 1`` care bits of a cube are random."""
    b = boundary_node(N)
    forced = [N - 1, b, b + 1, None]
    cubes = []
    for f in forced:
        c = ["*"] * N
        pool = [i for i in range(N) if i != f]
        for j in rng.choice(pool, size=n_care - (f is not None), replace=False):
            c[int(j)] = int(rng.integers(0, 2))
        if f is not None:
            c[f] = int(rng.integers(0, 2))
        cubes.append(tuple(c))
    return [cubes[:2], cubes[2:]]


def edge_actions(rng, B, A, N, offset=1):
    """Action rows [B][A] (0 = none) that hit nodes 0, 63, 64 (where they exist) and ``N - 1`` in the first
    rows, duplicates included, random elsewhere with about half the slots empty."""
    a = rng.integers(offset, N + offset, size=(B, A)).astype(np.int32)
    a[rng.random((B, A)) < 0.5] = 0
    for r, node in enumerate([n for n in (0, 63, 64, N - 1) if n < N]):
        a[r, 0] = node + offset
        a[r, 1 % A] = node + offset if r % 2 else a[r, 1 % A]
    return a
