"""Fixture generator for attractor discovery: ``attractors_small.json``.

Build container only (it needs the reference checkout that ``refload`` loads, networkx and scipy);
tests read the JSON and never import this file.

For each ``(N, max_preds, seed)`` case the reference's own code gives the attractors:
``base.Graph`` built by ``refload.build_graph`` from ``synthetic_predictor_sets`` (node IDs remapped
to ``0..N-1``: ``Node.getStateProbs`` indexes the state tuple by ID, ``base.py:75-77``), the loop of
``Graph.genSTG`` (``base.py:199-218``) with ``getNextStates(state=s)`` -- the no-argument call is the
line that fails at HEAD (``base.py:228``) -- and ``findAttractors`` (``base.py:398-399``).

Run: ``python tests/golden/make_golden_attractors.py`` from the repository root.
"""

from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1] / "gym-pbn-stac_amd"))

# (N, max_preds, seed) -> attractor sizes the reference must give
CASES = [
    ((8, 2, 6), [16, 32]),
    ((8, 2, 9), [8, 8]),
    ((8, 2, 2), [53]),
    ((10, 2, 0), [32, 128]),
    ((10, 2, 4), [640]),
    ((10, 2, 8), [2]),
    ((12, 3, 1), [128, 256]),
]


def remapped_sets(n, max_preds, seed):
    from gym_pbn_amd.network import synthetic_predictor_sets

    sets, ids = synthetic_predictor_sets(n, max_preds=max_preds, seed=seed)
    index_of = {int(g): i for i, g in enumerate(ids)}
    for ps in sets:
        for q in range(ps.shape[1]):
            ps[2, q] = [index_of[int(g)] for g in ps[2, q]]
    return sets, list(range(n))


def check_sign_rule(sets):
    """``getStateProbs`` decides with ``logistic.cdf(y) < 0.5``, ``Predstep`` with ``y < 0``."""
    from scipy.stats import logistic

    for ps in sets:
        for q in range(ps.shape[1]):
            A = np.asarray(ps[1, q], dtype=np.float64)
            for pat in itertools.product([0, 1], repeat=4):
                y = np.matmul(np.array(pat, dtype=np.float64).reshape(1, 4), A)
                assert bool(logistic.cdf(y) < 0.5) == bool(y < 0.0), (pat, float(y))


def reference_attractors(base, sets, ids):
    import networkx as nx
    import refload

    g = refload.build_graph(base, sets, ids)
    n = len(ids)
    stg = nx.DiGraph()
    stg.add_nodes_from(itertools.product([0, 1], repeat=n))
    for s in itertools.product([0, 1], repeat=n):  # genSTG's loop, base.py:208-214
        g.setState(s)
        for t in g.getNextStates(state=s):
            stg.add_edge(s, t)
    return [sorted(a) for a in base.findAttractors(stg)]


def main():
    import refload

    base, _, _ = refload.load_hot_path()
    out = {"format": "state = list of node values, node 0 first", "cases": []}
    for (n, max_preds, seed), want in CASES:
        sets, ids = remapped_sets(n, max_preds, seed)
        check_sign_rule(sets)
        attractors = sorted(reference_attractors(base, sets, ids), key=lambda a: (len(a), a[0][::-1]))
        sizes = [len(a) for a in attractors]
        assert sizes == want, f"{(n, max_preds, seed)}: reference sizes {sizes}, expected {want}"
        n_transient = (1 << n) - sum(sizes)
        if len(attractors) == 2:
            assert n_transient > 0, f"{(n, max_preds, seed)}: two attractors and no transient state"
        out["cases"].append({
            "n_nodes": n, "max_preds": max_preds, "seed": seed,
            "predictor_sets": [[[float(ps[0, q]), [float(v) for v in np.asarray(ps[1, q]).reshape(-1)],
                                 [int(v) for v in ps[2, q]]] for q in range(ps.shape[1])] for ps in sets],
            "attractors": [[list(s) for s in a] for a in attractors],
            "n_transient": n_transient,
        })
        print((n, max_preds, seed), sizes, "transient", n_transient, flush=True)
    (HERE / "attractors_small.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main()
