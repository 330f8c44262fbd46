"""Fixture generator for the exact transition graph: ``stg_small.json``.

Build container only (it needs the reference checkout that ``refload`` loads and scipy); tests read the JSON and never
import this file.

For two of the golden nets of ``attractors_small.json`` the reference's own ``Graph.getNextStates``
(``base.py:221-242``) gives ``{next_state: prob}`` for every one of the ``2**N`` states: ``base.Graph`` built by
``refload.build_graph`` from the same remapped predictor sets ``make_golden_attractors.py`` uses, ``setState(s)`` and
``getNextStates(state=s)`` as ``genSTG``'s loop does (``base.py:208-214``; the no-argument call is the line that fails
at HEAD, ``base.py:228``). Only the recorded dict is kept: ``[state, next_state, prob]`` with both states as integers
(node ``i`` = bit ``i``) and ``prob`` the reference's double, which JSON round-trips exactly.

Run: ``python tests/golden/make_golden_stg.py`` from the repository root.
"""

from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1] / "gym-pbn-stac_amd"))

CASES = [(8, 2, 6), (10, 2, 0)]  # (N, max_preds, seed): cases of attractors_small.json


def as_int(state):
    return sum(int(v) << i for i, v in enumerate(state))


def main():
    import refload
    from make_golden_attractors import check_sign_rule, remapped_sets

    base, _, _ = refload.load_hot_path()
    out = {"format": "edges: [state, next_state, prob]; a state is an integer, node i = bit i; prob is "
                     "Graph.getNextStates' value (the stay mass is the entry state == next_state)",
           "cases": []}
    for n, max_preds, seed in CASES:
        sets, ids = remapped_sets(n, max_preds, seed)
        check_sign_rule(sets)
        g = refload.build_graph(base, sets, ids)
        edges = []
        for s in itertools.product([0, 1], repeat=n):
            g.setState(s)
            for t, p in g.getNextStates(state=s).items():
                edges.append([as_int(s), as_int(t), float(p)])
        edges.sort(key=lambda e: (e[0], e[1]))
        out["cases"].append({"n_nodes": n, "max_preds": max_preds, "seed": seed, "edges": edges})
        print((n, max_preds, seed), len(edges), "edges", flush=True)
    (HERE / "stg_small.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main()
