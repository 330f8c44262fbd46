"""Fixture generator for attractor discovery on truth-table networks: ``attractors_tt_small.json``.

Build container only (it needs the reference checkout that ``refload`` loads, and networkx);
tests read the JSON and never import this file.

For each ``(n, k, det, seed)`` case the reference's own code gives the attractors of the ``"stg"``
graph: ``PBN(PBN_data).print_STG()`` (``common/pbn.py:132-199``, the async branch of
``_compute_next_states``) and networkx ``attracting_components`` -- which is
``PBNEnv.compute_attractors`` (``pbn_env.py:233-240``). The ``"step"`` graph (nodes ``1..n-1``
only, the graph ``PBN.step`` walks) has no reference function; its expected sets are built in
``tests/test_attractors_tt_host.py`` from the numpy restatement of the rule, and only their sizes
are recorded here (``step_sizes``) so that test can check it rebuilt the right thing.

Networks: every node gets ``k`` distinct inputs other than itself and a table whose entries are
0.0 with probability ``det``, 1.0 with probability ``det``, else uniform in [0, 1).

Run: ``python tests/golden/make_golden_tt_attractors.py`` from the repository root.
"""

from __future__ import annotations

import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

# (n, k, det, seed) -> attractor sizes of the "stg" graph (the reference must give them) and of the "step" graph
CASES = [
    ((8, 3, 0.47, 8), [1, 1], [1, 1, 1]),
    ((10, 3, 0.47, 1), [1, 1], [1, 1, 12, 12]),
    ((10, 3, 0.47, 5), [1, 2], [1, 1, 1]),
    ((10, 3, 0.40, 7), [32], [7, 15]),
    ((12, 3, 0.47, 8), [1, 1, 1], [1, 1, 1, 1]),
    ((12, 4, 0.47, 2), [1, 4], [1, 4, 2044]),
    ((12, 3, 0.47, 1), [3108], [4, 1504]),
]


def make_pbn_data(n, k, det, seed):
    """``PBN_DATA``: per node ``(input_mask, truth_table, name, is_control)``."""
    rng = np.random.default_rng(seed)
    data = []
    for i in range(n):
        inp = np.sort(rng.choice([j for j in range(n) if j != i], size=k, replace=False))
        u, v = rng.random(1 << k), rng.random(1 << k)
        table = np.where(u < det, 0.0, np.where(u < 2 * det, 1.0, v)).reshape((2,) * k)
        mask = np.zeros(n, dtype=bool)
        mask[inp] = True
        data.append((mask, table, f"n{i}", False))
    return data


def reference_attractors(pbn_mod, data):
    """``PBNEnv.compute_attractors`` on the reference's own STG: lists of state tuples, node 0 first."""
    import networkx as nx

    with contextlib.redirect_stdout(io.StringIO()):  # the constructor prints the network
        p = pbn_mod.PBN(PBN_data=data)
    stg = p.print_STG()
    out = []
    for comp in nx.algorithms.components.attracting_components(stg):
        out.append(sorted(tuple(int(x) for x in st.lstrip("[").rstrip("]").split()) for st in comp))
    return out


def step_attractor_sizes(data):
    """Sizes of the ``"step"`` graph's attractors: the reference's edge test with node 0 never moving."""
    import networkx as nx

    n = len(data)
    idx = np.arange(1 << n)
    bits = (idx[:, None] >> (n - 1 - np.arange(n))) & 1  # node 0 = most significant, as booleanize
    g = nx.DiGraph()
    g.add_nodes_from(idx.tolist())
    for i in range(1, n):
        mask, table = data[i][0], data[i][1]
        p = np.asarray(table)[tuple(bits[:, j] for j in np.nonzero(mask)[0])]
        move = ((p > 0.0) & (bits[:, i] == 0)) | ((p < 1.0) & (bits[:, i] == 1))
        src = idx[move]
        g.add_edges_from(zip(src.tolist(), (src ^ (1 << (n - 1 - i))).tolist()))
    return sorted(len(c) for c in nx.algorithms.components.attracting_components(g))


def main():
    import refload

    _, _, pbn_mod = refload.load_hot_path()
    out = {"format": "state = list of node values, node 0 first; tables in C order (first input = first axis)",
           "cases": []}
    for (n, k, det, seed), want_stg, want_step in CASES:
        data = make_pbn_data(n, k, det, seed)
        attractors = sorted(reference_attractors(pbn_mod, data), key=lambda a: (len(a), a[0][::-1]))
        sizes = [len(a) for a in attractors]
        assert sizes == want_stg, f"{(n, k, det, seed)}: reference sizes {sizes}, expected {want_stg}"
        step = step_attractor_sizes(data)
        assert step == want_step, f"{(n, k, det, seed)}: step-graph sizes {step}, expected {want_step}"
        out["cases"].append({
            "n_nodes": n, "k": k, "det": det, "seed": seed,
            "masks": [[int(b) for b in nd[0]] for nd in data],
            "tables": [[float(p) for p in np.asarray(nd[1]).reshape(-1)] for nd in data],
            "attractors": [[list(s) for s in a] for a in attractors],
            "step_sizes": want_step,
        })
        print((n, k, det, seed), "stg", sizes, "step", step, flush=True)
    (HERE / "attractors_tt_small.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main()
