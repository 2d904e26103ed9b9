#!/usr/bin/env python3
"""Record what every request does to the MU rule in every form it can be in: tests/golden/mu_form_transitions.json.

    python3 tools/record_mu_transitions.py [out.json]

The walk is tests/mu_form_walk.py (the eight forms x the gate settings each can exist under x the requests, on a strictly positive
data set and on one that is valid only under the mask; from the plain square form also with gram = 1 or active cross-orthogonality
weights set first).  Per cell: [return code, form afterwards, data_dependent].  data_dependent marks the cells of the second data set
whose code differs from the first's: there the data check decided, not the handle's state.  Codes and names only: nothing in the file
depends on the card.  Run it on the commit whose behaviour is to be kept.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mu_form_walk as walk  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "mu_form_transitions.json")
    tables = {ds: walk.form_losses(ds) for ds in walk.DATA_SETS}
    assert len(tables["pos"]) == len(walk.NAMED)
    cells = {}
    for cell in walk.cells():
        rc, after = walk.walk_cell(cell, tables[cell[0]])
        assert after != "unknown", f"{walk.key(cell)}: the loss afterwards is that of no form"
        cells[walk.key(cell)] = [rc, after, False]
    for k, v in cells.items():
        if k.startswith("holed|"):
            v[2] = v[0] != cells["pos|" + k[len("holed|"):]][0]
    doc = {"problem": dict(N=walk.N, T=walk.T, K=walk.K, L=walk.L), "gates": list(walk.GATES),
           "key": "data set|start|form|gates|request", "value": "[return code, form afterwards, data_dependent]", "cells": cells}
    with open(out, "w") as f:
        f.write(json.dumps(doc, indent=0, separators=(",", ":")) + "\n")
    print(f"{len(cells)} cells, {sum(v[0] != 0 for v in cells.values())} refused, {sum(v[2] for v in cells.values())} data-dependent -> {out}")


if __name__ == "__main__":
    main()
