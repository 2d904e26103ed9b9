#!/usr/bin/env python3
"""Writes tests/golden/mu_recentre_<name>.npz: the fp64 restatement of the MU rule with seqNMF's re-centring step
(tests/recentre_restatement.py: fit_mu_recentred) on the fixtures of recentre_restatement.FIXTURES, for the iteration counts
profiles/mu_recentre_precision.txt admits (tools/mu_recentre_precision.py).  Seeds and expected outputs only: the inputs are rebuilt from
the seeds by recentre_restatement.fixture_problem.  CPU only.

    python tools/mu_recentre_precision.py && python tests/golden/make_golden_recentre.py
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recentre_restatement as rr  # noqa: E402


def admitted():
    text = open(os.path.join(ROOT, "profiles", "mu_recentre_precision.txt")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^admit (\S+) (\d+)", text, re.M)}


def main():
    ok = admitted()
    for name, (N, T, K, L, seed, n_iter) in rr.FIXTURES.items():
        assert ok.get(name, 0) >= n_iter, f"{name}: {n_iter} iterations are not admitted ({ok.get(name)})"
        data, W0, H0, _ = rr.fixture_problem(name)
        r = rr.fit_mu_recentred(data, W0, H0, n_iter)
        path = os.path.join(HERE, f"mu_recentre_{name}.npz")
        np.savez_compressed(path, shape=np.array([N, T, K, L]), seed=seed, n_iter=n_iter, W=r["W"], H=r["H"], loss_hist=r["loss_hist"],
                            shifts=r["shifts"], moved=r["moved"])
        print(path, os.path.getsize(path), "bytes; moved", r["moved"].tolist())


if __name__ == "__main__":
    main()
