"""Writes tests/golden/fit_sep_n100_t250.npz: the separable fit (src/algs/separable.jl) of the reference's own test problem
(test/sep_test.jl: N=100, T=250, K=3, L=5, noise_level 0.1, thresh = 0.2 N - noise_level, pre=:svdcond), computed by the fp64
restatement tests/sep_restatement.py, for tests/test_sep_cpu.py and anyone who wants the numbers without numpy's RNG.

    python tests/golden/make_golden_sep.py

It re-runs sep_restatement.check_problem first: both modes take the same decisions, every decision margin is at least 1e-6 and
the NNLS step does not depend on the solver's tol.  Recorded: the case (N, T, K, L, noise, seed), thresh, the data, the sorted
vertices, the sorted groups, W, H, the loss and the literal-vs-rewritten floors.  Numbers only.  (Seed 1 passed at the first
try for every case of sep_restatement.CASES; no seed had to be replaced.)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import anls_restatement as A  # noqa: E402
import sep_restatement as S  # noqa: E402

if __name__ == "__main__":
    N, T, K, L, noise, _, seed = S.CASES["ref_noisy"]
    data, tW, tH, K, L, thresh = S.case_data("ref_noisy")
    ol, orw, floors, margins = S.check_problem("ref_noisy", data, K, L, thresh=thresh, pre=":svdcond")
    W, H = orw["W0"], orw["H0"]
    loss = np.linalg.norm(A.conv(W, H) - data) / np.linalg.norm(data)
    path = os.path.join(HERE, "fit_sep_n100_t250.npz")
    np.savez_compressed(path, case=np.array([N, T, K, L, noise, np.nan, seed]), thresh=thresh, data=data, vertices=np.array(orw["vertices"]),
                        groups=np.array(orw["groups"]), W=W, H=H, loss=loss, true_H=tH, floors=np.array([floors[k] for k in ("V", "G", "P", "W0", "H0")]))
    print(path, os.path.getsize(path), "bytes; loss", loss, "; least margins", {k: min(v) for k, v in margins["rewritten"].items()})
