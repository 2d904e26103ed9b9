"""Writes tests/golden/fit_admm_n40_t600_10.npz: ten outer iterations of the ADMM rule (src/algs/admm.jl, fit loop of
alternating.jl:44-67) computed by the fp64 restatement tests/admm_restatement.py, for tests/test_gpu_admm.py.

    python tests/golden/make_golden_admm.py

Besides the factors, loss_hist and the inner counts (W iters, W reverts, H iters, H reverts per outer iteration) it records the
smallest |diff - admm_tol| and |diff| over every revert / break decision of the fit: the test requires both to be at least 1e-7,
so that no decision the GPU has to reproduce is a tie."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import admm_restatement as R  # noqa: E402

N, T, K, L, ITERS, TOL = 40, 600, 4, 8, 10, 1e-4


def main(seed=7):
    rng = np.random.default_rng(seed)
    Wt = rng.random((K, N, L))
    Ht = rng.random((K, T)) * (rng.random((K, T)) < 0.2)
    data = R.conv(Wt, Ht) + 0.05 * rng.random((N, T))
    W0, H0 = rng.random((K, N, L)), rng.random((K, T))
    W, H = W0.copy(), H0.copy()
    loss_hist = [np.linalg.norm(R.conv(W, H) - data) / np.linalg.norm(data)]
    counts, m_tol, m_zero = [], np.inf, np.inf
    for _ in range(ITERS):
        tw, th = [], []
        W, _, wi, wr = R.update_motifs(data, H, L, tol=TOL, loss_trace=tw)
        H, loss, hi, hr = R.update_feature_maps(data, W, tol=TOL, loss_trace=th)
        for tr in (tw, th):
            a, b = R.decision_margins(tr, TOL)
            m_tol, m_zero = min(m_tol, a), min(m_zero, b)
        loss_hist.append(loss)
        counts.append((wi, wr, hi, hr))
    out = os.path.join(HERE, f"fit_admm_n{N}_t{T}_{ITERS}.npz")
    np.savez_compressed(out, data=data, W_init=W0, H_init=H0, W=W, H=H, loss_hist=np.array(loss_hist), counts=np.array(counts),
                        L=L, K=K, margin_tol=m_tol, margin_zero=m_zero)
    print(out, "counts", counts, "margins", m_tol, m_zero)


if __name__ == "__main__":
    main()
