"""Generates the KL-MU fixtures in tests/golden/ (mu_kl_*.npz) from tests/kl_mu_restatement.py.

Three reuse the inputs of the squared-error golden fits (data and initial factors are read from mu_small.npz, mu_small_reg.npz --
with all four regularisers -- and mu_k5.npz; their data are non-negative with exact zeros).  Four more cover K = 33, K = 32, T < L
and L = 40 on count data (kl_mu_restatement.count_problem: uint8 counts, float16 initial factors -- what lets them stay within the
250 KB of a golden file).  Every fixture holds the inputs, the regularisers, and W, H and loss_hist of the fp64 restatement after
max_itr iterations.  Three cannot hold W and H in fp64 within the size: the K = 33 and L = 40 fixtures hold them rounded to float32 (W32, H32:
6e-8 relative, against a bar of 1e-4); the K = 32 fixture (69 000 factor entries) holds their Frobenius norms, and
kl_mu_restatement.load_fixture recomputes W and H from the stored inputs and checks them against loss_hist and the norms.

The iteration counts are the ones profiles/mu_kl_precision.txt admits (tools/mu_kl_precision.py).

Run from the repo root:  python tests/golden/make_golden_kl_mu.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kl_mu_restatement as kr  # noqa: E402


def write(name, data, W0, H0, max_itr, reg, round32=False):
    W, H, lh = kr.fit_kl(np.asarray(data, dtype=np.float64), np.asarray(W0, dtype=np.float64), np.asarray(H0, dtype=np.float64),
                         max_itr=max_itr, **reg)
    r = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
    r.update(reg)
    out = (dict(W_norm=np.linalg.norm(W), H_norm=np.linalg.norm(H)) if round32 == "norms"
           else dict(W32=W.astype(np.float32), H32=H.astype(np.float32)) if round32 else dict(W=W, H=H))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, data=data, W0=W0, H0=H0, loss_hist=lh, max_itr=max_itr, **out, **r)
    print(name, data.shape, "K, N, L =", W0.shape, "zeros", float((np.asarray(data) == 0).mean()), "loss", lh[0], "->", lh[-1],
          os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 250_000


def main():
    for src, name, itr in (("mu_small", "mu_kl_small", 100), ("mu_small_reg", "mu_kl_small_reg", 20), ("mu_k5", "mu_kl_k5", 100)):
        g = np.load(os.path.join(HERE, src + ".npz"))
        reg = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H") if float(g[k]) != 0.0}
        write(name, g["data"], g["W0"], g["H0"], itr, reg)
    for name, (N, T, K, L), itr, r32 in (("mu_kl_k33", (70, 300, 33, 6), 20, True), ("mu_kl_k32", (96, 1000, 32, 12), 20, "norms"),
                                        ("mu_kl_short", (20, 7, 2, 10), 20, False), ("mu_kl_l40", (45, 130, 16, 40), 20, True)):
        data, W0, H0 = kr.count_problem(N, T, K, L, seed=5)
        write(name, data, W0, H0, itr, {}, round32=r32)


if __name__ == "__main__":
    main()
