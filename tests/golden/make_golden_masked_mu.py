"""Generates the masked-MU fixtures in tests/golden/ (mu_masked_*.npz) from tests/masked_mu_restatement.py.

The shapes are those of the unmasked golden fits (their data and initial factors are read from mu_small.npz, mu_small_reg.npz and
mu_k5.npz), plus one with K > 32 and one with T < L on random inputs.  Every fixture holds the inputs, the mask, and W, H and
loss_hist of the fp64 restatement.

Run from the repo root:  python tests/golden/make_golden_masked_mu.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import masked_mu_restatement as mr  # noqa: E402


def write(name, data, W0, H0, mask, max_itr, reg):
    W, H, lh = mr.fit_masked(data, mask, W0, H0, max_itr=max_itr, **reg)
    r = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
    r.update(reg)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), data=data, mask=mask, W0=W0, H0=H0, W=W, H=H, loss_hist=lh, max_itr=max_itr, **r)
    print(name, data.shape, "held out", 1.0 - mask.mean(), "loss", lh[0], "->", lh[-1])


def main():
    for src, name, frac, block in (("mu_small", "mu_masked_small", 0.2, None), ("mu_small_reg", "mu_masked_small_reg", 0.2, None),
                                   ("mu_k5", "mu_masked_k5", 0.5, 1)):
        g = np.load(os.path.join(HERE, src + ".npz"))
        K, N, L = g["W0"].shape
        T = g["data"].shape[1]
        mask = mr.block_mask(N, T, frac, L if block is None else block, seed=21)
        reg = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H") if float(g[k]) != 0.0}
        write(name, g["data"], g["W0"], g["H0"], mask, int(g["max_itr"]), reg)
    for name, (N, T, K, L), itr in (("mu_masked_k33", (37, 150, 33, 7), 10), ("mu_masked_short", (6, 3, 2, 5), 10)):
        rng = np.random.default_rng(5)
        W0, H0, data = rng.random((K, N, L)), rng.random((K, T)), rng.random((N, T))
        mask = mr.block_mask(N, T, 0.2, min(L, T), seed=22) if T >= L else np.array(
            [[1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 1.0]])
        write(name, data, W0, H0, mask, itr, {})


if __name__ == "__main__":
    main()
