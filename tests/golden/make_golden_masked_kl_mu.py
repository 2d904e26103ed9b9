"""Generates the masked KL-MU fixtures in tests/golden/ (mu_masked_kl_*.npz) from tests/masked_kl_mu_restatement.py.

Every fixture reuses the inputs (data, W0, H0) of the mu_kl_* fixture it names in `inputs` and stores only the mask (packed to
bits), the regularisers, max_itr, loss_hist and W and H of the fp64 restatement -- in fp64 where they fit the 250 KB of a golden
file, as float32 roundings (W32 / H32: 6e-8 relative, against a bar of 1e-4) for K = 33 and L = 40, and as Frobenius norms for
K = 32 (masked_kl_mu_restatement.load_fixture recomputes W and H there and checks them against loss_hist and the norms).  The fit
runs on data with NaN under mask == 0, which is also how the fixture is loaded.

    mu_kl_small      blocks of L                      mu_kl_k33    blocks + one unit and one sample never observed
    mu_kl_small_reg  blocks, all four regularisers    mu_kl_k32    blocks, 100 iterations
    mu_kl_k5         50 % speckle, 100 iterations     mu_kl_short  T < L, 5 iterations          mu_kl_l40  blocks

The iteration counts are ones profiles/mu_masked_kl_precision.txt admits (tools/mu_masked_kl_precision.py, which names the same
masks: FIXTURE_INPUTS there).

Run from the repo root:  python tests/golden/make_golden_masked_kl_mu.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import masked_kl_mu_restatement as mk  # noqa: E402

CASES = (("mu_masked_kl_small", "mu_kl_small", "blocks", False, 20, False), ("mu_masked_kl_small_reg", "mu_kl_small_reg", "blocks", True, 20, False),
         ("mu_masked_kl_k5", "mu_kl_k5", "speckle", False, 100, False), ("mu_masked_kl_k33", "mu_kl_k33", "dead", False, 20, True),
         ("mu_masked_kl_k32", "mu_kl_k32", "blocks", False, 100, "norms"), ("mu_masked_kl_short", "mu_kl_short", "blocks", False, 5, False),
         ("mu_masked_kl_l40", "mu_kl_l40", "blocks", False, 20, True))


def main():
    for name, src, kind, with_reg, itr, round32 in CASES:
        g = np.load(os.path.join(HERE, src + ".npz"))
        data, W0, H0 = (np.asarray(g[k], dtype=np.float64) for k in ("data", "W0", "H0"))
        K, N, L = W0.shape
        mask = mk.make_mask(kind, N, data.shape[1], L)
        reg = dict(mk.REG) if with_reg else dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
        W, H, lh = mk.fit_masked_kl(np.where(mask != 0, data, np.nan), mask, W0, H0, max_itr=itr, **reg)
        out = (dict(W_norm=np.linalg.norm(W), H_norm=np.linalg.norm(H)) if round32 == "norms"
               else dict(W32=W.astype(np.float32), H32=H.astype(np.float32)) if round32 else dict(W=W, H=H))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, inputs=src, mask_bits=np.packbits(mask.astype(np.uint8).ravel()), loss_hist=lh, max_itr=itr, **out, **reg)
        print(name, data.shape, "K, N, L =", W0.shape, "observed", float(mask.mean()), "loss", lh[0], "->", lh[-1], os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 250_000


if __name__ == "__main__":
    main()
