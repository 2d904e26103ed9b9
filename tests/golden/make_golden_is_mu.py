"""Generates the Itakura-Saito MU fixtures in tests/golden/ (mu_is_*.npz) from tests/is_mu_restatement.py.

The shapes are those of the KL fixtures (mu_kl_*.npz), on strictly positive data (is_mu_restatement.positive_problem: uint8 values
in 1 .. 255, float16 initial factors -- what lets them stay within the 250 KB of a golden file): the small shape without and with all
four regularisers, K = 5 (few components), K = 33, K = 32, T < L and L = 40.  Every fixture holds the inputs, the regularisers, and W,
H and loss_hist of the fp64 restatement after max_itr iterations.  Where W and H would not fit in fp64 the fixture holds them rounded
to float32 (W32, H32: 6e-8 relative, against a bar of 1e-4) or, for K = 32, their Frobenius norms, and
is_mu_restatement.load_fixture recomputes W and H from the stored inputs and checks them against loss_hist and the norms.

The iteration counts are the ones profiles/mu_is_precision.txt admits (tools/mu_is_precision.py, which reads CASES below): 100 where
WANT asks for it and the profile admits it, 20 otherwise.

Run from the repo root:  python tools/mu_is_precision.py && python tests/golden/make_golden_is_mu.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import is_mu_restatement as ir  # noqa: E402

REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)  # (the regularisers of mu_small_reg.npz)
# name, (N, T, K, L), regularisers, how W and H are stored, the count asked for
CASES = [("mu_is_small", (48, 300, 4, 8), {}, False, 100), ("mu_is_small_reg", (48, 300, 4, 8), REG, False, 20),
         ("mu_is_k5", (70, 257, 5, 10), {}, False, 100), ("mu_is_k33", (70, 300, 33, 6), {}, True, 20),
         ("mu_is_k32", (96, 1000, 32, 12), {}, "norms", 20), ("mu_is_short", (20, 7, 2, 10), {}, False, 20),
         ("mu_is_l40", (45, 130, 16, 40), {}, True, 20)]


def inputs(name):
    for n, shape, reg, _, _ in CASES:
        if n == name:
            return ir.positive_problem(*shape, seed=5) + (reg,)
    raise KeyError(name)


def admitted():
    out = {}
    for line in open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "mu_is_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


def write(name, data, W0, H0, max_itr, reg, round32=False):
    W, H, lh = ir.fit_is(np.asarray(data, dtype=np.float64), np.asarray(W0, dtype=np.float64), np.asarray(H0, dtype=np.float64),
                         max_itr=max_itr, **reg)
    r = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
    r.update(reg)
    out = (dict(W_norm=np.linalg.norm(W), H_norm=np.linalg.norm(H)) if round32 == "norms"
           else dict(W32=W.astype(np.float32), H32=H.astype(np.float32)) if round32 else dict(W=W, H=H))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, data=data, W0=W0, H0=H0, loss_hist=lh, max_itr=max_itr, **out, **r)
    print(name, data.shape, "K, N, L =", W0.shape, "min", int(np.min(data)), "loss", lh[0], "->", lh[-1], os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 250_000


def main():
    adm = admitted()
    for name, _, _, r32, want in CASES:
        data, W0, H0, reg = inputs(name)
        itr = want if adm[name] >= want else 20
        assert adm[name] >= itr, f"profiles/mu_is_precision.txt admits only {adm[name]} iterations on {name}"
        write(name, data, W0, H0, itr, reg, round32=r32)


if __name__ == "__main__":
    main()
