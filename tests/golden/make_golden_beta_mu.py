"""Generates the beta-divergence MU fixtures in tests/golden/ (mu_beta_*.npz) from tests/beta_mu_restatement.py.

The shapes are those of the KL and Itakura-Saito fixtures, on count data (kl_mu_restatement.count_problem: uint8 counts with exact
zeros and one all-zero unit, float16 initial factors -- what lets them stay within the 250 KB of a golden file): the small shape
without and with all four regularisers, K = 5 (few components), K = 33, K = 32, T < L and L = 40, each at beta = 0.5 and 1.5; the
small and the T < L shape also at beta = 0.25, 2 and 3 (both non-unit step exponents and the unit one).  Every fixture holds the
inputs, beta, the regularisers, and W, H and loss_hist of the fp64 restatement after max_itr iterations.  Where W and H would not fit
in fp64 the fixture holds them rounded to float32 (W32, H32: 6e-8 relative, against a bar of 1e-4) or, for K = 32, their Frobenius
norms, and beta_mu_restatement.load_fixture recomputes W and H from the stored inputs and checks them against loss_hist and the norms.

The iteration counts are the ones profiles/mu_beta_precision.txt admits (tools/mu_beta_precision.py, which reads CASES below): 100
where a shape asks for it and the profile admits it, 20 otherwise.

Run from the repo root:  python tools/mu_beta_precision.py && python tests/golden/make_golden_beta_mu.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import beta_mu_restatement as br  # noqa: E402

REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)  # (the regularisers of mu_small_reg.npz)
# name, (N, T, K, L), regularisers, how W and H are stored, the count asked for
SHAPES = [("small", (48, 300, 4, 8), {}, False, 100), ("small_reg", (48, 300, 4, 8), REG, False, 20),
          ("k5", (70, 257, 5, 10), {}, False, 100), ("k33", (70, 300, 33, 6), {}, True, 20),
          ("k32", (96, 1000, 32, 12), {}, "norms", 20), ("short", (20, 7, 2, 10), {}, False, 20),
          ("l40", (45, 130, 16, 40), {}, True, 20)]
BETAS_ALL = (0.5, 1.5)
BETAS_MORE = (0.25, 2.0, 3.0)  # on the shapes of MORE only
MORE = ("small", "short")


def tag(beta):
    return f"b{int(round(beta * 100)):03d}"


# name, shape name, beta
CASES = [(f"mu_beta_{s}_{tag(b)}", s, b) for s, *_ in SHAPES for b in BETAS_ALL + (BETAS_MORE if s in MORE else ())]


def shape_row(shape_name):
    for row in SHAPES:
        if row[0] == shape_name:
            return row
    raise KeyError(shape_name)


def inputs(shape_name):
    _, shape, reg, _, _ = shape_row(shape_name)
    return br.count_problem(*shape, seed=5) + (reg,)


def admitted():
    out = {}
    for line in open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "mu_beta_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


def write(name, data, W0, H0, beta, max_itr, reg, round32=False):
    W, H, lh = br.fit_beta(np.asarray(data, dtype=np.float64), np.asarray(W0, dtype=np.float64), np.asarray(H0, dtype=np.float64), beta,
                           max_itr=max_itr, **reg)
    r = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
    r.update(reg)
    out = (dict(W_norm=np.linalg.norm(W), H_norm=np.linalg.norm(H)) if round32 == "norms"
           else dict(W32=W.astype(np.float32), H32=H.astype(np.float32)) if round32 else dict(W=W, H=H))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, data=data, W0=W0, H0=H0, loss_hist=lh, max_itr=max_itr, beta=beta, **out, **r)
    print(name, data.shape, "K, N, L =", W0.shape, "zeros", f"{np.mean(data == 0):.2f}", "loss", lh[0], "->", lh[-1], os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 250_000


def main():
    adm = admitted()
    for name, s, beta in CASES:
        _, _, _, r32, want = shape_row(s)
        data, W0, H0, reg = inputs(s)
        itr = want if adm[name] >= want else 20
        assert adm[name] >= itr, f"profiles/mu_beta_precision.txt admits only {adm[name]} iterations on {name}"
        write(name, data, W0, H0, beta, itr, reg, round32=r32)


if __name__ == "__main__":
    main()
