"""Is fp32 enough for the ADMM rule's contractions?  Runs the fp64 restatement (tests/admm_restatement.py) of five outer
iterations of src/algs/admm.jl twice on one problem -- as written, and with the three contraction kinds (Gram, Hstk*X /
transconvolution, convolutions) rounded to fp32 while every solve stays fp64 -- and prints W, H and loss differences, the inner
iteration counts and reverts of every call, and cond(G) of every W call.  Output committed as profiles/admm_precision.txt.

    python tools/admm_precision.py [N T K L]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import admm_restatement as R  # noqa: E402


def f32(x):
    return x.astype(np.float32).astype(np.float64)


def run(data, W0, H0, contract, iters):
    W, H, L = W0.copy(), H0.copy(), W0.shape[2]
    rows = []
    for _ in range(iters):
        st = {}
        W, _, wi, wr = R.update_motifs(data, H, L, contract=contract, stats=st)
        H, loss, hi, hr = R.update_feature_maps(data, W, contract=contract)
        rows.append((W.copy(), H.copy(), loss, wi, wr, hi, hr, st["cond_G"]))
    return rows


def main():
    N, T, K, L = (int(a) for a in sys.argv[1:5]) if len(sys.argv) > 4 else (200, 8000, 8, 10)
    rng = np.random.default_rng(0)
    Wt = rng.random((K, N, L))
    Ht = rng.random((K, T)) * (rng.random((K, T)) < 0.1)
    data = R.conv(Wt, Ht) + 0.1 * rng.random((N, T))
    W0, H0 = rng.random((K, N, L)), rng.random((K, T))
    t0 = time.time()
    a = run(data, W0, H0, None, 5)
    b = run(data, W0, H0, f32, 5)
    print(f"ADMM rule, N={N} T={T} K={K} L={L}, 5 outer iterations from one random start (seed 0), restatement in fp64 vs the same")
    print("with every contraction result rounded to fp32 (solves, FFT, element-wise steps in fp64).  rel = Frobenius-relative.")
    print(f"{'itr':>3} {'cond(G) fp64':>13} {'relW':>10} {'relH':>10} {'|dloss|':>10}  {'fp64 Wit/rev Hit/rev':>21}  {'fp32 Wit/rev Hit/rev':>21}")
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    for i, (ra, rb) in enumerate(zip(a, b)):
        print(f"{i + 1:>3} {ra[7]:>13.3e} {rel(rb[0], ra[0]):>10.2e} {rel(rb[1], ra[1]):>10.2e} {abs(rb[2] - ra[2]):>10.2e}  "
              f"{'%d/%d %d/%d' % ra[3:7]:>21}  {'%d/%d %d/%d' % rb[3:7]:>21}")
    print(f"({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
