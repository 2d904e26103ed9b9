#!/usr/bin/env python3
"""What seqNMF's cross-orthogonality penalties cost against the plain squared-error MU rule (profiles/mu_xortho.txt): ms per
iteration of cmf_iterate at BASELINE config 2 (N=2000, T=50000, K=32, L=20) and at the shape of the reference's loss-vs-time figure
(N=250, T=50000, K=5, L=20), the plain rule, lambda alone and all three weights in the same run on the same handle, each from the same
initial factors.  The weights are small (1e-4): the cost does not depend on them, and the fit stays an ordinary one.  Two warm-up
runs, then the median, the smallest and the largest of 7 runs of `--iters` iterations each (the run's wall time divided by its
iterations; cmf_iterate returns when the last loss has arrived).  The last column counts the launches of the penalties' own kernels
per iteration (cmf_get_counter "xortho_launches").

    python3 tools/time_xortho_mu.py [--iters N] [--shape config2|figure]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402

SHAPES = {"config2": (2000, 50000, 32, 20, 20), "figure": (250, 50000, 5, 20, 200)}


def timed(rule, iters):
    for _ in range(2):
        rule.iterate(iters)
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        rule.iterate(iters)
        ts.append(1e3 * (time.perf_counter() - t0) / iters)
    return np.median(ts), min(ts), max(ts)


def main():
    which = [sys.argv[sys.argv.index("--shape") + 1]] if "--shape" in sys.argv else list(SHAPES)
    for name in which:
        N, T, K, L, iters = SHAPES[name]
        if "--iters" in sys.argv:
            iters = int(sys.argv[sys.argv.index("--iters") + 1])
        data = np.maximum(cmf.gen_synthetic(N=N, T=T, seed=1234), 0.0)
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
        rule = cmf.MultUpdate(data, W0, H0)
        base = None
        for case, weights in (("squared error", (0.0, 0.0, 0.0)), ("lambda", (1e-4, 0.0, 0.0)), ("lambda, lambda_H, lambda_W", (1e-4, 1e-4, 1e-4)),
                              ("squared error again", (0.0, 0.0, 0.0))):
            rule.set_xortho(*weights)
            rule.upload(W0, H0)
            before = rule.counter("xortho_launches")
            med, lo, hi = timed(rule, iters)
            per_it = (rule.counter("xortho_launches") - before) / (9 * iters)
            base = med if base is None else base
            print(f"{name} N={N} T={T} K={K} L={L} | {case:<28} | ms/iteration median {med:.4f} min {lo:.4f} max {hi:.4f} "
                  f"({iters} iterations per run) | vs squared error {100 * (med / base - 1):+.1f} % | {per_it:.0f} penalty launches per iteration",
                  flush=True)
        rule.close()


if __name__ == "__main__":
    main()
