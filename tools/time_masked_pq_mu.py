#!/usr/bin/env python3
"""What the Itakura-Saito and beta forms cost under a mask (profiles/mu_pq_masked.txt): ms per iteration of cmf_iterate at BASELINE
config 2 (N=2000, T=50000, K=32, L=20) and at the shape of the reference's loss-vs-time figure (N=250, T=50000, K=5, L=20) for
Itakura-Saito, beta = 0.5 and beta = 1.5, each unmasked and then under a mask (20 % held out in blocks of L), all on one handle in
one run (the synthetic data clipped at a small positive floor, which Itakura-Saito needs).  Two warm-up runs, then the median, the
smallest and the largest of 7 runs of `--iters` iterations each (the run's wall time divided by its iterations; cmf_iterate returns
when the last loss has arrived).

    python3 tools/time_masked_pq_mu.py [--iters N] [--shape config2|figure]

Under `rocprofv3 --kernel-trace --stats -- python3 tools/time_masked_pq_mu.py --shape figure --iters 50` the per-kernel table says
which launch carries a difference.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402

SHAPES = {"config2": (2000, 50000, 32, 20, 20), "figure": (250, 50000, 5, 20, 200)}
FORMS = (("Itakura-Saito", ":itakura_saito", None), ("beta = 0.5", ":beta", 0.5), ("beta = 1.5", ":beta", 1.5))


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
        data = np.maximum(cmf.gen_synthetic(N=N, T=T, seed=1234), 1e-3)
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
        mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=1)
        rule = cmf.MultUpdate(data, W0, H0)
        rule.set_option("pq_mask", 1)
        for form, kind, beta in FORMS:
            base = None
            for case, m in ((form, None), ("masked " + form, mask)):
                rule.set_mask(m)
                rule.set_divergence(kind, beta=beta)
                rule.upload(W0, H0)
                med, lo, hi = timed(rule, iters)
                base = med if base is None else base
                print(f"{name} N={N} T={T} K={K} L={L} | {case:<20} | ms/iteration median {med:.4f} min {lo:.4f} max {hi:.4f} "
                      f"({iters} iterations per run) | vs unmasked {100 * (med / base - 1):+.1f} %", flush=True)
        rule.close()


if __name__ == "__main__":
    main()
