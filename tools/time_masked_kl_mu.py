#!/usr/bin/env python3
"""What the KL form costs under a mask (profiles/mu_masked_kl.txt): ms per iteration of cmf_iterate at BASELINE config 2 (N=2000,
T=50000, K=32, L=20) and at the shape of the reference's loss-vs-time figure (N=250, T=50000, K=5, L=20) for the unmasked KL rule,
the masked squared-error rule and the masked KL rule (20 % held out in blocks of L), all on one handle in one run (the synthetic
data clipped at 0, which the KL rule needs).  Two warm-up runs, then the median, the smallest and the largest of 7 runs of
`--iters` iterations each (the run's wall time divided by its iterations; cmf_iterate returns when the last loss has arrived).

    python3 tools/time_masked_kl_mu.py [--iters N] [--shape config2|figure]

Under `rocprofv3 --kernel-trace --stats -- python3 tools/time_masked_kl_mu.py --shape figure --iters 50` the per-kernel table says
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
        mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=1)
        rule = cmf.MultUpdate(data, W0, H0)
        rule.set_option("kl_mask", 1)
        base = None
        for case, kind, m in (("KL", ":kl", None), ("masked squared error", ":square", mask), ("masked KL", ":kl", mask),
                              ("KL again", ":kl", None)):
            if m is None:  # (the order keeps every intermediate state one the library accepts)
                rule.set_mask(None)
                rule.set_divergence(kind)
            else:
                rule.set_divergence(kind)
                rule.set_mask(m)
            rule.upload(W0, H0)
            med, lo, hi = timed(rule, iters)
            base = med if base is None else base
            print(f"{name} N={N} T={T} K={K} L={L} | {case:<20} | ms/iteration median {med:.4f} min {lo:.4f} max {hi:.4f} "
                  f"({iters} iterations per run) | vs KL {100 * (med / base - 1):+.1f} %", flush=True)
        rule.close()


if __name__ == "__main__":
    main()
