#!/usr/bin/env python3
"""What one null draw of seqNMF's significance test costs (profiles/significance.txt): ms per draw of cmf_null_moments at BASELINE
config 2 (N=2000, T=50000, K=32, L=20) and at the shape of the reference's loss-vs-time figure (N=250, T=50000, K=5, L=20), against
what a draw would cost through the rule's own kernels: the same handle's one-source transconv launch plus its slab sum.  Both are timed
in the same run with HIP events on the handle's stream (cmf_time_kernel "signif_draw": one default batch of draws -- shift table,
contraction with the moments epilogue, reduction over the t blocks -- divided by the draws of the batch; "transconv1_sum").  Five
measurements of `--reps` repetitions each, alternating; the median, the smallest and the largest.  The last lines time whole calls of
cmf_null_moments from the host (wall clock, the read-back of the sums included) for the default number of draws 2 ceil(K / 0.05), at
the default batch and at eight times as many draws per batch.

    python3 tools/time_significance.py [--reps N] [--shape config2|figure]
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402

SHAPES = {"config2": (2000, 50000, 32, 20), "figure": (250, 50000, 5, 20)}


def main():
    which = [sys.argv[sys.argv.index("--shape") + 1]] if "--shape" in sys.argv else list(SHAPES)
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    for name in which:
        N, T, K, L = SHAPES[name]
        data = np.maximum(cmf.gen_synthetic(N=N, T=T, seed=1234), 0.0)
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
        rule = cmf.MultUpdate(data, W0, H0)
        try:
            m = 32 // math.gcd(K, 32)
            batch = m * -(-256 // (K * m))
            ts = {"signif_draw": [], "transconv1_sum": []}
            flops = 0.0
            for _ in range(5):
                for kname in ts:
                    ms, flops = rule.time_kernel(kname, reps)
                    ts[kname].append(ms)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            for kname, v in ts.items():
                print(f"{name} N={N} T={T} K={K} L={L} | {kname:<14} | ms median {med[kname]:.4f} min {min(v):.4f} max {max(v):.4f} "
                      f"({reps} repetitions per measurement) | {flops / med[kname] / 1e9:.1f} TFLOP/s of 2 K N S", flush=True)
            small = "transconv_kernel" if rule.counter(f"launches:transconv_kernel<{min(32, -(-L // 4) * 4)}>") > 0 else "few-component C3 form"
            print(f"{name} | draws per batch {batch} ({batch * K} columns in {-(-batch * K // 32)} blocks of 32) | the rule's C3 launch is the {small} | "
                  f"draw / (transconv + slab sum) = {med['signif_draw'] / med['transconv1_sum']:.3f}", flush=True)
            nnull = 2 * math.ceil(K / 0.05)
            for b in (batch, 8 * batch):  # (the default, and eight times as many columns per launch: more pairs per resident wave)
                rule.set_option("signif_batch", b)
                rule.null_moments(0, 0, b)
                t0 = time.perf_counter()
                rule.null_moments(0, 0, 1 + nnull)
                wall = time.perf_counter() - t0
                print(f"{name} | cmf_null_moments, {1 + nnull} draws, signif_batch {b}: {1e3 * wall:.1f} ms wall ({1e3 * wall / (1 + nnull):.4f} ms per draw)", flush=True)
        finally:
            rule.close()


if __name__ == "__main__":
    main()
