#!/usr/bin/env python3
"""What a mask costs the HALS rule (library option "hals_mask"; profiles/hals_masked.txt): ms per HALS iteration (update_motifs +
update_feature_maps, call by call) at BASELINE config 5 (N=2000, T=50000, K=32, L=20) and at the shape of the reference's
loss-vs-time figure (N=250, T=50000, K=5, L=20), for five cases -- unmasked (the default hals_gram = 2), unmasked with hals_gram = 0
(both projections from the stored residual: what the masked form runs), an all-ones mask, 20 % held out in blocks of L, and the
last again with hals_chase = 0 (the masked residual conv in one launch behind the sweep instead of chasing it).  Two warm-up runs,
then the median, the smallest and the largest of 7 runs of `--iters` iterations each (the run's wall time divided by its iterations;
update_feature_maps returns when its loss has arrived).

    python3 tools/time_masked_hals.py [--iters N] [--shape config5|figure] [--out FILE]

Under `rocprofv3 --kernel-trace --stats -- python3 tools/time_masked_hals.py --shape config5` the per-kernel table says which kernel
carries the difference.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402

SHAPES = {"config5": (2000, 50000, 32, 20, 10), "figure": (250, 50000, 5, 20, 20)}


def run(rule, iters):
    for _ in range(iters):
        rule.update_motifs()
        rule.update_feature_maps()


def timed(rule, iters):
    for _ in range(2):
        run(rule, iters)
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        run(rule, iters)
        ts.append(1e3 * (time.perf_counter() - t0) / iters)
    return np.median(ts), min(ts), max(ts)


def main():
    which = [sys.argv[sys.argv.index("--shape") + 1]] if "--shape" in sys.argv else list(SHAPES)
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
    for name in which:
        N, T, K, L, iters = SHAPES[name]
        if "--iters" in sys.argv:
            iters = int(sys.argv[sys.argv.index("--iters") + 1])
        data = cmf.gen_synthetic(N=N, T=T, seed=1234)
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
        rule = cmf.HALSUpdate(data, W0, H0)
        rule.set_option("hals_mask", 1)
        held = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=5)
        base = None
        for case, mask, opts in (("unmasked (hals_gram = 2)", None, {}), ("unmasked, hals_gram = 0", None, {"hals_gram": 0}),
                                 ("all-ones mask", np.ones((N, T), order="F"), {}), ("20 % held out in blocks of L", held, {}),
                                 ("20 % held out, hals_chase = 0", held, {"hals_chase": 0})):
            rule.set_mask(mask)
            for k, v in dict({"hals_gram": 2, "hals_chase": -1}, **opts).items():
                rule.set_option(k, v)
            rule.upload(W0, H0)
            before = rule.counter("hals_masked_convs"), rule.counter("launches:conv3_chase_kernel")
            med, lo, hi = timed(rule, iters)
            n = 9 * iters
            line = (f"{name} N={N} T={T} K={K} L={L} | {case:<30} | ms/iteration median {med:.4f} min {lo:.4f} max {hi:.4f} "
                    f"({iters} iterations per run) | vs unmasked {100 * (med / (base or med) - 1):+.1f} % | per iteration: masked convs "
                    f"{(rule.counter('hals_masked_convs') - before[0]) / n:.2f}, chasing launches {(rule.counter('launches:conv3_chase_kernel') - before[1]) / n:.2f}, "
                    f"pipeline reruns so far {rule.counter('hals_pipeline_reruns')}")
            base = med if base is None else base
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        rule.close()


if __name__ == "__main__":
    main()
