#!/usr/bin/env python3
"""What seqNMF's re-centring step costs inside the MU iteration (profiles/mu_recentre.txt): ms per cmf_iterate iteration with and without
cmf_mu_set_recentre, at BASELINE config 2 (N=2000, T=50000, K=32, L=20) and at the shape of the reference's loss-vs-time figure
(N=250, T=50000, K=5, L=20).  Both are timed in the same run on the same handle, alternating: two warm-up batches, then seven
measurements each of `--iters` iterations in one cmf_iterate call (wall clock around the call: the batch is pipelined, the host only
waits for the last loss); the median, the smallest and the largest.

Two states per shape:
  steady   the fit has run 30 iterations with the step on: nearly every step decides for all-zero shifts and moves no data
  forced   cmf_recentre_shifts of the resident W is all zero, and the motifs are then displaced by two lags on the host (with H moved to
           match) before every measurement of ONE iteration: the step of that iteration moves every component back

    python3 tools/time_recentre_mu.py [--iters N] [--shape config2|figure]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402

SHAPES = {"config2": (2000, 50000, 32, 20), "figure": (250, 50000, 5, 20)}


def timed(rule, n):
    rule.synchronize()
    t0 = time.perf_counter()
    rule.iterate(n)
    return 1e3 * (time.perf_counter() - t0) / n


def line(name, what, ts):
    med = {k: float(np.median(v)) for k, v in ts.items()}
    print(f"{name} | {what} | ms per iteration: off median {med[0]:.4f} min {min(ts[0]):.4f} max {max(ts[0]):.4f} | on median {med[1]:.4f} "
          f"min {min(ts[1]):.4f} max {max(ts[1]):.4f} | step {med[1] - med[0]:+.4f} ms ({100 * (med[1] / med[0] - 1):+.2f} %)", flush=True)


def main():
    which = [sys.argv[sys.argv.index("--shape") + 1]] if "--shape" in sys.argv else list(SHAPES)
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    for name in which:
        N, T, K, L = SHAPES[name]
        data = np.maximum(cmf.gen_synthetic(N=N, T=T, seed=1234), 0.0)
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
        rule = cmf.MultUpdate(data, W0, H0)
        try:
            rule.set_recentre(True)
            rule.iterate(30)
            ts = {0: [], 1: []}
            for rep in range(2 + 7):  # two warm-ups, seven measurements, alternating
                for on in (0, 1):
                    rule.set_recentre(on)
                    ms = timed(rule, iters)
                    if rep >= 2:
                        ts[on].append(ms)
            moved = int(rule.recentre_info()[1].sum())
            line(f"{name} N={N} T={T} K={K} L={L}", f"steady state, {iters} iterations per call (sum of |s_k| since the start: {moved})", ts)
            launches = rule.counter("recentre_launches")
            # forced: displace every motif by two lags on the host, then time ONE iteration whose step moves them back
            ts = {0: [], 1: []}
            W, H = rule.download()
            W, H, _ = cmf.recentre(W, H)
            floor = float(np.finfo(np.float64).eps)
            Wd, Hd = np.full_like(W, floor), np.full_like(H, floor)
            Wd[:, :, 2:] = W[:, :, :-2]
            Hd[:, :-2] = H[:, 2:]
            for rep in range(2 + 7):
                for on in (0, 1):
                    rule.upload(Wd, Hd)
                    rule.set_recentre(on)
                    ms = timed(rule, 1)
                    if rep >= 2:
                        ts[on].append(ms)
                    if on:
                        last = rule.recentre_info()[0]
            line(f"{name} N={N} T={T} K={K} L={L}", f"forced shift, ONE iteration per call (last shifts: {np.bincount(np.abs(last)).tolist()} components by |s_k|)", ts)
            print(f"{name} | recentre_launches {launches} -> {rule.counter('recentre_launches')}", flush=True)
        finally:
            rule.close()


if __name__ == "__main__":
    main()
