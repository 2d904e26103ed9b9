#!/usr/bin/env python3
"""The ANLS rule (src/algs/anls.jl) at the shape of the reference's loss-vs-time figure (N=250, T=50000, K=5, L=20,
figures/fast_bcd/synthetic_comparison.jl:58-67) on one GPU: update_motifs! and update_feature_maps! in both variants, each
call timed on the host clock (the calls synchronise) -- two warm-up calls, then REPS timed ones on the same inputs; the median,
the smallest and the largest are printed, with the pivoting rounds of the call.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel table (profiles/anls_fig_shape.txt has both).

    python3 tools/time_anls.py [--restatement] [--reps N] [--backup-only]
    python3 tools/time_anls.py --kernel-table <rocprofv3 dir>/<name>_kernel_stats.csv

--backup-only sets cmf_set_option "anls_backup_only": every exchange moves one index, so the same answers take more pivoting
rounds; the two runs together split a call's time into a part per round and a part per problem.

--restatement also times the fp64 numpy restatement (tests/anls_restatement.py, Gram mode) of the same calls on the CPU
(OMP_NUM_THREADS sets its BLAS threads; its sweep along T is a Python loop)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def kernel_table(path):
    import csv
    import re

    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "anls" not in name and "fp64" not in name:
            continue
        m = re.search(r"fp64_gemm_kernel<\w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)", name)
        short = (f"contraction {m.group(1)} x {m.group(2)} -> {m.group(3)}" if m
                 else re.sub(r"\(.*", "", name).replace("void ", "").replace("anls::", "").replace("fp64::", ""))
        rows.append((short, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e6))
    tot = sum(r[2] for r in rows)
    print(f"{'kernel':<62} {'calls':>6} {'total ms':>9} {'avg ms':>8} {'share':>6}")
    for r in sorted(rows, key=lambda r: -r[2]):
        print(f"{r[0]:<62} {r[1]:>6} {r[2]:>9.2f} {r[3]:>8.3f} {100 * r[2] / tot:>5.1f}%")
    print(f"{'total':<62} {'':>6} {tot:>9.2f}")


def timed(f, reps):
    for _ in range(2):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return np.median(ts), min(ts), max(ts)


def main():
    if "--kernel-table" in sys.argv:
        return kernel_table(sys.argv[sys.argv.index("--kernel-table") + 1])
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    import anls_restatement as R
    import cmf_jl_amd as cmf

    N, T, K, L = R.FIG
    data, W0, H0 = R.problem(N, T, K, L, seed=100)
    t0 = time.perf_counter()
    rule = cmf.ANLSUpdate(data, W0, H0)
    print(f"figure shape (N={N} T={T} K={K} L={L}), fp64; ANLSUpdate construction (cmf_create + cmf_anls_prepare): "
          f"{1e3 * (time.perf_counter() - t0):.1f} ms; {reps} timed calls after 2 warm-up calls: median [min .. max]")
    try:
        if "--backup-only" in sys.argv:
            rule.set_option("anls_backup_only", 1)
            print("anls_backup_only = 1")
        W = W0.copy(order="F")
        med, lo, hi = timed(lambda: rule.update_motifs(data, W, H0), reps)
        print(f"update_motifs!                     : {med:8.2f} ms [{lo:.2f} .. {hi:.2f}]  pivoting rounds {rule.last_W_exchanges} over {N} problems "
              f"of {K * L} unknowns", flush=True)
        for v in ("basic", "block"):
            H = H0.copy(order="F")

            def call():
                H[...] = H0
                return rule.update_feature_maps(data, W, H, variant=v)

            med, lo, hi = timed(call, reps)
            print(f"update_feature_maps! variant=:{v:5s} : {med:8.2f} ms [{lo:.2f} .. {hi:.2f}]  pivoting rounds {rule.last_H_exchanges} over {T} "
                  f"columns ({1e3 * med / T:.2f} us per column)  loss {call():.6f}", flush=True)
    finally:
        rule.close()
    if "--restatement" in sys.argv:
        out = []
        t0 = time.perf_counter()
        Wr = R.update_motifs(data, H0, L)
        out.append(f"update_motifs! {time.perf_counter() - t0:.2f} s")
        for v in ("basic", "block"):
            t0 = time.perf_counter()
            R.update_feature_maps(data, Wr, H0, variant=v)
            out.append(f"update_feature_maps! :{v} {time.perf_counter() - t0:.2f} s")
        print(f"fp64 numpy restatement of the same calls ({os.environ.get('OMP_NUM_THREADS', 'all')} BLAS threads): " + ", ".join(out), flush=True)


if __name__ == "__main__":
    main()
