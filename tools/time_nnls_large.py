#!/usr/bin/env python3
"""The NNLS solver for 129 .. 1024 unknowns (cmf_set_option "nnls_large", csrc/cmf_nnls_large.h) on one GPU: update_motifs! of the
ANLS rule or the NNLS step of the separable fit at a given shape, each call timed on the host clock (the calls synchronise) --
two warm-up calls, then REPS timed ones on the same inputs; the median, the smallest and the largest are printed with the
pivoting rounds of the call.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel table
(profiles/nnls_large.txt has both).

    python3 tools/time_nnls_large.py --w N,T,K,L [--option 0|1] [--reps N] [--restatement]
    python3 tools/time_nnls_large.py --sep N,T,K,L [--reps N] [--restatement]
    python3 tools/time_nnls_large.py --kernel-table <rocprofv3 dir>/<name>_kernel_stats.csv

--w: data and factors of anls_restatement.problem(N, T, K, L, seed=100); --option 0 leaves the option off (K*L <= 128 only).
--sep: the input of sep_restatement.case_data((N, T, K, L, 0.1, None, 1)); SPA picks the K*L vertices, cmf_sep_nnls is timed.
--restatement also times the fp64 numpy restatement of the same call on the CPU (OMP_NUM_THREADS sets its BLAS threads)."""
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
        m = re.search(r"fp64_gemm_kernel<\w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)", name)
        short = (f"contraction {m.group(1)} x {m.group(2)} -> {m.group(3)}" if m
                 else re.sub(r"\(.*", "", name).replace("void ", "").replace("anls::", "").replace("fp64::", "").replace("sep::", ""))
        rows.append((short, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e6))
    tot = sum(r[2] for r in rows)
    print(f"{'kernel':<62} {'calls':>6} {'total ms':>9} {'avg ms':>9} {'share':>6}")
    for r in sorted(rows, key=lambda r: -r[2]):
        print(f"{r[0]:<62} {r[1]:>6} {r[2]:>9.2f} {r[3]:>9.3f} {100 * r[2] / tot:>5.1f}%")
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


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    if "--kernel-table" in sys.argv:
        return kernel_table(arg("--kernel-table"))
    reps = int(arg("--reps", 7))
    threads = os.environ.get("OMP_NUM_THREADS", "all")
    import anls_restatement as R
    import cmf_jl_amd as cmf

    if "--w" in sys.argv:
        N, T, K, L = (int(v) for v in arg("--w").split(","))
        on = int(arg("--option", 1))
        data, W0, H0 = R.problem(N, T, K, L, seed=100)
        rule = cmf.ANLSUpdate(data, W0, H0)
        try:
            rule.set_option("nnls_large", on)
            W = W0.copy(order="F")
            med, lo, hi = timed(lambda: rule.update_motifs(data, W, H0), reps)
            print(f"update_motifs! N={N} T={T} K={K} L={L} nnls_large={on}: {med:9.2f} ms [{lo:.2f} .. {hi:.2f}] ({reps} calls after 2 warm-up)  pivoting rounds "
                  f"{rule.last_W_exchanges} over {N} problems of {K * L} unknowns ({rule.last_W_exchanges / N:.2f} per problem)", flush=True)
        finally:
            rule.close()
        if "--restatement" in sys.argv:
            t0 = time.perf_counter()
            sg = {}
            Wr = R.update_motifs(data, H0, L, stats=sg)
            print(f"fp64 numpy restatement of the same call ({threads} BLAS threads): {time.perf_counter() - t0:.2f} s, pivoting rounds {sg['exchanges']}; "
                  f"GPU vs restatement rel {R.rel(W, Wr):.2e}", flush=True)
    if "--sep" in sys.argv:
        import sep_restatement as S

        N, T, K, L = (int(v) for v in arg("--sep").split(","))
        data, _, _, K, L, thresh = S.case_data((N, T, K, L, 0.1, None, 1))
        rule = cmf.Separable(data, K, L)
        try:
            rule.set_option("nnls_large", 1)
            vertices = rule.spa(thresh=thresh)
            out = []
            med, lo, hi = timed(lambda: out.append(rule.nnls(vertices)), reps)
            print(f"cmf_sep_nnls N={N} T={T} R={K * L}: {med:9.2f} ms [{lo:.2f} .. {hi:.2f}] ({reps} calls after 2 warm-up)  pivoting rounds "
                  f"{rule.last_nnls_exchanges} over {T} problems ({rule.last_nnls_exchanges / T:.2f} per problem)", flush=True)
        finally:
            rule.close()
        if "--restatement" in sys.argv:
            t0 = time.perf_counter()
            st = {}
            _, Gr = S.nnls_step(data, vertices, stats=st)[:2]
            print(f"fp64 numpy restatement of the same step ({threads} BLAS threads): {time.perf_counter() - t0:.2f} s; GPU vs restatement G rel "
                  f"{R.rel(out[-1][1], Gr):.2e}", flush=True)


if __name__ == "__main__":
    main()
