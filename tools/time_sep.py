#!/usr/bin/env python3
"""The separable fit (src/algs/separable.jl) at the figure shape (N=250, T=50000, K=5, L=20) on one GPU, stage by stage: each
stage timed on the host clock (every entry synchronises before it returns) -- two warm-up calls, then REPS timed ones on the
same inputs; the median, the smallest and the largest are printed.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel table (profiles/sep_fig_shape.txt has both).

    python3 tools/time_sep.py [--restatement] [--reps N] [--only-spa]
    python3 tools/time_sep.py --kernel-table <rocprofv3 dir>/<name>_kernel_stats.csv

--restatement also times the fp64 numpy restatement (tests/sep_restatement.py, rewritten mode) of the same stages on the CPU
(OMP_NUM_THREADS sets its BLAS threads).  --kernel-table also prints what share of the 6.3 TB/s copy rate sep_project_kernel
reaches (one read and one write of N x T doubles per call); for that figure profile a run with --only-spa, which makes nothing
but SPA calls without `pre`, so that every sep_project_kernel call moves the same N x T residual."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

N, T, K, L = 250, 50000, 5, 20
COPY_RATE = 6.3e12  # bytes/s


def kernel_table(path):
    import csv
    import re

    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "sep" not in name and "anls" not in name and "fp64" not in name:
            continue
        m = re.search(r"fp64_gemm_kernel<\w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)", name)
        short = (f"contraction {m.group(1)} x {m.group(2)} -> {m.group(3)}" if m
                 else re.sub(r"\(.*", "", name).replace("void ", "").replace("sep::", "").replace("anls::", "").replace("fp64::", ""))
        rows.append((short, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e6))
    tot = sum(r[2] for r in rows)
    print(f"{'kernel':<62} {'calls':>6} {'total ms':>9} {'avg ms':>8} {'share':>6}")
    for r in sorted(rows, key=lambda r: -r[2]):
        print(f"{r[0]:<62} {r[1]:>6} {r[2]:>9.2f} {r[3]:>8.3f} {100 * r[2] / tot:>5.1f}%")
    print(f"{'total':<62} {'':>6} {tot:>9.2f}")
    for r in rows:
        if r[0].startswith("sep_project_kernel") and not any(q[0].startswith("anls") for q in rows):  # (an --only-spa run)
            rate = 2 * N * T * 8 / (r[3] * 1e-3)
            print(f"sep_project_kernel: {2 * N * T * 8 / 1e6:.0f} MB per call in {r[3]:.3f} ms = {rate / 1e12:.2f} TB/s = {100 * rate / COPY_RATE:.0f} % of {COPY_RATE / 1e12} TB/s "
                  "(in a run with --only-spa; the average includes the first round of each call, which only reads; the residual, "
                  f"{N * T * 8 / 2**20:.0f} MiB, fits in the 256 MiB Infinity Cache)")


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
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    import sep_restatement as S
    import cmf_jl_amd as cmf

    data, tW, tH, _, _, thresh = S.case_data((N, T, K, L, 0.1, None, 1))
    R = K * L
    t0 = time.perf_counter()
    rule = cmf.Separable(data, K, L)
    print(f"figure shape (N={N} T={T} K={K} L={L}, R={R}), fp64; Separable construction (cmf_create + cmf_sep_prepare): "
          f"{1e3 * (time.perf_counter() - t0):.1f} ms; {reps} timed calls after 2 warm-up calls: median [min .. max]")

    def line(name, f, extra=""):
        med, lo, hi = timed(f, reps)
        print(f"{name:<34}: {med:9.2f} ms [{lo:.2f} .. {hi:.2f}]  {extra}", flush=True)

    try:
        vertices = rule.spa(thresh=thresh)
        if "--only-spa" in sys.argv:
            return line("SPA (R rounds, pre=nothing)", lambda: rule.spa(thresh=thresh), f"{2 * R} kernels, one read-back")
        V, G = rule.nnls(vertices)
        P, head = rule.shift_table(G)
        groups = rule.cluster(P, head)
        line("SPA (R rounds, pre=nothing)", lambda: rule.spa(thresh=thresh), f"{2 * R} kernels, one read-back")
        line("SPA pre=:svdcond", lambda: rule.spa(thresh=thresh, pre=":svdcond"), "incl. X X' on the device and eigh on the host")
        line("NNLS + renormalize!", lambda: rule.nnls(vertices), f"pivoting rounds {rule.last_nnls_exchanges} over {T} problems of {R} unknowns")
        line("shift table (P, head)", lambda: rule.shift_table(G), f"2 R^2 L T = {2 * R * R * L * T / 1e9:.1f} GFLOP, incl. the transposes of G and P on the host")
        line("grouping + sorting (host, numpy)", lambda: rule.cluster(P, head))
        line("construct_WH (host side of the ABI)", lambda: rule.construct(V, G, groups))
    finally:
        rule.close()
    line("separable_fit end to end", lambda: cmf.separable_fit(data, K, L, thresh=thresh), "incl. handle construction and upload")
    if "--restatement" in sys.argv:
        out = []

        def one(name, f):
            t0 = time.perf_counter()
            r = f()
            out.append(f"{name} {time.perf_counter() - t0:.2f} s")
            return r

        v = one("SPA", lambda: S.spa(data, R, thresh=thresh))
        Vr, Gr = one("NNLS", lambda: S.nnls_step(data, v))
        tab = one("shift table", lambda: S.shift_table(Gr, L))
        one("grouping + sorting", lambda: [S.sort_group(g, Gr, L, table=tab) for g in S.find_groups(S.similarity(Gr, L, table=tab), K, L)])
        print(f"fp64 numpy restatement (rewritten mode) of the same stages ({os.environ.get('OMP_NUM_THREADS', 'all')} BLAS threads): " + ", ".join(out),
              flush=True)
        assert v == vertices


if __name__ == "__main__":
    main()
