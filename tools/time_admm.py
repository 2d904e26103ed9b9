#!/usr/bin/env python3
"""The ADMM rule (src/algs/admm.jl) at config 2's size (N=2000, T=50000, K=32, L=20) on one GPU: one update_motifs! and one
update_feature_maps! from init_rand's start, each timed on the host clock (the calls synchronise), with the inner iteration
counts and reverts and the achieved fp64 rate of the contractions (3 per inner iteration on each side, 2*K*N*L*T flop each).
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel table (profiles/admm_config2.txt has both).

    python3 tools/time_admm.py [--restatement]
    python3 tools/time_admm.py --kernel-table <rocprofv3 dir>/<name>_kernel_stats.csv

--kernel-table prints the per-kernel table of such a run's CSV (`--output-format csv`): the ADMM kernels, a contraction named by
its operand loaders and epilogue, with calls, total and mean time, share, and the contractions' share of the whole.

--restatement also times the fp64 numpy restatement (tests/admm_restatement.py) of the same two calls on the same inputs, on the CPU
(OMP_NUM_THREADS sets its BLAS threads; most of its element-wise work is single-threaded numpy)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

N, T, K, L = 2000, 50000, 32, 20


def kernel_table(path):
    import csv
    import re

    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "admm" not in name and "fp64" not in name:
            continue
        m = re.search(r"fp64_gemm_kernel<\w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)(?:<[^>]*>)?, \w+::(\w+)", name)
        short = (f"contraction {m.group(1)} x {m.group(2)} -> {m.group(3)}" + (" (circ)" if "LagH<true>" in name else "") if m
                 else re.sub(r"\(.*", "", name).replace("void ", "").replace("admm::", "").replace("fp64::", ""))
        rows.append((short, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e6))
    tot = sum(r[2] for r in rows)
    con = sum(r[2] for r in rows if r[0].startswith("contraction"))
    print(f"{'kernel':<62} {'calls':>6} {'total ms':>9} {'avg ms':>8} {'share':>6}")
    for r in sorted(rows, key=lambda r: -r[2]):
        print(f"{r[0]:<62} {r[1]:>6} {r[2]:>9.2f} {r[3]:>8.3f} {100 * r[2] / tot:>5.1f}%")
    print(f"{'total':<62} {'':>6} {tot:>9.2f}")
    print(f"contractions {con:.1f} ms ({100 * con / tot:.0f} %), everything else {tot - con:.1f} ms ({100 * (tot - con) / tot:.0f} %)")


def main():
    if "--kernel-table" in sys.argv:
        return kernel_table(sys.argv[sys.argv.index("--kernel-table") + 1])
    import cmf_jl_amd as cmf

    data = cmf.gen_synthetic(N=N, T=T, seed=1234)
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
    W, H = np.array(W0, order="F"), np.array(H0, order="F")
    flop = 2.0 * K * N * L * T
    t0 = time.perf_counter()
    rule = cmf.ADMMUpdate(data, W, H)
    t_prep = time.perf_counter() - t0
    print(f"config 2 (N={N} T={T} K={K} L={L}), fp64; ADMMUpdate construction (cmf_create + cmf_admm_prepare): {1e3 * t_prep:.1f} ms")
    try:
        t0 = time.perf_counter()
        rule.update_motifs(data, W, H)
        tw = time.perf_counter() - t0
        print(f"update_motifs!      : {1e3 * tw:9.1f} ms  inner iterations {rule.last_W_iters:2d}  reverts {rule.last_W_reverts}  "
              f"contractions {3 * rule.last_W_iters} x {flop:.3g} flop (+ the Gram, {2.0 * (L * K) ** 2 * T:.3g}) -> "
              f"{(3 * rule.last_W_iters * flop + 2.0 * (L * K) ** 2 * T) / tw / 1e12:.2f} TFLOP/s over the whole call", flush=True)
        t0 = time.perf_counter()
        loss = rule.update_feature_maps(data, W, H)
        th = time.perf_counter() - t0
        print(f"update_feature_maps!: {1e3 * th:9.1f} ms  inner iterations {rule.last_H_iters:2d}  reverts {rule.last_H_reverts}  "
              f"contractions {3 * rule.last_H_iters + 1} x {flop:.3g} flop -> {(3 * rule.last_H_iters + 1) * flop / th / 1e12:.2f} TFLOP/s "
              f"over the whole call; loss {loss:.6f}", flush=True)
    finally:
        rule.close()
    if "--restatement" in sys.argv:
        import admm_restatement as R

        d = np.asarray(data)
        t0 = time.perf_counter()
        Wr, _, wi, wr = R.update_motifs(d, np.asarray(H0), L)
        tw = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, hi, hr = R.update_feature_maps(d, Wr)
        th = time.perf_counter() - t0
        print(f"fp64 numpy restatement of the same calls ({os.environ.get('OMP_NUM_THREADS', 'all')} BLAS threads): update_motifs! "
              f"{tw:.1f} s ({wi} inner iterations, {wr} reverts), update_feature_maps! {th:.1f} s ({hi} inner iterations, {hr} reverts)",
              flush=True)


if __name__ == "__main__":
    main()
