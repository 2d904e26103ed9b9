#!/usr/bin/env python3
"""Per test shape of the ANLS rule (tests/anls_restatement.py: CASES and the figure shape): the floor -- what the restatement's
literal and Gram modes differ by on the same call -- and, when a GPU is present, the GPU-vs-restatement difference of the same
call, the bar the tests hold it to (1000 x floor, at most 1e-8), the zero-pattern mismatches off the near-degenerate entries, the
near-degenerate count and the pivoting rounds on both sides.  Writes the table to stdout (profiles/anls_precision.txt).

    python3 tools/anls_precision.py [--no-fig] [--cpu]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import anls_restatement as R  # noqa: E402


def main():
    cmf = None
    if "--cpu" not in sys.argv:
        import cmf_jl_amd as cmf

        if cmf.load_library().cmf_device_count() < 1:
            cmf = None
    shapes = [(name, *R.CASES[name], i) for i, name in enumerate(sorted(R.CASES))]
    if "--no-fig" not in sys.argv:
        shapes.append(("fig", *R.FIG, "wh", ("basic", "block"), 100))
    print(f"{'shape':8s} {'N':>4} {'T':>6} {'K':>3} {'L':>3} {'call':8s} {'floor':>9} {'bar':>9} {'GPU-vs-R':>9} {'mism':>5} {'near':>5} {'entries':>8} "
          f"{'rounds R':>9} {'rounds GPU':>10} {'|loss diff|':>11}")
    for name, N, T, K, L, steps, variants, seed in shapes:
        data, W0, H0 = R.problem(N, T, K, L, seed)
        rule = cmf.ANLSUpdate(data, W0, H0) if cmf else None
        try:
            W = W0
            calls = ([("W", None)] if "w" in steps else []) + [("H " + v, v) for v in variants]
            for label, v in calls:
                sl, sg = {}, {}
                if v is None:
                    Xl, Xg = R.update_motifs(data, H0, L, mode="literal", stats=sl), R.update_motifs(data, H0, L, stats=sg)
                    W = np.asfortranarray(Xg)
                else:
                    (Xl, _), (Xg, lg) = (R.update_feature_maps(data, W, H0, variant=v, mode="literal", stats=sl),
                                         R.update_feature_maps(data, W, H0, variant=v, stats=sg))
                floor = R.rel(Xl, Xg)
                gpu = mism = rounds = dl = float("nan")
                if rule is not None:
                    if v is None:
                        X = W0.copy(order="F")
                        rule.update_motifs(data, X, H0)
                        rounds = rule.last_W_exchanges
                    else:
                        X = H0.copy(order="F")
                        dl = abs(rule.update_feature_maps(data, W, X, variant=v) - lg)
                        rounds = rule.last_H_exchanges
                    gpu, mism = R.rel(X, Xg), int((((X > 0) != (Xg > 0)) & ~sg["near"]).sum())
                print(f"{name:8s} {N:>4} {T:>6} {K:>3} {L:>3} {label:8s} {floor:>9.2e} {R.bar(floor, 1e-8):>9.2e} {gpu:>9.2e} {mism:>5} "
                      f"{int(sg['near'].sum()):>5} {Xg.size:>8} {sg['exchanges']:>9} {rounds:>10} {dl:>11.1e}", flush=True)
        finally:
            if rule is not None:
                rule.close()


if __name__ == "__main__":
    main()
