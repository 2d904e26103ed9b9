#!/usr/bin/env python3
"""How long an Itakura-Saito MU fit may run under the 1e-4 bar (CPU only; writes profiles/mu_is_precision.txt).

The device contracts in fp32 and forms Q = 1 / e, P = (data Q) Q and the loss terms (r - 1) - log(r) in fp32.
tests/is_mu_restatement.py is rerun with float32 contractions AND a float32 epilogue (cdtype = edtype = float32) and compared with its
fp64 run, on the inputs of the fixtures tests/test_gpu_is_mu.py fits (tests/golden/make_golden_is_mu.py: CASES) and on the two
mid-size shapes that test fits: the distance is the largest of the Frobenius-relative errors of W and of H and the largest relative
error of loss_hist up to that iteration.  A (case, count) pair is ADMITTED to the GPU test when that distance is at most a THIRD of
the bar at every count up to it: the other two thirds are left for what this model does not cover (the device's division and logf,
the order of the sums).  The `admit` lines at the end are what tests/test_gpu_is_mu.py and the fixture generator read.

    python tools/mu_is_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import is_mu_restatement as ir  # noqa: E402
import make_golden_is_mu as mg  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20, 50, 100)
SYNTHETIC = [(130, 700, 32, 20), (250, 2000, 5, 20)]


def cases():
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    for name, _, _, _, _ in mg.CASES:
        data, W0, H0, reg = mg.inputs(name)
        yield name, f64(data), f64(W0), f64(H0), reg
    for (N, T, K, L) in SYNTHETIC:
        data, W0, H0 = ir.positive_problem(N, T, K, L, seed=3)
        yield f"synthetic({N},{T},{K},{L})", f64(data), f64(W0), f64(H0), {}


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(data, W0, H0, reg, dtype):
    W, H = W0.copy(), H0.copy()
    out, losses = {}, [ir.is_loss(data, W, H, dtype, dtype)]
    for it in range(1, max(COUNTS) + 1):
        ir.update_motifs(data, W, H, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), cdtype=dtype, edtype=dtype)
        losses.append(ir.update_feature_maps(data, W, H, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), cdtype=dtype, edtype=dtype))
        if it in COUNTS:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def main():
    lines = ["# distance of the Itakura-Saito restatement with float32 contractions and a float32 epilogue (Q, P, the loss terms) from its",
             "# fp64 run (max of relW, relH, max rel loss_hist)",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS) + " | loss at it=100"]
    admit = []
    for name, data, W0, H0, reg in cases():
        a = trajectory(data, W0, H0, reg, np.float64)
        b = trajectory(data, W0, H0, reg, np.float32)
        row, ok = [], 0
        for c in COUNTS:
            d = max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1]), float(np.max(np.abs(b[c][2] - a[c][2]) / a[c][2])))
            row.append(f"{d:.2e}")
            if d <= BAR / 3 and ok == (COUNTS[COUNTS.index(c) - 1] if COUNTS.index(c) else 0):
                ok = c
        lines.append(f"{name} | " + " | ".join(row) + f" | {a[100][2][-1]:.3e}")
        admit.append((name, ok))
    lines.append(f"# admitted: the largest count up to which every distance is at most a third of the bar ({BAR / 3:.2e})")
    lines += [f"admit {name} {ok}" for name, ok in admit]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_is_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
