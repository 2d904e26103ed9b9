#!/usr/bin/env python3
"""How long an MU fit with seqNMF's cross-orthogonality penalties may run under the 1e-4 bar (CPU only; writes
profiles/mu_xortho_precision.txt).

The device contracts in fp32 and forms S, off, the enlarged denominators and the quotients in fp32.  tests/xortho_mu_restatement.py
is rerun with float32 contractions and a float32 epilogue (cdtype = float32) and compared with its fp64 run, on the inputs of the
fixtures tests/test_gpu_xortho_mu.py fits (xortho_mu_restatement.CASES): the distance is the largest of the Frobenius-relative errors
of W and of H and the largest relative error of loss_hist up to that iteration.  A (case, count) pair is ADMITTED to the GPU test when
that distance is at most a THIRD of the bar at every count up to it: the other two thirds are left for what this model does not cover
(the order of the sums, the device's division).  The `admit` lines are what tests/test_xortho_mu_cpu.py, tests/test_gpu_xortho_mu.py
and the fixture writer read.  The model is tools/mu_beta_precision.py's.

    python tools/mu_xortho_precision.py && python tests/xortho_mu_restatement.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xortho_mu_restatement as xr  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20, 50, 100)


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(data, W0, H0, weights, reg, dtype, counts):
    W, H = W0.copy(), H0.copy()
    out, losses = {}, [xr.compute_loss(data, W, H, dtype)]
    for it in range(1, max(counts) + 1):
        xr.update_motifs(data, W, H, *weights, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), cdtype=dtype)
        losses.append(xr.update_feature_maps(data, W, H, *weights, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), cdtype=dtype))
        if it in counts:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def distances(shape_name, weights, counts):
    """{count: (factor distance, loss distance)} and the fp64 loss at the last count."""
    data, W0, H0, reg = xr.inputs(shape_name)
    a = trajectory(data, W0, H0, weights, reg, np.float64, counts)
    b = trajectory(data, W0, H0, weights, reg, np.float32, counts)
    out = {c: (max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1])), float(np.max(np.abs(b[c][2] - a[c][2]) / np.abs(a[c][2]))))
           for c in counts}
    return out, a[max(counts)][2][-1]


def main():
    lines = ["# distance of the cross-orthogonality restatement with float32 contractions and a float32 epilogue from its fp64 run",
             "# (max of relW, relH, max rel loss_hist); weight sets: " + ", ".join(f"{k} = {v}" for k, v in xr.WEIGHT_SETS.items())
             + "; scaled to lambda = " + ", ".join(f"{v} on {k}" for k, v in xr.SHAPE_LAM.items()),
             "# case | " + " | ".join(f"it={c}" for c in COUNTS) + " | loss at it=100"]
    admit = []
    for name, s, wset in xr.CASES:
        dist, last = distances(s, xr.weights_of(s, wset), COUNTS)
        row, ok = [], 0
        for i, c in enumerate(COUNTS):
            d = max(dist[c])
            row.append(f"{d:.2e}")
            if d <= BAR / 3 and ok == (COUNTS[i - 1] if i else 0):
                ok = c
        lines.append(f"{name} | " + " | ".join(row) + f" | {last:.3e}")
        admit.append((name, ok))
    lines.append(f"# admitted: the largest count up to which every distance is at most a third of the bar ({BAR / 3:.2e})")
    lines += [f"admit {name} {ok}" for name, ok in admit]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_xortho_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
