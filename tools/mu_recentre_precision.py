#!/usr/bin/env python3
"""How long an MU fit with seqNMF's re-centring step may run under the 1e-4 bar, and how safe its shift decisions are against rounding
(CPU only; writes profiles/mu_recentre_precision.txt).

tests/recentre_restatement.py's fit_mu_recentred is rerun as its float32 model (float32 factors, contractions and element-wise updates;
the masses summed in fp64 from the float32 W, as on the device) and compared with its fp64 run on the fixtures of
tests/test_gpu_recentre.py (recentre_restatement.FIXTURES):

  distance   the largest of the Frobenius-relative errors of W and of H and the largest relative error of loss_hist up to a count.  A
             count is ADMITTED while the distance is at most a THIRD of the bar at every count up to it (the other two thirds are left
             for what the model does not cover: the order of the sums, the device's division).
  margin     per fixture, over all steps up to the admitted count and all live components: `diff`, the largest difference between the
             two runs' ratios m1 / m0, and `gap`, the smallest distance of the fp64 ratio from an integer.  A fixture is admitted only
             if gap >= 10 diff, so that a rounding difference cannot flip a floor -- a condition on the inputs, met by choice of seed.

    python tools/mu_recentre_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recentre_restatement as rr  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 8, 10, 12, 16, 20)


def frob_rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def measure(name):
    data, W0, H0, _ = rr.fixture_problem(name)
    rows = {}
    for c in COUNTS:
        a = rr.fit_mu_recentred(data, W0, H0, c)
        b = rr.fit_mu_recentred(data, W0, H0, c, dtype=np.float32)
        dist = max(frob_rel(b["W"], a["W"]), frob_rel(b["H"], a["H"]), float(np.max(np.abs(b["loss_hist"] - a["loss_hist"]) / np.abs(a["loss_hist"]))))
        live = np.isfinite(a["ratios"]) & np.isfinite(b["ratios"])
        same = np.array_equal(a["shifts"], b["shifts"])
        diff = float(np.max(np.abs(a["ratios"] - b["ratios"])[live])) if same else float("inf")
        gap = float(np.min(np.abs(a["ratios"] - np.round(a["ratios"]))[live]))
        rows[c] = (dist, diff, gap, int(a["moved"].sum()))
    return rows


def main():
    lines = ["# distance of the re-centred MU restatement's float32 model from its fp64 run (max of relW, relH, max rel loss_hist), and the margin of",
             "# its shift decisions: diff = largest |ratio32 - ratio64| of m1 / m0, gap = smallest distance of the fp64 ratio from an integer",
             "# fixture | count | distance | diff | gap | sum of |s_k| so far"]
    admit = []
    for name in rr.FIXTURES:
        rows, ok = measure(name), 0
        for i, c in enumerate(COUNTS):
            dist, diff, gap, moved = rows[c]
            lines.append(f"{name} | {c} | {dist:.2e} | {diff:.2e} | {gap:.2e} | {moved}")
            if dist <= BAR / 3 and gap >= 10 * diff and ok == (COUNTS[i - 1] if i else 0):
                ok = c
        admit.append((name, ok, rows[ok][1] if ok else float("nan"), rows[ok][2] if ok else float("nan")))
    lines.append(f"# admitted: the largest count up to which every distance is at most a third of the bar ({BAR / 3:.2e}) and gap >= 10 diff")
    lines += [f"admit {name} {ok} diff {diff:.3e} gap {gap:.3e}" for name, ok, diff, gap in admit]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_recentre_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
