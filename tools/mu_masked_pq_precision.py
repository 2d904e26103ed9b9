#!/usr/bin/env python3
"""How long an Itakura-Saito or beta MU fit under a 0/1 mask may run under the 1e-4 bar (CPU only; writes
profiles/mu_masked_pq_precision.txt), by the rule of profiles/mu_beta_precision.txt.

tests/masked_pq_mu_restatement.py is rerun with float32 contractions AND a float32 epilogue (cdtype = edtype = float32) and compared
with its fp64 run on the cases tests/golden/make_golden_masked_pq_mu.py writes fixtures for (CASES there) and on those the GPU test
compares with the restatement directly (LIVE there): the distance is the largest
of the Frobenius-relative errors of W and of H and the largest relative error of loss_hist up to that iteration.  A (case, count)
pair is ADMITTED when that distance is at most a THIRD of the bar at every count up to it: the other two thirds are left for what
this model does not cover (the device's v_log_f32 / v_exp_f32 and division, the order of the sums).  The `admit` lines are what the
fixture generator and tests/test_masked_pq_mu_cpu.py read.

    python tools/mu_masked_pq_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_masked_pq_mu as mg  # noqa: E402
import masked_pq_mu_restatement as pm  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20)


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(case, dtype, counts):
    shape, kind, with_reg, beta, _ = case
    data, _, mask, W0, H0 = pm.synthetic_case(shape, kind)
    reg = dict(pm.REG) if with_reg else dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
    xs, count = pm.check_data(data, mask, beta)
    W, H = W0.copy(), H0.copy()
    out, losses = {}, [pm.masked_loss(xs, mask, count, W, H, beta, dtype, dtype)]
    for it in range(1, max(counts) + 1):
        pm.update_motifs(xs, mask, W, H, beta, l1W=reg["l1W"], l2W=reg["l2W"], cdtype=dtype, edtype=dtype)
        losses.append(pm.update_feature_maps(xs, mask, count, W, H, beta, l1H=reg["l1H"], l2H=reg["l2H"], cdtype=dtype, edtype=dtype))
        if it in counts:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def distances(case, counts):
    a = trajectory(case, np.float64, counts)
    b = trajectory(case, np.float32, counts)
    return {c: max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1]), float(np.max(np.abs(b[c][2] - a[c][2]) / np.abs(a[c][2]))))
            for c in counts}, a[max(counts)][2][-1]


def main():
    lines = ["# distance of the masked Itakura-Saito / beta restatement with float32 contractions and a float32 epilogue (Q, P, the loss",
             "# terms) from its fp64 run (max of relW, relH, max rel loss_hist); b000 is Itakura-Saito",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS) + f" | loss at it={max(COUNTS)}"]
    admit = []
    for case in mg.CASES + mg.LIVE:
        counts = tuple(c for c in COUNTS if c <= max(case[4], 1))  # (no further than the fixture asks for)
        dist, last = distances(case, counts)
        name = pm.case_name(*case[:4])
        row, ok = [], 0
        for i, c in enumerate(COUNTS):
            if c not in dist:
                row.append("-")
                continue
            row.append(f"{dist[c]:.2e}")
            if dist[c] <= BAR / 3 and ok == (COUNTS[i - 1] if i else 0):
                ok = c
        lines.append(f"{name} | " + " | ".join(row) + f" | {last:.3e}")
        admit.append((name, ok))
        print(lines[-1], flush=True)
    lines.append(f"# admitted: the largest count up to which every distance is at most a third of the bar ({BAR / 3:.2e})")
    lines += [f"admit {name} {ok}" for name, ok in admit]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_masked_pq_precision.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
