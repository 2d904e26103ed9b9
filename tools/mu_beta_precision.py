#!/usr/bin/env python3
"""How long a beta-divergence MU fit may run under the 1e-4 bar, and how close to 0 and 1 beta may come (CPU only; writes
profiles/mu_beta_precision.txt).

The device contracts in fp32 and forms Q = exp2((beta - 1) log2 e), P = data exp2((beta - 2) log2 e) and the loss terms
y^beta phi(x / y) in fp32.  tests/beta_mu_restatement.py is rerun with float32 contractions AND a float32 epilogue (cdtype = edtype =
float32) and compared with its fp64 run, on the inputs of the fixtures tests/test_gpu_beta_mu.py fits
(tests/golden/make_golden_beta_mu.py: CASES): the distance is the largest of the Frobenius-relative errors of W and of H and the
largest relative error of loss_hist up to that iteration.  A (case, count) pair is ADMITTED to the GPU test when that distance is at
most a THIRD of the bar at every count up to it: the other two thirds are left for what this model does not cover (the device's
v_log_f32 / v_exp_f32 and division, the order of the sums).  The `admit` lines are what tests/test_gpu_beta_mu.py and the fixture
generator read.

The `window` line: the loss carries the factor 1 / (beta (beta - 1)), so its float32 error grows towards beta = 0 and beta = 1.  The
half-width of the refused window around each is the smallest step of LADDER at whose edges (beta = w, 1 - w, 1 + w) the distance
after WINDOW_COUNT iterations stays within a third of the bar on every fixture shape.  include/cmf_hip.h (CMF_BETA_WINDOW), host.py
and the restatement hold the same number; tests/test_beta_mu_cpu.py checks that they agree with this file's line.

    python tools/mu_beta_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import beta_mu_restatement as br  # noqa: E402
import make_golden_beta_mu as mg  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20, 50, 100)
LADDER = (0.01, 0.02, 0.05, 0.1)
WINDOW_COUNT = 20
TABLE_BETAS = (0.02, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.98, 1.02, 1.05, 1.1, 1.5, 2, 3, 4)
TABLE_SHAPES = ("small", "short")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(data, W0, H0, beta, reg, dtype, counts):
    W, H = W0.copy(), H0.copy()
    out, losses = {}, [br.beta_loss(data, W, H, beta, dtype, dtype)]
    for it in range(1, max(counts) + 1):
        br.update_motifs(data, W, H, beta, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), cdtype=dtype, edtype=dtype)
        losses.append(br.update_feature_maps(data, W, H, beta, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), cdtype=dtype, edtype=dtype))
        if it in counts:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def distances(shape_name, beta, counts):
    """{count: (factor distance, loss distance)} and the fp64 loss at the last count."""
    data, W0, H0, reg = mg.inputs(shape_name)
    data, W0, H0 = f64(data), f64(W0), f64(H0)
    a = trajectory(data, W0, H0, beta, reg, np.float64, counts)
    b = trajectory(data, W0, H0, beta, reg, np.float32, counts)
    out = {c: (max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1])), float(np.max(np.abs(b[c][2] - a[c][2]) / np.abs(a[c][2]))))
           for c in counts}
    return out, a[max(counts)][2][-1]


def main():
    lines = ["# distance of the beta-divergence restatement with float32 contractions and a float32 epilogue (Q, P, the loss terms) from",
             "# its fp64 run (max of relW, relH, max rel loss_hist)",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS) + " | loss at it=100"]
    admit = []
    for name, s, beta in mg.CASES:
        dist, last = distances(s, beta, COUNTS)
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

    lines.append(f"# the window: distance after {WINDOW_COUNT} iterations at the edges of each step of the ladder, the worst over the fixture shapes")
    lines.append("# step | beta = step | beta = 1 - step | beta = 1 + step")
    window = None
    for w in LADDER:
        worst = []
        for beta in (w, 1.0 - w, 1.0 + w):
            worst.append(max(max(distances(s, beta, (WINDOW_COUNT,))[0][WINDOW_COUNT]) for s, *_ in mg.SHAPES))
        lines.append(f"# {w:g} | " + " | ".join(f"{d:.2e}" for d in worst))
        if window is None and max(worst) <= BAR / 3:
            window = w
    assert window is not None, "no step of the ladder keeps the loss within a third of the bar"
    lines.append(f"# the smallest step whose edges stay within {BAR / 3:.2e}: beta < window and |beta - 1| < window are refused")
    lines.append(f"window {window:g}")

    lines.append(f"# beta | shape | factors after {WINDOW_COUNT} | loss_hist after {WINDOW_COUNT} | factors after 100 | loss_hist after 100")
    for beta in TABLE_BETAS:
        for s in TABLE_SHAPES:
            dist, _ = distances(s, float(beta), (WINDOW_COUNT, 100))
            lines.append(f"# {beta:g} | {s} | {dist[WINDOW_COUNT][0]:.2e} | {dist[WINDOW_COUNT][1]:.2e} | {dist[100][0]:.2e} | {dist[100][1]:.2e}")
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_beta_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
