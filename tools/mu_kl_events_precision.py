#!/usr/bin/env python3
"""How long a KL-MU fit on an event list may run under the 1e-4 bar (CPU only; writes profiles/mu_kl_events_precision.txt).

The device gathers in fp32.  tests/events_kl_restatement.py is rerun with its gathered sums (est at the events, numW, numH) in float32
and compared with its fp64 run, on the event lists of the fixtures tests/test_gpu_events_kl.py fits (tests/golden/mu_kl_*.npz) and on
the sparse problems it generates: the distance is the largest of the Frobenius-relative errors of W and of H and the largest relative
error of loss_hist up to that iteration.  A (case, count) pair is ADMITTED to the GPU test when that distance is at most a THIRD of the
bar at every count up to it: the other two thirds are left for what this model does not cover (the fp32 division, logf, the order of
the sums).  The `admit` lines at the end are what tests/test_gpu_events_kl.py reads.

    python tools/mu_kl_events_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import events_kl_restatement as er  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20, 50, 100)
FIXTURES = ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_k33", "mu_kl_k32", "mu_kl_short", "mu_kl_l40"]
SPARSE = er.PROBLEMS + [er.MEMORY_PROBLEM]  # (name, generator, arguments, the largest count looked at, regularisers)


def cases():
    for name in FIXTURES:
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
        yield name, er.from_dense(f64(g["data"])), f64(g["W0"]), f64(g["H0"]), {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")}, max(COUNTS)
    for name, gen, kw, top, reg in SPARSE:
        ev, W0, H0 = gen(**kw)
        yield name, ev, W0, H0, reg, top


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(ev, W0, H0, reg, cdtype, top):
    W, H = W0.copy(), H0.copy()
    out, losses = {}, [er.kl_loss(ev, W, H, cdtype)]
    for it in range(1, top + 1):
        er.update_motifs(ev, W, H, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), cdtype=cdtype)
        losses.append(er.update_feature_maps(ev, W, H, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), cdtype=cdtype))
        if it in COUNTS:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def main():
    lines = ["# distance of the event-form KL restatement with float32 gathered sums from its fp64 run (max of relW, relH, max rel loss_hist)",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS) + "   (-: not looked at)"]
    admit = []
    for name, ev, W0, H0, reg, top in cases():
        a = trajectory(ev, W0, H0, reg, np.float64, top)
        b = trajectory(ev, W0, H0, reg, np.float32, top)
        row, ok = [], 0
        for c in COUNTS:
            if c > top:
                row.append("-")
                continue
            d = max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1]), float(np.max(np.abs(b[c][2] - a[c][2]) / a[c][2])))
            row.append(f"{d:.2e}")
            if d <= BAR / 3 and ok == (COUNTS[COUNTS.index(c) - 1] if COUNTS.index(c) else 0):
                ok = c
        lines.append(f"{name} | " + " | ".join(row))
        admit.append((name, ok))
    lines.append(f"# admitted: the largest count up to which every distance is at most a third of the bar ({BAR / 3:.2e})")
    lines += [f"admit {name} {ok}" for name, ok in admit]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_kl_events_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
