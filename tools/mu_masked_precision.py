#!/usr/bin/env python3
"""How long a masked MU fit may run under the 1e-4 bar (CPU only; writes profiles/mu_masked_precision.txt).

The device contracts in fp32.  tests/masked_mu_restatement.py is rerun with its contractions in float32 and compared with its
fp64 run, on the shapes and masks tests/test_gpu_masked_mu.py fits: the distance is the largest of the Frobenius-relative errors
of W and of H and the largest relative error of loss_hist up to that iteration.  The GPU test may fit for the largest count
(100 if it holds) at which that distance stays below a QUARTER of the bar on every case: tests/test_gpu_masked_mu.py's FIT_ITERS.

    python tools/mu_masked_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import masked_mu_restatement as mr  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20, 30, 50, 75, 100)
SHAPES = [(48, 300, 4, 8), (130, 700, 32, 20), (37, 150, 33, 7), (20, 200, 6, 40), (6, 3, 2, 5), (250, 2000, 5, 20)]
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)


def cases():
    for (N, T, K, L) in SHAPES:
        rng = np.random.default_rng(3)
        W0, H0, data = rng.random((K, N, L)), rng.random((K, T)), rng.random((N, T))
        for mname, mask in (("20% blocks of L", mr.block_mask(N, T, 0.2, L, 11)), ("50% speckle", mr.block_mask(N, T, 0.5, 1, 12))):
            if not mask.any():
                continue
            for rname, reg in (("", {}), (" +reg", REG)):
                yield f"({N},{T},{K},{L}) {mname}{rname}", data, mask, W0, H0, reg


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(data, mask, W0, H0, reg, cdtype):
    W, H = W0.copy(), H0.copy()
    rule = mr.MaskedMult(data, mask)
    out, losses = {}, [mr.masked_loss(rule, W, H, cdtype)]
    for it in range(1, max(COUNTS) + 1):
        mr.update_motifs(rule, W, H, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), cdtype=cdtype)
        losses.append(mr.update_feature_maps(rule, W, H, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), cdtype=cdtype))
        if it in COUNTS:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def main():
    lines = ["# distance of the restatement with float32 contractions from its fp64 run (max of relW, relH, max rel loss_hist)",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS)]
    worst = {c: 0.0 for c in COUNTS}
    for name, data, mask, W0, H0, reg in cases():
        a = trajectory(data, mask, W0, H0, reg, np.float64)
        b = trajectory(data, mask, W0, H0, reg, np.float32)
        row = []
        for c in COUNTS:
            d = max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1]), float(np.max(np.abs(b[c][2] - a[c][2]) / a[c][2])))
            worst[c] = max(worst[c], d)
            row.append(f"{d:.2e}")
        lines.append(f"{name} | " + " | ".join(row))
    lines.append("worst | " + " | ".join(f"{worst[c]:.2e}" for c in COUNTS))
    ok = [c for c in COUNTS if all(worst[q] < BAR / 4 for q in COUNTS if q <= c)]
    lines.append(f"# largest count with the worst distance below a quarter of the bar ({BAR / 4:.1e}) up to it: {max(ok) if ok else 0}")
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_masked_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
