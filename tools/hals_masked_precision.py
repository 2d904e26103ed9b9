#!/usr/bin/env python3
"""How long a masked HALS fit (library option "hals_mask") may be compared under the 1e-4 bar (CPU only; writes
profiles/hals_masked_precision.txt).

The device contracts in fp32 and holds the sweeps' state in fp32.  tests/masked_hals_restatement.py's model of that arithmetic
(f32_iteration: conv, masked residual, G and P contracted in float32, the Gram-projected sweeps of tests/hals_gram_form.py run in
float32) is compared with the same iteration in float64, on the shapes, masks and regularisers tests/test_gpu_masked_hals.py fits:
the distance is the largest of the Frobenius-relative errors of W and of H and the largest relative error of loss_hist up to that
iteration.  A (shape, mask) case is compared on the device only over the iterations where that distance stays within a THIRD of the
bar, the project's admission rule (tests/test_gpu_masked_hals.py: COMPARE_ITERS).

    python tools/hals_masked_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hals_gram_form as gf  # noqa: E402
import masked_hals_restatement as hr  # noqa: E402
from oracle import cmf_oracle as oracle  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10)
SHAPES = [(70, 4130, 32, 5), (37, 150, 3, 4), (20, 200, 33, 3)]
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)


def problem(N, T, K, L):
    """Planted sequences and the least-squares-scaled random start of init_rand: the problems of the HALS parity tests
    (tests/test_gpu_parity.py) and of tests/test_gpu_masked_hals.py (its problem())."""
    data, _, _ = oracle.c_gen_synthetic(N=N, T=T, K=3, L=L, seed=1234)
    data = np.maximum(data, 0.0)
    W0, H0 = oracle.c_init_rand(data, L=L, K=K, seed=0)
    return W0, H0, data


def cases():
    for (N, T, K, L) in SHAPES:
        W0, H0, data = problem(N, T, K, L)
        for mname, mask in hr.masks(N, T, L).items():
            for rname, reg in (("", {}), (" +reg", REG)):
                yield f"({N},{T},{K},{L}) {mname}{rname}", data, mask, W0, H0, reg


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(data, mask, W0, H0, reg, dtype):
    W, H = W0.copy(), H0.copy()
    out, losses = {}, []
    for it in range(1, max(COUNTS) + 1):
        W, H, loss = hr.f32_iteration(oracle, gf, data, mask, W, H, reg.get("l1W", 0), reg.get("l2W", 0), reg.get("l1H", 0), reg.get("l2H", 0), dtype)
        losses.append(loss)
        if it in COUNTS:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def main():
    lines = ["# distance of the restatement with float32 contractions and sweeps from its fp64 run (max of relW, relH, max rel loss_hist)",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS) + " | compared up to"]
    worst = {c: 0.0 for c in COUNTS}
    for name, data, mask, W0, H0, reg in cases():
        a = trajectory(data, mask, W0, H0, reg, np.float64)
        b = trajectory(data, mask, W0, H0, reg, np.float32)
        row, upto = [], 0
        for c in COUNTS:
            d = max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1]), float(np.max(np.abs(b[c][2] - a[c][2]) / a[c][2])))
            worst[c] = max(worst[c], d)
            row.append(f"{d:.2e}")
            if d < BAR / 3 and upto == ([0] + list(COUNTS))[COUNTS.index(c)]:
                upto = c
        lines.append(f"{name} | " + " | ".join(row) + f" | {upto}")
        print(lines[-1], flush=True)
    lines.append("worst | " + " | ".join(f"{worst[c]:.2e}" for c in COUNTS) + " |")
    lines.append(f"# a case is compared on the device up to the largest count with the distance below a third of the bar ({BAR / 3:.1e}) at every count up to it")
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "hals_masked_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
