#!/usr/bin/env python3
"""How long a masked KL-MU fit may run under the 1e-4 bar (CPU only; writes profiles/mu_masked_kl_precision.txt).

tools/mu_kl_precision.py for the rule under a mask: tests/masked_kl_mu_restatement.py is rerun with its contractions in float32 and
compared with its fp64 run -- the largest of the Frobenius-relative errors of W and of H and the largest relative error of loss_hist
up to that iteration -- on the fixtures tests/test_gpu_masked_kl_mu.py fits (tests/golden/mu_masked_kl_*.npz, once they exist) and
on every shape of masked_kl_mu_restatement.SHAPES under its three masks, without and with the regularisers, data NaN under
mask == 0.  A (case, count) pair is ADMITTED when that distance is at most a THIRD of the bar at every count up to it.  The
unregularised T < L cases drive the loss to round-off level within a few iterations, where its relative error means nothing:
they are admitted for correspondingly few.  The `admit` lines at the end are what the tests read.

    python tools/mu_masked_kl_precision.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import masked_kl_mu_restatement as mk  # noqa: E402

BAR = 1e-4
COUNTS = (1, 2, 5, 10, 20, 50, 100)
FIXTURE_INPUTS = {"mu_masked_kl_small": ("mu_kl_small", "blocks", False), "mu_masked_kl_small_reg": ("mu_kl_small_reg", "blocks", True),
                  "mu_masked_kl_k5": ("mu_kl_k5", "speckle", False), "mu_masked_kl_k33": ("mu_kl_k33", "dead", False),
                  "mu_masked_kl_k32": ("mu_kl_k32", "blocks", False), "mu_masked_kl_short": ("mu_kl_short", "blocks", False),
                  "mu_masked_kl_l40": ("mu_kl_l40", "blocks", False)}  # fixture: (inputs, mask, all four regularisers)


def fixture_case(name):
    """(data with NaN under the mask, mask, W0, H0, reg) of a fixture: the inputs of the mu_kl_* file under the fixture's mask."""
    src, kind, reg = FIXTURE_INPUTS[name]
    g = np.load(os.path.join(ROOT, "tests", "golden", src + ".npz"))
    data, W0, H0 = (np.asarray(g[k], dtype=np.float64) for k in ("data", "W0", "H0"))
    K, N, L = W0.shape
    mask = mk.make_mask(kind, N, data.shape[1], L)
    return np.where(mask != 0, data, np.nan), mask, W0, H0, dict(mk.REG) if reg else {}


def cases():
    for name in FIXTURE_INPUTS:
        yield (name,) + fixture_case(name)
    for shape in mk.SHAPES:
        for kind in mk.MASKS:
            data, _, mask, W0, H0 = mk.synthetic_case(shape, kind)
            for reg in ({}, dict(mk.REG)):
                yield mk.case_name(shape, kind, reg), data, mask, W0, H0, reg


def frob_rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trajectory(data, mask, W0, H0, reg, cdtype):
    rule = mk.MaskedKL(data, mask)
    W, H = W0.copy(), H0.copy()
    out, losses = {}, [mk.masked_kl_loss(rule, W, H, cdtype)]
    for it in range(1, max(COUNTS) + 1):
        mk.update_motifs(rule, W, H, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), cdtype=cdtype)
        losses.append(mk.update_feature_maps(rule, W, H, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), cdtype=cdtype))
        if it in COUNTS:
            out[it] = (W.copy(), H.copy(), np.asarray(losses))
    return out


def main():
    lines = ["# distance of the masked KL restatement with float32 contractions from its fp64 run (max of relW, relH, max rel loss_hist)",
             "# case | " + " | ".join(f"it={c}" for c in COUNTS)]
    admit = []
    for name, data, mask, W0, H0, reg in cases():
        a = trajectory(data, mask, W0, H0, reg, np.float64)
        b = trajectory(data, mask, W0, H0, reg, np.float32)
        row, ok = [], 0
        for c in COUNTS:
            with np.errstate(divide="ignore", invalid="ignore"):
                dl = float(np.max(np.abs(b[c][2] - a[c][2]) / a[c][2]))
            d = max(frob_rel(b[c][0], a[c][0]), frob_rel(b[c][1], a[c][1]), dl)
            row.append(f"{d:.2e}")
            if d <= BAR / 3 and ok == (COUNTS[COUNTS.index(c) - 1] if COUNTS.index(c) else 0):
                ok = c
        lines.append(f"{name} | " + " | ".join(row))
        admit.append((name, ok))
    lines.append(f"# admitted: the largest count up to which every distance is at most a third of the bar ({BAR / 3:.2e})")
    lines += [f"admit {name} {ok}" for name, ok in admit]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "mu_masked_kl_precision.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
