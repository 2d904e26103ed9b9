#!/usr/bin/env python3
"""The bar of the real-valued cases of tests/test_gpu_significance.py, measured on the CPU (writes profiles/significance_precision.txt).

The device contracts in fp32 (the data and the motifs rounded to fp32, the overlap accumulated in fp32), widens the overlap to fp64 and
forms the raw power sums S1, S2, S3 in fp64; the skewness is host arithmetic on those sums.  tests/significance_restatement.py is run
that way (contraction = float32, raw sums) and compared with its fp64 run scored the textbook way (two-pass centred moments), on the
real-valued inputs of the tests: the planted-sequence problem and the gen_synthetic split with W from a 30-iteration fit.

    row <input> draw-components=<count> err=<largest |skew32 - skew64|> closest_null=<smallest |skewnull - skew|>
    bar skew <value>      8 x the largest err, rounded UP to one significant digit (the convention of profiles/mu_divergence_elementwise.txt)

The condition -- not a measurement -- is closest_null >= 4 x bar on every row: an error within the bar then cannot flip a comparison
skewnull > skew, so the p-values of the device equal the restatement's exactly.  The tool fails when a row misses it.

    make -C oracle && python tools/significance_precision.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import significance_restatement as sr  # noqa: E402
from oracle import cmf_oracle  # noqa: E402

MARGIN, CONDITION = 8, 4


def round_up_1(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def row(name, W, X, seed, nnull):
    K, N, L = W.shape
    T = X.shape[1]
    draws = range(1 + nnull)
    s32 = sr.null_moments(W, X, seed, draws, contraction=np.float32)
    sk32, _ = sr.skew_from_sums(s32, T)
    sk64 = np.zeros_like(sk32)
    for j, d in enumerate(draws):
        sk64[:, j] = sr.skew_two_pass(sr.transconv(sr.null_motif(W, sr.null_shifts(seed, [d], K, N, L)[:, :, 0]), X))
    err = float(np.nanmax(np.abs(sk32 - sk64)))
    gap = float(np.nanmin(np.abs(sk64[:, 1:] - sk64[:, :1])))
    return name, sk32.size, err, gap


if __name__ == "__main__":
    rows = []
    W, X = sr.planted_problem()
    rows.append(row("planted_%dx%dx%dx%d" % sr.PLANTED_SHAPE, W, X, sr.PLANTED_SEED, sr.PLANTED_NNULL))
    W, X = sr.split_problem(cmf_oracle)
    rows.append(row("split_%dx%dx%dx%d" % sr.SPLIT_SHAPE, W, X, sr.SPLIT_SEED, sr.default_nnull(W.shape[0], 0.05)))
    bar = round_up_1(MARGIN * max(r[2] for r in rows))
    lines = ["# tools/significance_precision.py: float32 contraction + fp64 raw power sums against the fp64 two-pass skewness (CPU).",
             "# bar = %d x the largest err, rounded up to one significant digit; condition: closest_null >= %d x bar on every row." % (MARGIN, CONDITION)]
    for name, count, err, gap in rows:
        lines.append("row %s draw-components=%d err=%.3g closest_null=%.3g" % (name, count, err, gap))
    lines.append("bar skew %g" % bar)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    bad = [r for r in rows if r[3] < CONDITION * bar]
    if bad:
        sys.exit("closest_null < %d x bar on %s" % (CONDITION, [r[0] for r in bad]))
    with open(os.path.join(ROOT, "profiles", "significance_precision.txt"), "w") as f:
        f.write(text)
