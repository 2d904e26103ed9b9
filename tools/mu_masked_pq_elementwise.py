#!/usr/bin/env python3
"""The element-wise bar of the masked Itakura-Saito / beta forms on the integer problems (tests/test_gpu_masked_pq_mu.py), measured
on the CPU (writes profiles/mu_masked_pq_elementwise.txt), by the rule of tools/mu_divergence_elementwise.py, whose own file this
tool does not touch.

For every (form, shape, family) of tests/exact_masked_pq.py (FORMS x SHAPES; family "W": one update_motifs!, family "H": one
update_feature_maps! and its loss) the fp64 half is rerun with cdtype = edtype = float32, and a `row` line records err (the largest
element-wise relative error of the updated factor), loss_err and the sensitivity (the smallest relative change of an element when
one positive term of its numerator or denominator sum is removed; `>=`: the closed-form lower bound was enough).

`bar <form> <value>`: 8 x the largest err of the form, rounded UP to one significant digit.  There is no `lossbar` line: the loss is
held to the unmasked twin's line of profiles/mu_divergence_elementwise.txt, which was measured over the whole table (the masked loss
sums a subset of the same float32 terms; loss_err of these few rows is recorded only).  The factor 8 is for what the model leaves out (v_rcp_f32 / v_log_f32 / v_exp_f32 at about 1 ulp each, the order of the
sums, the fp32 step).  The condition -- not a measurement -- is sensitivity >= 4 x bar on every row; the tool fails when a row misses
it, and the GPU test asserts it again from its own arrays.  `gpu` / `gpuloss` lines are what an MI355X run of the test observed; they
are appended by hand from the test's output and kept when the tool rewrites the file.

    python tools/mu_masked_pq_elementwise.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import exact_masked_pq as xq  # noqa: E402
import exact_problems as ep  # noqa: E402
from mu_divergence_elementwise import CONDITION, EXACT_BELOW, MARGIN, round_up_1  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mu_masked_pq_elementwise.txt")


def main():
    rows = []
    for s in xq.SHAPES:
        shape = s[:4]
        for family in ("W", "H"):
            for form in xq.FORMS:
                W, H, X, mask, _ = xq.make_problem(shape, family, form)
                a = xq.masked_half(form, family, X, mask, W, H)
                m = xq.masked_half(form, family, X, mask, W, H, cdtype=np.float32, edtype=np.float32)
                err = float(ep.rel_err(m["new"], a["new"]).max())
                loss_err = abs(m["loss"] - a["loss"]) / a["loss"] if family == "H" else 0.0
                sens, bound = xq.sensitivity(form, a, exact=False), True
                if sens < EXACT_BELOW:
                    sens, bound = xq.sensitivity(form, a), False
                rows.append((form, shape, family, err, loss_err, sens, bound))
    kept = [ln for ln in (open(OUT).read().splitlines() if os.path.exists(OUT) else []) if ln.split()[:1] and ln.split()[0] in ("gpu", "gpuloss")]
    lines = ["# tools/mu_masked_pq_elementwise.py: the masked Itakura-Saito / beta halves (tests/exact_masked_pq.py) with float32 contractions and a",
             "# float32 epilogue against their fp64 runs, one update per (form, shape, family); a quarter of the entries held out in blocks of 1 x 8.",
             "# bar = %d x the largest err of the form, rounded up to one significant digit; condition: sensitivity >= %d x bar on every row." % (MARGIN, CONDITION),
             "# No lossbar of its own: the GPU test holds the loss to the UNMASKED twin's `lossbar` line of profiles/mu_divergence_elementwise.txt",
             "# (is 5e-06, beta050 2e-05, beta150 7e-07), which was taken over the whole integer table; the masked loss is a sub-sum of the very same",
             "# float32 terms, and the few rows here understate the worst of a nearly cancelling sum of roundings (loss_err of the rows: for the record)."]
    bars, failed = {}, []
    for form in xq.FORMS:
        mine = [r for r in rows if r[0] == form]
        bars[form] = (round_up_1(MARGIN * max(r[3] for r in mine)), round_up_1(MARGIN * max(r[4] for r in mine)))
        worst = max(mine, key=lambda r: r[3])
        lines.append("bar %s %g" % (form, bars[form][0]))
        lines.append("worst %s err=%.3g at %s family %s loss_err=%.3g min_sensitivity=%.3g" % (
            form, worst[3], "x".join(map(str, worst[1])), worst[2], max(r[4] for r in mine), min(r[5] for r in mine)))
    for form, shape, family, err, loss_err, sens, bound in rows:
        ok = sens >= CONDITION * bars[form][0]
        if not ok:
            failed.append((form, shape, family, sens))
        lines.append("row %s %s %s err=%.3g loss_err=%.3g sensitivity%s%.3g%s" % (
            form, "x".join(map(str, shape)), family, err, loss_err, ">=" if bound else "=", sens, "" if ok else " BELOW-4-BAR"))
    with open(OUT, "w") as f:
        f.write("\n".join(lines + kept) + "\n")
    print("\n".join(ln for ln in lines if not ln.startswith("row ")))
    if failed:
        raise SystemExit("sensitivity below %d x bar: %s" % (CONDITION, failed))


if __name__ == "__main__":
    main()
