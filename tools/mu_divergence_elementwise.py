#!/usr/bin/env python3
"""The element-wise bar of tests/test_gpu_divergence_paths.py, measured on the CPU (writes profiles/mu_divergence_elementwise.txt).

On the integer problems of tests/exact_problems.py est = tensor_conv(W, H) is exact in fp32, so what separates the device from the
fp64 restatement in ONE update of a divergence form is the fp32 epilogue that forms R / P / Q, the fp32 contraction of those with the
other factor, and the element-wise step.  For every (form, shape, family) of the shared table (exact_problems.SHAPES; family "W": one
update_motifs!, family "H": one update_feature_maps! and its loss; KL, masked KL and the beta forms a second time with zeros in the
data; Itakura-Saito and beta = 0.5 on data relative to est; Itakura-Saito, beta = 0.5 and beta = 1.5 once more under the 0/1 mask, by
tests/masked_pq_mu_restatement.py: exact_problems.FORMS) the restatement is run with cdtype = edtype = float32 against its fp64 run, and a `row` line records

    err          the largest element-wise relative error of the updated factor
    loss_err     the relative error of the loss (family "H")
    sensitivity  exact_problems.sensitivity: the smallest relative change of an element when one positive term of its numerator or
                 denominator sum is removed (`>=`: the closed-form lower bound was enough)

`bar <form> <value>`: 8 x the largest err of the form, rounded UP to one significant digit; `lossbar <form> <value>` the same from
loss_err.  The factor 8 is for what the model leaves out: v_rcp_f32 / v_log_f32 / v_exp_f32 at about 1 ulp each, the order of the
sums, the fp32 step.  The condition -- not a measurement -- is sensitivity >= 4 x bar on every row; the tool fails when a row misses
it (narrow the data range or change the row: the bar is never raised), and the GPU test asserts it again from its own arrays.

`gpu <form> <value>` / `gpuloss <form> <value>` lines are what an MI355X run of the test observed (the worst element per form); they
are appended by hand from the test's output and kept when the tool rewrites the file.

    python tools/mu_divergence_elementwise.py [-j PROCESSES]
"""
import math
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")  # (one process per shape: the BLAS threads would fight each other)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exact_problems as ep  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mu_divergence_elementwise.txt")
MARGIN = 8
CONDITION = 4
EXACT_BELOW = 1e-4  # the closed-form lower bound of the sensitivity is replaced by the exact value when it is below this


def variants():
    return [(form, z) for form, f in ep.FORMS.items() for z in ((False, True) if f[3] else (False,))]


def round_up_1(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def one_shape(shape):
    N, T, K, L = shape
    rows = []
    for family in ("W", "H"):
        for zeros, relative in ((False, False), (True, False), (False, True), (True, True)):
            W, H, X, mask = ep.make_divergence_problem(N, T, K, L, family, zeros=zeros, relative=relative)
            for form, z in variants():
                if z != zeros or ep.FORMS[form][4] != relative:
                    continue
                a = ep.divergence_half(form, family, X, mask, W, H)
                m = ep.divergence_half(form, family, X, mask, W, H, cdtype=np.float32, edtype=np.float32)
                err = float(ep.rel_err(m["new"], a["new"]).max())
                loss_err = abs(m["loss"] - a["loss"]) / a["loss"] if family == "H" else 0.0
                sens, bound = ep.sensitivity(form, a, exact=False), True
                if sens < EXACT_BELOW:
                    sens, bound = ep.sensitivity(form, a), False
                rows.append((form, zeros, shape, family, err, loss_err, sens, bound))
    return rows


def main():
    jobs = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else min(8, os.cpu_count() or 1)
    shapes = sorted({s[:4] for s in ep.SHAPES}, key=lambda s: -s[0] * s[1] * s[3])
    if jobs > 1:
        from multiprocessing import Pool

        with Pool(jobs) as pool:
            rows = [r for part in pool.imap_unordered(one_shape, shapes) for r in part]
    else:
        rows = [r for s in shapes for r in one_shape(s)]
    order = {s[:4]: i for i, s in enumerate(ep.SHAPES)}
    rows.sort(key=lambda r: (list(ep.FORMS).index(r[0]), r[1], order[r[2]], r[3]))
    kept = [ln for ln in (open(OUT).read().splitlines() if os.path.exists(OUT) else []) if ln.split()[:1] and ln.split()[0] in ("gpu", "gpuloss")]
    lines = ["# tools/mu_divergence_elementwise.py: the restatements with float32 contractions and a float32 epilogue against their fp64 runs,",
             "# one update per (form, shape, family) of tests/exact_problems.py SHAPES; data in {%d ... %d} (+zeros: one entry in eight 0)." % (ep.DIV_XMIN, ep.DIV_XMAX),
             "# bar = %d x the largest err of the form, rounded up to one significant digit; condition: sensitivity >= %d x bar on every row." % (MARGIN, CONDITION)]
    bars, failed = {}, []
    for form in ep.FORMS:
        mine = [r for r in rows if r[0] == form]
        bars[form] = (round_up_1(MARGIN * max(r[4] for r in mine)), round_up_1(MARGIN * max(r[5] for r in mine)))
        worst = max(mine, key=lambda r: r[4])
        lines.append("bar %s %g" % (form, bars[form][0]))
        lines.append("lossbar %s %g" % (form, bars[form][1]))
        lines.append("worst %s err=%.3g at %s family %s%s loss_err=%.3g min_sensitivity=%.3g" % (
            form, worst[4], "x".join(map(str, worst[2])), worst[3], " +zeros" if worst[1] else "", max(r[5] for r in mine), min(r[6] for r in mine)))
    for form, zeros, shape, family, err, loss_err, sens, bound in rows:
        ok = sens >= CONDITION * bars[form][0]
        if not ok:
            failed.append((form, zeros, shape, family, sens))
        lines.append("row %s%s %s %s err=%.3g loss_err=%.3g sensitivity%s%.3g%s" % (
            form, "+zeros" if zeros else "", "x".join(map(str, shape)), family, err, loss_err, ">=" if bound else "=", sens, "" if ok else " BELOW-4-BAR"))
    with open(OUT, "w") as f:
        f.write("\n".join(lines + kept) + "\n")
    print("\n".join(ln for ln in lines if not ln.startswith("row ")))
    if failed:
        raise SystemExit("sensitivity below %d x bar: %s" % (CONDITION, failed))


if __name__ == "__main__":
    main()
