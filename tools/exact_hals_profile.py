"""The CPU half of profiles/exact_hals.txt: per row of tests/exact_problems.HALS_SHAPES, half and regulariser pair, the float32 model's
worst element-wise distance from the fp64 restatement of the sweep (hals_gram_form.w_half / h_half) in units of the fp32 spacing at
scale = max(|value before the clamp|, |old value|), the shares of strictly positive and clamped elements (for H also among the last
L - 1 columns), the largest contraction in absolute sums, and for the H half the float32 model's relative error of the loss; then the
bars: 4 times the worst model error of each half, at least 8 (the loss: 4 times the worst model, no floor).  In a second pass, AT those
bars: the elements that decide their clamp within the bar (excused from the zero-pattern check), the closest of the others, and the
elements whose zero pattern differs between the model and fp64.

    python tools/exact_hals_profile.py > rows.txt      (the `row` and `bar` lines; the `gpu` lines come from the GPU test's output)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_problems as ep  # noqa: E402

KEYS = ("model", "pos", "clamp", "edge_pos", "edge_clamp", "abs_sum", "close", "min_pre", "zero_mismatch", "loss_model")


def model_values(family, W, H, X, reg, a):
    """model (and loss_model) of one `row` line and the model's zero pattern, from the fp64 half a."""
    m = ep.hals_half(family, W, H, X, reg, np.float32)
    b = dict(model=float(ep.hals_units(m["new"], a).max()))
    if family == "H":
        b["loss_model"] = abs(m["loss"] - a["loss"]) / a["loss"]
    return b, m["new"] > 0


def bar_values(family, a, model_positive, bar):
    """The values of a `row` line that depend on the half's bar, and the preconditions."""
    b = ep.hals_preconditions(family, a, bar)
    b["zero_mismatch"] = int((model_positive != (a["new"] > 0)).sum())
    return b


def main():
    kept = []
    for N, T, K, L in [s[:4] for s in ep.HALS_SHAPES]:
        for family in ("W", "H"):
            W, H, X = ep.make_hals_problem(N, T, K, L, family)
            for r, reg in enumerate(ep.HALS_REGS):
                a = ep.hals_half(family, W, H, X, reg)
                b, positive = model_values(family, W, H, X, reg, a)
                small = {k: a[k] for k in ("W", "H", "R", "pre", "scale", "diag", "new") + (("Hu", "HH") if family == "W" else ("PW",))}
                kept.append((f"{N}x{T}x{K}x{L}", family, r, b, small, positive))
    bars = {f: max(ep.HALS_BAR_FLOOR, ep.HALS_BAR_FACTOR * max(k[3]["model"] for k in kept if k[1] == f)) for f in "WH"}
    for shape, family, r, b, a, positive in kept:
        b.update(bar_values(family, a, positive, bars[family]))
        print(f"row {shape} {family} reg{r} " + " ".join(f"{k}={b[k]:.6g}" for k in KEYS if k in b), flush=True)
    for f in "WH":
        print(f"bar {f} {bars[f]:.6g}")
    print(f"bar loss {ep.HALS_BAR_FACTOR * max(k[3]['loss_model'] for k in kept if k[1] == 'H'):.6g}")


if __name__ == "__main__":
    main()
