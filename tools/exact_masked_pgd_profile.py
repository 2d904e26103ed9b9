"""The CPU half of profiles/exact_masked_pgd.txt: per row of tests/exact_problems.SHAPES, family and variant, the float32 model's worst
distance from the fp64 PGD half-step in ulp (fused and unfused), one unit of a contraction in ulp (pgd_preconditions "units"), the step
against the smallest updated entry; for the masked MU rule the largest masked sum and the fewest observed terms of an element.

    python tools/exact_masked_pgd_profile.py > rows.txt      (the `row` lines; the `gpu` lines come from the GPU tests' output)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_problems as ep  # noqa: E402


def main():
    for N, T, K, L in [s[:4] for s in ep.SHAPES]:
        shape = f"{N}x{T}x{K}x{L}"
        for family in ("W", "H"):
            W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
            for variant in ep.pgd_variants(N):
                a = ep.pgd_half(variant, family, W, H, X, mask)
                b = ep.assert_pgd_preconditions(a, X, mask, f"{shape} {family} {variant}")
                worst = max(float(ep.ulps(ep.pgd_f32_model(a, f), a["new"]).max()) for f in (False, True))
                print(f"row pgd {shape} {family} {variant} model_ulp={worst:.3f} units={b['units']:.1f} alpha_g={b['alpha_g']:.3f} "
                      f"min_new={b['min_new']:.3f} abs_sum={b['absG']:.0f} sumsq={b['sumsq']:.0f}", flush=True)
            W, H, X = ep.make_problem(N, T, K, L, family)
            a = ep.masked_mu_half(family, W, H, X, ep.mu_mask(N, T))
            seen = ep.assert_masked_mu_preconditions(a, f"{shape} {family}")
            unobserved = int((seen == 0).sum())
            print(f"row masked_mu {shape} {family} mask max_sum={max(a['num'].max(), a['den'].max()):.0f} min_observed={seen[seen > 0].min():.0f} unobserved={unobserved} "
                  f"model_ulp={float(ep.ulps(a['new'].astype(np.float32), a['new']).max()):.3f}", flush=True)


if __name__ == "__main__":
    main()
