#!/usr/bin/env python3
"""Bit-level digest of the MU rule's eight forms (square, KL, Itakura-Saito and beta = 0.5, each with and without a mask) through every driver.

    python3 tools/mu_forms_digest.py > digest.txt

One line per case: the SHA-256 (first 16 hex digits) of the bytes of W, of H and of the loss array, and the non-zero launch
counters (cmf_get_counter).  Two builds of the library compute the same thing through the same launches exactly when their outputs
are the same text: run it on both and `diff` (profiles/mu_forms_digest_*.txt).  The cases: the forms x the shapes (48, 300, 4, 8),
(96, 1000, 32, 12), (37, 150, 33, 7) (few components / the one-wave tiles with their cut tail / the general-K kernel) x reuse_est 1, 0
x three iterations call by call, cmf_iterate(3), cmf_fit(max_itr = 3); option conv_kernel = 2 at K = 32; cmf_masked_loss with both
values of `complement` under the four masked forms; non-zero l1 / l2 once per form.  Data is strictly positive (Itakura-Saito accepts
it) and comes, like the initial factors, from the library's counter RNG.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402
from exact_problems import LAUNCH_PATHS  # noqa: E402

SHAPES = [(48, 300, 4, 8), (96, 1000, 32, 12), (37, 150, 33, 7)]
FORMS = [("square", ":square", False), ("square+mask", ":square", True), ("kl", ":kl", False), ("kl+mask", ":kl", True),
         ("is", ":itakura_saito", False), ("is+mask", ":itakura_saito", True), ("beta", ":beta", False), ("beta+mask", ":beta", True)]
COUNTERS = ["launches:" + p for p in LAUNCH_PATHS] + ["speculated_contractions", "small_k_fused_h_updates"]
REG = dict(l1W=0.01, l2W=0.02, l1H=0.03, l2H=0.005)
_PROBLEMS = {}


def problem(shape):
    if shape not in _PROBLEMS:
        N, T, K, L = shape
        data = np.maximum(cmf.gen_synthetic(N=N, T=T, K=3, L=L, seed=1234 + N), 0.0) + 0.05
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=T)
        _PROBLEMS[shape] = (data, W0, H0, cmf.holdout_mask(N, T, frac=0.2, block=L, seed=K))
    return _PROBLEMS[shape]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()[:16]


def make_rule(shape, kind, masked, options):
    data, W0, H0, mask = problem(shape)
    rule = cmf.MultUpdate(data, W0, H0)
    rule.set_option("kl_mask", 1)
    rule.set_option("pq_mask", 1)
    for k, v in options.items():
        rule.set_option(k, v)
    rule.set_divergence(kind, beta=0.5 if kind == ":beta" else None)
    if masked:
        rule.set_mask(mask)
    return rule


def run(shape, form, driver, options, reg, held_out=False):
    name, kind, masked = form
    rule = make_rule(shape, kind, masked, options)
    try:
        if driver == "calls":
            lh = [rule.compute_loss()]
            for _ in range(3):
                rule.update_motifs(l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
                lh.append(rule.update_feature_maps(l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0)))
        elif driver == "iterate":
            lh = [rule.compute_loss()] + list(rule.iterate(3, **reg))
        else:
            lh, _, _ = rule.fit_native(3, np.inf, False, 3, 1e-4, False, **reg)
        if held_out:
            lh = list(lh) + list(rule.masked_loss(False)) + list(rule.masked_loss(True)) + [rule.update_feature_maps()]
        W, H = rule.download()
        counts = " ".join(f"{c}={v}" for c, v in ((c, rule.counter(c)) for c in COUNTERS) if v)
    finally:
        rule.close()
    opts = ",".join(f"{k}={v}" for k, v in options.items()) or "-"
    print(f"{name} {shape} {driver} {opts} reg={'yes' if reg else 'no'}{' held_out' if held_out else ''} | W {sha(W)} H {sha(H)} "
          f"loss {sha(lh)} | {counts}", flush=True)


def main():
    for form in FORMS:
        for shape in SHAPES:
            for reuse in (1, 0):
                for driver in ("calls", "iterate", "fit"):
                    run(shape, form, driver, dict(reuse_est=reuse), {})
        for reuse in (1, 0):  # the 128 x 128 tiles where the mode has them
            run(SHAPES[1], form, "iterate", dict(conv_kernel=2, reuse_est=reuse), {})
        for shape in SHAPES:
            run(shape, form, "iterate", {}, REG)
        if form[2]:
            for shape in SHAPES:
                for reuse in (1, 0):
                    run(shape, form, "calls", dict(reuse_est=reuse), {}, held_out=True)


if __name__ == "__main__":
    main()
