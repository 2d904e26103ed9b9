#!/usr/bin/env python3
"""Bit-level digest of the PGD rule on a lone handle and on T-sharded groups, half-step by half-step.

    python3 tools/pgd_digest.py [--full] > digest.txt

One line per case: per half-step `W:H`, the SHA-256 (first 8 hex digits) of the bytes of W and of H after it; `steps`, the digest of
rule.steps after every half-step; `loss`, the digest of the returned losses; `n`, the digest of the non-zero launch and collective
counters (cmf_get_counter), whose text stands once in the legend at the end.  --full prints steps, losses and counters themselves (a
line is then some 600 characters long: to find what differs, not to keep).  Two builds of the library compute the same thing through
the same launches exactly when their outputs are the same text: run it on both and `diff` (profiles/pgd_once_digest_*.txt).  The cases: the
shapes (48, 300, 4, 8), (96, 1000, 32, 12), (37, 150, 33, 7) (few components / the one-wave tiles with their cut tail / the general-K
kernel) x a lone handle, devices=[0, 0], devices=[0, 0, 0] x SquareLoss, AbsoluteLoss, each with and without a MaskedLoss mask x
Nonneg / UnitNorm / no constraint on both factors x three drives: three iterations call by call (the H half transposes the resident
residual), the H half first (est is void: the transposing residual conv), and the calls of an eval_mode=True fit (H halves only).
Non-zero penalties once per shape and handle; one row with the recording sharded on one device (CMF_TEST_HOOKS=1 CMF_MAX_COLUMNS=300).
Data and factors come from gen_synthetic / init_rand: nothing is an integer.
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
HANDLES = [None, [0, 0], [0, 0, 0]]
LOSSES = ["square", "abs", "square+mask", "abs+mask"]
CONSTRAINTS = [("nonneg", cmf.NonnegConstraint), ("unitnorm", cmf.UnitNormConstraint), ("none", None)]
DRIVES = ["calls", "h_first", "eval"]
COUNTERS = ["launches:" + p for p in LAUNCH_PATHS] + ["allreduce_calls", "allgather_calls"]
_PROBLEMS = {}


def problem(shape):
    if shape not in _PROBLEMS:
        N, T, K, L = shape
        data = cmf.gen_synthetic(N=N, T=T, K=3, L=L, seed=1234 + N)
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=T)
        mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=K)
        losses = {"square": cmf.SquareLoss(), "abs": cmf.AbsoluteLoss()}
        losses.update({k + "+mask": cmf.MaskedLoss(v, mask) for k, v in list(losses.items())})
        _PROBLEMS[shape] = (data, W0, H0, losses)
    return _PROBLEMS[shape]


FULL = "--full" in sys.argv
_LEGEND = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()[:8]


def counter(rule, name):
    try:
        return rule.counter(name)
    except cmf.CMFError:  # (the collective counters exist on groups only)
        return 0


def run(shape, devices, loss, constraint, drive, penalties=False, tag=""):
    data, W0, H0, losses = problem(shape)
    penW = [cmf.SquarePenalty(0.3), cmf.AbsolutePenalty(0.02)] if penalties else None
    penH = [cmf.SquarePenalty(0.05), cmf.AbsolutePenalty(0.01)] if penalties else None
    rule = cmf.PGDUpdate(data, W0, H0, devices=devices)
    halves, steps, lh = [], [], []
    try:
        def half(which):
            if which == "W":
                rule.update_motifs(loss_func=losses[loss], constrW=constraint[1], penaltiesW=penW)
            else:
                lh.append(rule.update_feature_maps(loss_func=losses[loss], constrH=constraint[1], penaltiesH=penH))
            W, H = rule.download()
            halves.append(f"{which} {sha(W)}:{sha(H)}")
            steps.extend(rule.steps)

        for which in {"calls": "WHWHWH", "h_first": "HWHWHW", "eval": "HHH"}[drive]:
            half(which)
        counts = " ".join(f"{c}={v}" for c, v in ((c, counter(rule, c)) for c in COUNTERS) if v)
    finally:
        rule.close()
    n = hashlib.sha256(counts.encode()).hexdigest()[:8]
    _LEGEND[n] = counts
    tail = (f"steps {' '.join(repr(x) for x in steps)} | loss {' '.join(repr(x) for x in lh)} | {counts}" if FULL
            else f"steps {sha(steps)} loss {sha(lh)} n {n}")
    print(f"{','.join(map(str, shape))} {'devices=' + str(devices).replace(' ', '') if devices else 'lone'} {loss} {constraint[0]} {drive}"
          f"{' penalties' if penalties else ''}{tag} | {' '.join(halves)} | {tail}", flush=True)


def main():
    for shape in SHAPES:
        for devices in HANDLES:
            for loss in LOSSES:
                for constraint in CONSTRAINTS:
                    for drive in DRIVES:
                        run(shape, devices, loss, constraint, drive)
            run(shape, devices, "abs+mask", CONSTRAINTS[0], "calls", penalties=True)
    os.environ["CMF_TEST_HOOKS"] = "1"  # a recording longer than a handle holds: cmf_create shards it on one device
    os.environ["CMF_MAX_COLUMNS"] = "300"
    try:
        run(SHAPES[1], None, "square+mask", CONSTRAINTS[1], "calls", tag=" CMF_MAX_COLUMNS=300")
    finally:
        os.environ.pop("CMF_MAX_COLUMNS")
        os.environ.pop("CMF_TEST_HOOKS")
    if not FULL:
        for n, counts in sorted(_LEGEND.items()):
            print(f"n {n} = {counts}")


if __name__ == "__main__":
    main()
