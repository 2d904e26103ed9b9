"""The Itakura-Saito and beta forms of the MU rule UNDER A 0/1 MASK on the integer problems of tests/exact_problems.py (the fp64 half
for tests/test_gpu_masked_pq_mu.py and tools/mu_masked_pq_elementwise.py).

est = tensor_conv(W, H) is a small integer, exact in fp32 on every conv path, so P and Q are element-wise functions of exact operands
and the select that zeroes the held-out entries is exact: the updated factor is compared with fp64 per element at a bar near fp32
rounding (profiles/mu_masked_pq_elementwise.txt), far below what one missing or one surplus term moves (exact_problems.sensitivity).
A held-out entry that leaked into a sum would be such a surplus term.

The problems are exact_problems.make_divergence_problem's (its 0/1 mask in blocks of 1 x 8, a quarter held out), the data range the
unmasked form of the same beta uses there (exact_problems.FORMS: relative data for Itakura-Saito and beta = 0.5); the device is
given NaN under the mask.
"""
import numpy as np

import exact_problems as ep
import masked_pq_mu_restatement as pm

# form -> (the unmasked form of exact_problems.FORMS whose data range and step it shares, beta (0: Itakura-Saito))
FORMS = {"is_mask": ("is", 0.0), "beta050_mask": ("beta050", 0.5), "beta150_mask": ("beta150", 1.5)}
# the smallest rows of exact_problems.SHAPES that reach each conv path of the masked families under the row's configurations: conv3 in
# 16 pieces, in 4 pieces (conv_split = 4) and in whole tiles (conv_split = 0) and conv2 (conv_kernel = 2) at K = 32; conv_kernel at
# K = 20 with L <= 32 and L > 32; T shorter than 2 L; the few-component tiles with 1, 2 and 3 k pairs, in quarter pieces and whole
SHAPE_KEYS = [(130, 700, 32, 20), (70, 600, 20, 12), (70, 600, 20, 40), (30, 24, 32, 12), (31, 420, 2, 33), (48, 300, 4, 8), (250, 1500, 5, 20)]
SHAPES = [s for s in ep.SHAPES if s[:4] in SHAPE_KEYS]
assert len(SHAPES) == len(SHAPE_KEYS)


def make_problem(shape, family, form):
    """(W, H, X, mask, data): the integer problem of the form's unmasked twin; data is X with NaN under the mask."""
    W, H, X, mask = ep.make_divergence_problem(*shape, family, relative=ep.FORMS[FORMS[form][0]][4])
    return W, H, X, mask, np.asfortranarray(np.where(mask != 0, X, np.nan))


def masked_half(form, family, X, mask, W, H, cdtype=np.float64, edtype=np.float64):
    """exact_problems.divergence_half of the unmasked twin with P and Q selected to exact 0 under the mask and the loss taken over
    the observed entries (masked_pq_mu_restatement): one update_motifs! (family "W") or update_feature_maps! (family "H")."""
    base, beta = FORMS[form]
    obs = np.asarray(mask) != 0
    xs = np.where(obs, X, 1.0)  # (a placeholder under the mask that the selects never let through)

    def select(stage, a):
        if stage == "sources":
            a["P"], a["Q"] = np.where(obs, a["P"], 0.0), np.where(obs, a["Q"], 0.0)

    a = ep.divergence_half(base, family, xs, mask, W, H, cdtype, edtype, corrupt=select)
    if family == "H":
        a["loss"] = pm.divergence_sum(xs, mask, W, a["new"], beta, cdtype=cdtype, edtype=edtype)[0] / int(obs.sum())
    return a


def sensitivity(form, a, exact=True):
    return ep.sensitivity(FORMS[form][0], a, exact)


def read_bars(path):
    return ep.read_bars(path)
