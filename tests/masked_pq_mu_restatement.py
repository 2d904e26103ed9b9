"""The Itakura-Saito and beta forms of the MU rule under a 0/1 mask, restated literally in numpy (the reference for
tests/test_masked_pq_mu_cpu.py, tests/test_gpu_masked_pq_mu.py, tools/mu_masked_pq_precision.py and
tests/golden/make_golden_masked_pq_mu.py).

Notation of tests/is_mu_restatement.py, tests/beta_mu_restatement.py and tests/masked_kl_mu_restatement.py: M is N x T of 0 and 1
(1 = observed), eps = eps(Float64), e = tensor_conv(W, H) + eps.  ``beta`` is 0 for Itakura-Saito (whose own composition of P, Q and
of the loss term is used, as on the device) and the beta of the beta-divergence otherwise.

    Q = M .* e.^(beta - 1)           (Itakura-Saito: M ./ e)
    P = M .* data .* e.^(beta - 2)   (Itakura-Saito: (data .* Q) .* Q where M == 1)
    both EXACTLY 0 where M == 0, by a select: what data holds there (NaN, Inf, negatives) never enters
    update_motifs!, update_feature_maps!:  the contractions and the step (exponent gamma(beta), 1/2 for Itakura-Saito) of the
                                           unmasked form, taken on this (P, Q)
    loss = sum over the entries with M == 1 of d_beta(data | e) / #{M == 1}        (e from the new H)

Data must pass the form's check WHERE OBSERVED (Itakura-Saito: finite and > 0; beta: finite and >= 0).  A unit or a sample with
nothing observed is legal: both sums are 0 there and the factor entries fall to eps.  With an all-ones mask this is the unmasked
restatement.

`cdtype` / `edtype`: the number formats of the contractions and of the epilogue, as in the two unmasked restatements.
"""
import numpy as np

import beta_mu_restatement as br
import is_mu_restatement as ir
import masked_kl_mu_restatement as mk
from kl_mu_restatement import hxt, tensor_conv, tensor_transconv

EPS = ir.EPS
REG = mk.REG
SHAPES = mk.SHAPES
MASKS = mk.MASKS
make_mask = mk.make_mask
BETAS = (0.0, 0.5, 1.5)           # on every shape (0: Itakura-Saito)
BETAS_FIRST = (0.25, 2.0, 3.0)    # on the first shape only


def form_name(beta):
    return "is" if beta == 0 else "beta"


def case_name(shape, kind, reg, beta):
    """The name a synthetic case goes by in profiles/mu_masked_pq_precision.txt."""
    return "synthetic(%d,%d,%d,%d):%s%s:b%03d" % (tuple(shape) + (kind, ":reg" if reg else "", int(round(100 * beta))))


def fixture_name(shape, kind, reg, beta):
    """tests/golden/mu_masked_is_<shape>_<mask>[_reg].npz / mu_masked_beta_<shape>_<mask>[_reg]_bNNN.npz"""
    stem = "mu_masked_%s_%s_%s%s" % (form_name(beta), "x".join(str(int(v)) for v in shape), kind, "_reg" if reg else "")
    return stem + (".npz" if beta == 0 else "_b%03d.npz" % int(round(100 * beta)))


def synthetic_case(shape, kind):
    """(data with NaN under the mask, its clean copy, mask, W0, H0) of a shape of SHAPES under one of MASKS, regenerated from seeds:
    strictly positive uint8-valued data (is_mu_restatement.positive_problem: legal for every beta) and float16-valued factors."""
    N, T, K, L = shape
    data, W0, H0 = ir.positive_problem(N, T, K, L, seed=7)
    clean = np.asfortranarray(data.astype(np.float64))
    mask = make_mask(kind, N, T, L)
    return (np.where(mask != 0, clean, np.nan), clean, mask, np.asfortranarray(W0.astype(np.float64)),
            np.asfortranarray(H0.astype(np.float64)))


def check_data(data, mask, beta):
    """The form's check over the observed entries alone; returns (select(mask, data, 1), observed count).  (The 1 under the mask is
    a placeholder the selects below never let through.)"""
    mask = np.asarray(mask, dtype=np.float64)
    if not np.isin(mask, (0.0, 1.0)).all():
        raise ValueError("mask must hold 0 and 1 only")
    if not mask.any():
        raise ValueError("the mask observes nothing")
    obs = mask != 0
    x = np.asarray(data, dtype=np.float64)[obs]
    if beta == 0:
        bad = int(np.sum(~(np.isfinite(x) & (x > 0))))
        if bad:
            raise ValueError(f"{ir.MESSAGE} ({bad} entries are zero, negative, NaN or infinite): add a small floor to the spectrogram")
    else:
        bad = int(np.sum(~(np.isfinite(x) & (x >= 0))))
        if bad:
            raise ValueError(f"{br.MESSAGE} ({bad} entries are negative, NaN or infinite)")
    return np.where(obs, np.asarray(data, dtype=np.float64), 1.0), int(obs.sum())


def pq(xs, mask, W, H, beta, cdtype=np.float64, edtype=np.float64):
    """(P, Q) of the form on select(mask, data, 1), then selected to exact 0 where mask == 0."""
    P, Q = ir.pq(xs, W, H, cdtype, edtype) if beta == 0 else br.pq(xs, W, H, beta, cdtype, edtype)
    obs = np.asarray(mask) != 0
    return np.where(obs, P, 0.0), np.where(obs, Q, 0.0)


def term_array(x, e, beta, edtype=np.float64):
    """d_beta(x | e) per entry in the device's composition (Itakura-Saito: (r - 1) - log(r), r = x * (1 / e) in float32, x / e in fp64)."""
    if beta == 0:
        x, e = x.astype(edtype), e.astype(edtype)
        r = x * (edtype(1.0) / e) if edtype is not np.float64 else x / e
        return ((r - edtype(1.0)) - np.log(r)).astype(np.float64)
    return br.terms(x, e, beta, edtype).astype(np.float64)


def divergence_sum(data, mask, W, H, beta, complement=False, cdtype=np.float64, edtype=np.float64):
    """(sum of d_beta(data | e), number of entries) over mask == 1 (complement: mask == 0), by select."""
    sel = (np.asarray(mask) == 0) if complement else (np.asarray(mask) != 0)
    e = tensor_conv(W, H, cdtype).astype(edtype) + edtype(EPS)
    x = np.where(sel, np.asarray(data, dtype=np.float64), 1.0)
    t = term_array(x, e, beta, edtype)
    return float(np.sum(np.where(sel, t, 0.0))), int(sel.sum())


heldout_sums = divergence_sum


def masked_loss(xs, mask, count, W, H, beta, cdtype=np.float64, edtype=np.float64):
    return divergence_sum(xs, mask, W, H, beta, False, cdtype, edtype)[0] / count


def _gamma(beta):
    return 0.5 if beta == 0 else br.gamma(beta)


def _step(x, num, den, g):
    q = num / den
    x *= q if g == 1.0 else (np.sqrt(q) if g == 0.5 else q ** g)
    np.maximum(x, EPS, out=x)
    return x


def update_motifs(xs, mask, W, H, beta, l1W=0.0, l2W=0.0, cdtype=np.float64, edtype=np.float64):
    L = W.shape[2]
    P, Q = pq(xs, mask, W, H, beta, cdtype, edtype)
    numW = hxt(H, P, L, cdtype)
    denomW = hxt(H, Q, L, cdtype)
    return _step(W, numW, ((denomW + l1W) + (2.0 * l2W) * W) + EPS, _gamma(beta))


def update_feature_maps(xs, mask, count, W, H, beta, l1H=0.0, l2H=0.0, cdtype=np.float64, edtype=np.float64):
    P, Q = pq(xs, mask, W, H, beta, cdtype, edtype)
    numH = tensor_transconv(W, P, cdtype)
    denomH = tensor_transconv(W, Q, cdtype)
    _step(H, numH, ((denomH + l1H) + (2.0 * l2H) * H) + EPS, _gamma(beta))
    return masked_loss(xs, mask, count, W, H, beta, cdtype, edtype)


def fit_masked_pq(data, mask, W_init, H_init, beta, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64,
                  edtype=np.float64):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations.  beta = 0: Itakura-Saito."""
    if beta != 0:
        br.check_beta(beta)
    xs, count = check_data(data, mask, beta)
    mask = np.asarray(mask, dtype=np.float64)
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [masked_loss(xs, mask, count, W, H, beta, cdtype, edtype)]
    for _ in range(int(max_itr)):
        update_motifs(xs, mask, W, H, beta, l1W=l1W, l2W=l2W, cdtype=cdtype, edtype=edtype)
        loss_hist.append(update_feature_maps(xs, mask, count, W, H, beta, l1H=l1H, l2H=l2H, cdtype=cdtype, edtype=edtype))
    return W, H, np.asarray(loss_hist)


def load_fixture(path):
    """A tests/golden/mu_masked_is_* / mu_masked_beta_* file with its inputs regenerated from seeds (the file holds none): the shape,
    the mask kind, beta, the regularisers, max_itr, loss_hist and W and H as float32 roundings (W32 / H32: 6e-8 relative)."""
    g = np.load(path)
    shape = tuple(int(v) for v in g["shape"])
    kind = str(g["kind"])
    data, clean, mask, W0, H0 = synthetic_case(shape, kind)
    out = dict(shape=shape, kind=kind, data=data, clean=clean, mask=mask, W0=W0, H0=H0, beta=float(g["beta"]), max_itr=int(g["max_itr"]),
               loss_hist=np.asarray(g["loss_hist"], dtype=np.float64), reg={k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")})
    import os

    w = g if "W32" in g.files else np.load(os.path.join(os.path.dirname(path), str(g["W_file"])))  # (a companion file where both would not fit)
    out["W"], out["H"] = np.asarray(w["W32"], dtype=np.float64), np.asarray(g["H32"], dtype=np.float64)
    return out
