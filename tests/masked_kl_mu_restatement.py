"""The KL form of the MU rule under a 0/1 mask, restated literally in fp64 numpy (the reference for
tests/test_masked_kl_mu_cpu.py, tests/test_gpu_masked_kl_mu.py and tests/golden/make_golden_masked_kl_mu.py).

Notation of tests/masked_mu_restatement.py and tests/kl_mu_restatement.py: M is N x T of 0 and 1 (1 = observed),
Xm = select(M, data, 0), eps = eps(Float64) (src/CMF.jl:20), e = tensor_conv(W, H) + eps.

    R = Xm ./ e                                   exactly 0 where M == 0, whatever data holds there (NaN, Inf, negatives)
    update_motifs!:        numW[:, :, l] = shift(H, l) R[:, 1+l:T]'            (mult.jl:32 with data -> R)
                           denomW[:, :, l] = shift(H, l) M[:, 1+l:T]'          (mult.jl:33 with est -> M: differs from n to n)
                           W .*= numW ./ (((denomW + l1W) + 2 l2W W) + eps);  W = max(eps, W)      (mult.jl:37-38 unchanged)
    update_feature_maps!:  R from the new W;  numH = transconv(W, R);  denomH = transconv(W, M);   (mult.jl:51-52 unchanged)
                           loss = D_M / sum(Xm)   (e from the new H)
    D_M = sum over the entries with M == 1 of (x > 0 ? x log(x / e) : 0) - x + e

Data must be finite and non-negative WHERE OBSERVED with sum(Xm) > 0.  A unit or a sample with nothing observed is legal:
numerator and denominator are both 0 there and the factor entries fall to eps.  With an all-ones mask this is the rule of
tests/kl_mu_restatement.py (whose denominators are these contractions written as sums: ones_denominators there).

`cdtype`: the number format the CONTRACTIONS are carried out in, as in kl_mu_restatement (tools/mu_masked_kl_precision.py).
`edtype` (ratio, divergence_sum and masked_kl_loss only): the number format of the epilogue that forms R and the loss terms, as there.
"""
import numpy as np

import kl_mu_restatement as kr
import masked_mu_restatement as mr

EPS = kr.EPS
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)  # (the regularisers of tests/test_gpu_masked_mu.py)
# the smallest shapes (N, T, K, L) that reach each conv path: conv_small with 2 k pairs | 3 k pairs, the preloaded data tile, several
# rounds | conv3 and conv2 (K % 32 == 0) | conv_kernel (any K) | L > 32 | T < L (twice)
SHAPES = [(48, 300, 4, 8), (250, 2000, 5, 20), (96, 1000, 32, 12), (37, 150, 33, 7), (20, 200, 6, 40), (6, 3, 2, 5), (20, 7, 2, 10)]
MASKS = ("blocks", "speckle", "dead")


def make_mask(kind, N, T, L):
    """The three masks of tests/test_gpu_masked_mu.py::make_mask: blocks of L at 20 %, 50 % speckle, and blocks with one unit and one
    sample never observed."""
    if kind == "blocks":
        m = mr.block_mask(N, T, 0.2, min(L, T), 11)
    elif kind == "speckle":
        m = mr.block_mask(N, T, 0.5, 1, 12)
    else:
        m = mr.block_mask(N, T, 0.2, min(L, T), 13)
        m[N // 2, :] = 0.0
        m[:, T // 3] = 0.0
    if not m.any():
        m[0, 0] = 1.0
    return np.asfortranarray(m)


def case_name(shape, kind, reg):
    """The name a synthetic case goes by in profiles/mu_masked_kl_precision.txt."""
    return "synthetic(%d,%d,%d,%d):%s%s" % (tuple(shape) + (kind, ":reg" if reg else ""))


def synthetic_case(shape, kind):
    """(data with NaN under the mask, its clean copy, mask, W0, H0) of a shape of SHAPES under one of MASKS.  The observed data
    keep a positive sum (an entry is set where the draw left none)."""
    N, T, K, L = shape
    clean, W0, H0 = kr.synthetic(N, T, K, L, seed=4)
    mask = make_mask(kind, N, T, L)
    if not select(mask, clean).sum() > 0:
        i, j = np.argwhere(mask != 0)[0]
        clean[i, j] = 1.0
    return np.where(mask != 0, clean, np.nan), clean, mask, W0, H0


def select(mask, a):
    """select(mask, a, 0): what `a` holds under mask == 0 (NaN, Inf) never enters."""
    return np.where(np.asarray(mask) != 0, a, 0.0)


class MaskedKL:
    """State of the rule: the mask, Xm and its sum (what installing the second of mask and divergence checks)."""

    def __init__(self, data, mask):
        mask = np.asarray(mask, dtype=np.float64)
        if not np.isin(mask, (0.0, 1.0)).all():
            raise ValueError("mask must hold 0 and 1 only")
        if not mask.any():
            raise ValueError("the mask observes nothing")
        self.mask = mask
        self.Xm = kr.check_data(select(mask, np.asarray(data, dtype=np.float64)))  # finite, non-negative, positive sum: where observed
        self.xm_sum = float(np.sum(self.Xm))


def ratio(rule, W, H, cdtype=np.float64, edtype=np.float64):
    """R = Xm ./ (tensor_conv(W, H) + eps)."""
    if edtype is np.float64:
        return rule.Xm / (kr.tensor_conv(W, H, cdtype) + EPS)
    return (rule.Xm.astype(edtype) / (kr.tensor_conv(W, H, cdtype).astype(edtype) + edtype(EPS))).astype(np.float64)


def divergence_sum(data, mask, est_eps, complement=False, edtype=np.float64):
    """The divergence terms summed over the entries with mask == 1 (complement: mask == 0), by select."""
    sel = (np.asarray(mask) == 0) if complement else (np.asarray(mask) != 0)
    x = np.where(sel, data, 0.0)
    pos = x > 0
    if edtype is not np.float64:  # (the terms in edtype, in the device's order, summed in fp64)
        xe, e = x.astype(edtype), est_eps.astype(edtype)
        q = np.where(pos, xe, edtype(1.0)) / np.where(pos, e, edtype(1.0))
        term = np.where(pos, xe * np.log(q), edtype(0.0)) + (e - xe)
        return float(np.sum(np.where(sel, term, edtype(0.0)).astype(np.float64)))
    q = np.where(pos, x, 1.0) / np.where(pos, est_eps, 1.0)
    term = np.where(pos, x * np.log(q), 0.0) - x + est_eps
    return float(np.sum(np.where(sel, term, 0.0)))


def masked_kl_loss(rule, W, H, cdtype=np.float64, edtype=np.float64):
    """D_M(data, tensor_conv(W, H) + eps) / sum(Xm)."""
    return divergence_sum(rule.Xm, rule.mask, kr.tensor_conv(W, H, cdtype) + EPS, edtype=edtype) / rule.xm_sum


def update_motifs(rule, W, H, l1W=0.0, l2W=0.0, cdtype=np.float64):
    """update_motifs! of the masked KL rule.  W in place."""
    L = W.shape[2]
    R = ratio(rule, W, H, cdtype)
    numW = kr.hxt(H, R, L, cdtype)  # mult.jl:32 with data -> R
    denomW = kr.hxt(H, rule.mask, L, cdtype)  # mult.jl:33 with est -> M
    den = ((denomW + l1W) + (2.0 * l2W) * W) + EPS  # :37
    W *= numW / den
    np.maximum(W, EPS, out=W)  # :38
    return W


def update_feature_maps(rule, W, H, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """update_feature_maps! of the masked KL rule.  H in place; returns the loss."""
    R = ratio(rule, W, H, cdtype)  # (e from the new W)
    numH = kr.tensor_transconv(W, R, cdtype)  # :47 with data -> R
    denomH = kr.tensor_transconv(W, rule.mask, cdtype)  # :48 with est -> M
    den = ((denomH + l1H) + (2.0 * l2H) * H) + EPS  # :51
    H *= numH / den
    np.maximum(H, EPS, out=H)  # :52
    return masked_kl_loss(rule, W, H, cdtype)  # (e from the new H)


def fit_masked_kl(data, mask, W_init, H_init, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations."""
    rule = MaskedKL(data, mask)
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [masked_kl_loss(rule, W, H, cdtype)]
    for _ in range(int(max_itr)):
        update_motifs(rule, W, H, l1W=l1W, l2W=l2W, cdtype=cdtype)
        loss_hist.append(update_feature_maps(rule, W, H, l1H=l1H, l2H=l2H, cdtype=cdtype))
    return W, H, np.asarray(loss_hist)


def heldout_sums(data, mask, W, H, complement=False):
    """(sum of the divergence terms, sum of data) over the entries with mask == 1, or with mask == 0 (complement): by select."""
    sel = (np.asarray(mask) == 0) if complement else (np.asarray(mask) != 0)
    return divergence_sum(data, mask, kr.tensor_conv(W, H) + EPS, complement), float(np.sum(np.where(sel, data, 0.0)))


def load_fixture(path, golden_dir=None):
    """A tests/golden/mu_masked_kl_*.npz file as float64 arrays.  The inputs (data, W0, H0) are those of the mu_kl_* fixture the
    file names (`inputs`); the file itself holds the packed mask, the regularisers, max_itr, loss_hist and W and H -- in fp64, as
    their float32 roundings (W32 / H32) or as their Frobenius norms only, in which case W and H are recomputed here and must
    reproduce the stored loss_hist and norms (kl_mu_restatement.load_fixture's three forms).  Data under mask == 0 is replaced
    by NaN: what the rule must never read."""
    import os

    g = np.load(path)
    src = np.load(os.path.join(golden_dir or os.path.dirname(path), str(g["inputs"]) + ".npz"))
    out = {k: np.asarray(src[k], dtype=np.float64) for k in ("data", "W0", "H0")}
    N, T = out["data"].shape
    out["mask"] = np.asfortranarray(np.unpackbits(g["mask_bits"])[: N * T].reshape(N, T).astype(np.float64))
    out["clean"] = out["data"]
    out["data"] = np.where(out["mask"] != 0, out["data"], np.nan)
    out["loss_hist"] = np.asarray(g["loss_hist"], dtype=np.float64)
    out["max_itr"] = int(g["max_itr"])
    out["reg"] = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")}
    out["inputs"] = str(g["inputs"])
    out["exact"] = "W" in g.files
    if "W" in g.files or "W32" in g.files:
        out["W"] = np.asarray(g["W"] if "W" in g.files else g["W32"], dtype=np.float64)
        out["H"] = np.asarray(g["H"] if "H" in g.files else g["H32"], dtype=np.float64)
    else:
        W, H, lh = fit_masked_kl(out["data"], out["mask"], out["W0"], out["H0"], max_itr=out["max_itr"], **out["reg"])
        np.testing.assert_allclose(lh, out["loss_hist"], rtol=1e-10)
        np.testing.assert_allclose([np.linalg.norm(W), np.linalg.norm(H)], [float(g["W_norm"]), float(g["H_norm"])], rtol=1e-10)
        out["W"], out["H"] = W, H
    return out
