"""The MU rule under a mask, restated literally in fp64 numpy (the reference for tests/test_masked_mu_cpu.py,
tests/test_gpu_masked_mu.py and tests/golden/make_golden_masked_mu.py).

It is src/algs/mult.jl:23-58 with data -> Xm = select(mask, data, 0) and est -> mask .* est wherever the rule reads them:

    update_motifs!:        est = M .* conv(W, H);  numW[:, :, l] = shift(H, l) Xm[:, 1+l:T]';  denomW[:, :, l] = shift(H, l) est[:, 1+l:T]'
                           W .*= numW ./ (denomW + l1W + 2 l2W W + eps);  W = max(eps, W)
    update_feature_maps!:  est = M .* conv(W, H);  numH = transconv(W, Xm);  denomH = transconv(W, est);  the same update of H
                           loss = norm(M .* (conv(W, H) - data)) / norm(Xm)

which is the multiplicative update of norm(M .* (data - conv(W, H)))^2 (MaskedLoss, pgd.jl:58-70, for the MU rule).  The
operations follow oracle/cmf_oracle.py's MU rule in the same order, so that an all-ones mask reproduces it (bit for bit with
LITERAL_SLICES, below).

`cdtype`: the number format the CONTRACTIONS (conv, transconv, the numW / denomW products) are carried out in; float32 models the
device's arithmetic (tools/mu_masked_precision.py measures how far that drifts from fp64).  Everything else stays fp64.

LITERAL_SLICES: the oracle multiplies the strided slices W[:, :, lag] as they are, which numpy cannot hand to BLAS (a plain loop,
~1 GFLOP/s).  True keeps that -- the operation order of the oracle, bit for bit; False (default) copies each slice first so that the
products run in BLAS (another summation order inside the product: agrees with the literal form to ~1e-15 relative per product,
tests/test_masked_mu_cpu.py holds the two together), which is what lets the tests afford 100-iteration fits and config 2.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)  # eps(): src/CMF.jl:20
LITERAL_SLICES = False


def _lag(Wc, lag):
    return Wc[:, :, lag] if LITERAL_SLICES else np.ascontiguousarray(Wc[:, :, lag])


def _c(a, cdtype):
    return a.astype(cdtype, copy=False)


def tensor_conv(W, H, cdtype=np.float64):
    """tensor_conv!: src/common.jl:24-34."""
    K, N, L = W.shape
    T = H.shape[1]
    est = np.zeros((N, T))
    Wc, Hc = _c(W, cdtype), _c(H, cdtype)
    for lag in range(min(L, T)):
        est[:, lag:] += (_lag(Wc, lag).T @ Hc[:, : T - lag]).astype(np.float64, copy=False)
    return est


def tensor_transconv(W, X, cdtype=np.float64):
    """tensor_transconv!: src/common.jl:71-81."""
    K, N, L = W.shape
    T = X.shape[1]
    res = np.zeros((K, T))
    Wc, Xc = _c(W, cdtype), _c(X, cdtype)
    for lag in range(min(L, T)):
        res[:, : T - lag] += (_lag(Wc, lag) @ Xc[:, lag:]).astype(np.float64, copy=False)
    return res


def select(mask, a):
    """select(mask, a, 0): what `a` holds under mask == 0 (NaN, Inf) never enters."""
    return np.where(mask != 0, a, 0.0)


class MaskedMult:
    """State of the rule: the mask, Xm and its norm."""

    def __init__(self, data, mask):
        mask = np.asarray(mask, dtype=np.float64)
        if not np.isin(mask, (0.0, 1.0)).all():
            raise ValueError("mask must hold 0 and 1 only")
        if not mask.any():
            raise ValueError("the mask observes nothing")
        self.mask = mask
        self.Xm = select(mask, np.asarray(data, dtype=np.float64))
        self.xm_norm = np.linalg.norm(self.Xm)


def masked_loss(rule, W, H, cdtype=np.float64):
    """norm(M .* (conv(W, H) - data)) / norm(Xm)."""
    est = select(rule.mask, tensor_conv(W, H, cdtype))
    return np.linalg.norm(est - rule.Xm) / rule.xm_norm


def update_motifs(rule, W, H, l1W=0.0, l2W=0.0, cdtype=np.float64):
    """mult.jl:23-39 under the mask.  W in place."""
    K, N, L = W.shape
    T = H.shape[1]
    est = select(rule.mask, tensor_conv(W, H, cdtype))  # :28
    numW, denomW = np.zeros(W.shape), np.zeros(W.shape)
    Hc, Xc, Ec = _c(H, cdtype), _c(rule.Xm, cdtype), _c(est, cdtype)
    for lag in range(L):  # :31-34
        if lag < T:
            numW[:, :, lag] = Hc[:, : T - lag] @ Xc[:, lag:].T
            denomW[:, :, lag] = Hc[:, : T - lag] @ Ec[:, lag:].T
    den = ((denomW + l1W) + (2.0 * l2W) * W) + EPS  # :37
    W *= numW / den
    np.maximum(W, EPS, out=W)  # :38
    return W


def update_feature_maps(rule, W, H, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """mult.jl:42-58 under the mask.  H in place; returns the loss."""
    est = select(rule.mask, tensor_conv(W, H, cdtype))  # :44
    numH = tensor_transconv(W, rule.Xm, cdtype)  # :47
    denomH = tensor_transconv(W, est, cdtype)  # :48
    den = ((denomH + l1H) + (2.0 * l2H) * H) + EPS  # :51
    H *= numH / den
    np.maximum(H, EPS, out=H)  # :52
    est = select(rule.mask, tensor_conv(W, H, cdtype))  # :55
    return np.linalg.norm(est - rule.Xm) / rule.xm_norm  # :56-57


def fit_masked(data, mask, W_init, H_init, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations."""
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    rule = MaskedMult(data, mask)
    loss_hist = [masked_loss(rule, W, H, cdtype)]
    for _ in range(int(max_itr)):
        update_motifs(rule, W, H, l1W=l1W, l2W=l2W, cdtype=cdtype)
        loss_hist.append(update_feature_maps(rule, W, H, l1H=l1H, l2H=l2H, cdtype=cdtype))
    return W, H, np.asarray(loss_hist)


def heldout_sums(data, mask, W, H, complement=False):
    """(sum of (conv(W, H) - data)^2, sum of data^2) over the entries with mask == 1, or with mask == 0 (complement): by select."""
    sel = (np.asarray(mask) == 0) if complement else (np.asarray(mask) != 0)
    est = tensor_conv(W, H)
    r = np.where(sel, est - np.where(sel, data, 0.0), 0.0)
    d = np.where(sel, data, 0.0)
    return float(np.sum(r * r)), float(np.sum(d * d))


def block_mask(N, T, frac, block, seed):
    """A plain 0/1 mask for fixtures: each (unit, slot of `block` samples) is held out with probability frac (independent of
    cmf.holdout_mask, so that fixtures do not move with it)."""
    rng = np.random.default_rng(seed)
    nslots = (T + block - 1) // block
    held = rng.random((N, nslots)) < frac
    return np.where(np.repeat(held, block, axis=1)[:, :T], 0.0, 1.0)
