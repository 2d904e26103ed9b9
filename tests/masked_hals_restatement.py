"""TEST INFRASTRUCTURE: fp64 restatement of the HALS rule under a 0/1 mask by imputation (library option "hals_mask").

Before each half-update the held-out entries of the data are replaced by the current estimate,

    X~ = where(M, X, tensor_conv(W, H)),

and the oracle's ordinary HALS half-update (oracle/cmf_oracle.py: hals_update_motifs, hals_update_feature_maps) runs on X~.  The rule
only ever reads the residual, and est - X~ = M .* (est - X): the imputation is "the residual is 0 where nothing is observed".  Every
step of a half-update exactly minimises a block of norm(X~ - conv(W, H))^2, which majorises norm(M .* (X - conv(W, H)))^2 with equality
at the current point, so without regularisers the masked loss cannot go up.

Two ways to hold the residual, the same in exact arithmetic:

  carried   (rule given) the oracle's HALSUpdate carries its residual from half-update to half-update (hals.jl:6-28); the imputation sets
            its held-out entries to 0 in front of each.  With an all-ones mask nothing is set: the oracle's fit bit for bit.
  fresh     (rule None) the residual is formed from W, H and X~ in front of each half-update -- what the device does.

use_c: the half-updates through the oracle's C restatement (c_fit_hals: one iteration on X~ for the W half, one in eval mode for the H
half) instead of its numpy loops -- the same numbers to rounding, in a fraction of the time on long recordings (fresh form only).

The loss is norm(M .* (est - X)) / norm(M .* X), the masked MU rule's (tests/masked_mu_restatement.py).  Values of X at held-out
entries are never read into a result: np.where selects around them."""
import numpy as np


def observed(mask):
    return np.asarray(mask) != 0


def impute(o, data, mask, W, H):
    """X~ = where(M, X, tensor_conv(W, H))"""
    return np.where(observed(mask), data, o.tensor_conv(W, H))


def masked_resid(o, data, mask, W, H):
    """M .* (tensor_conv(W, H) - X) = tensor_conv(W, H) - X~, without reading X where it is held out into the result"""
    with np.errstate(invalid="ignore"):
        return np.where(observed(mask), o.tensor_conv(W, H) - data, 0.0)


def masked_loss(o, data, mask, W, H, resid=None):
    r = masked_resid(o, data, mask, W, H) if resid is None else np.where(observed(mask), resid, 0.0)
    return float(np.linalg.norm(r) / np.linalg.norm(np.where(observed(mask), data, 0.0)))


class MaskedHALS:
    """The oracle's HALSUpdate on X~: the carried residual, and the norm the loss is divided by."""

    def __init__(self, o, data, mask, W, H):
        self.resids = masked_resid(o, data, mask, W, H)
        self.data_norm = float(np.linalg.norm(np.where(observed(mask), data, 0.0)))


def _rule_for(o, rule, data, mask, W, H):
    if rule is None:
        return MaskedHALS(o, data, mask, W, H)
    rule.resids[~observed(mask)] = 0.0  # the imputation: est - X~ is 0 where nothing is observed
    return rule


def masked_hals_half_W(o, data, mask, W, H, l1W=0.0, l2W=0.0, rule=None, use_c=False):
    """update_motifs! on X~.  W in place; returns W."""
    if use_c:
        assert rule is None
        Wn, _, _, _ = o.c_fit_hals(impute(o, data, mask, W, H), W, H, max_itr=1, check_convergence=False, l1W=l1W, l2W=l2W)
        W[...] = Wn  # (the H half that c_fit_hals runs behind it does not touch W)
        return W
    r = _rule_for(o, rule, data, mask, W, H)
    return o.hals_update_motifs(r, None, W, H, l1W=l1W, l2W=l2W)


def masked_hals_half_H(o, data, mask, W, H, l1H=0.0, l2H=0.0, rule=None, use_c=False):
    """update_feature_maps! on X~.  H in place; returns norm(M .* (est - X)) / norm(M .* X) for the updated H."""
    if use_c:
        assert rule is None
        _, Hn, _, _ = o.c_fit_hals(impute(o, data, mask, W, H), W, H, max_itr=1, check_convergence=False, eval_mode=True, l1H=l1H, l2H=l2H)
        H[...] = Hn
        return masked_loss(o, data, mask, W, H)
    r = _rule_for(o, rule, data, mask, W, H)
    o.hals_update_feature_maps(r, None, W, H, l1H=l1H, l2H=l2H)
    # (the residual the sweep leaves is est - X~ for the X~ of BEFORE the sweep: its observed entries are those of est - X)
    return float(np.linalg.norm(np.where(observed(mask), r.resids, 0.0)) / r.data_norm)


def masked_hals_fit(o, data, mask, W_init, H_init, max_itr=10, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, carried=True, use_c=False):
    """fit(::AlternatingOptimizer{HALSUpdate}) (oracle.fit_hals without the convergence test) under the mask.
    Returns W, H, loss_hist (max_itr + 1 entries: norm(M .* (est - X)) / norm(M .* X) per iteration, the initial one first)."""
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    rule = MaskedHALS(o, data, mask, W, H) if carried and not use_c else None
    loss_hist = [masked_loss(o, data, mask, W, H)]
    for _ in range(max_itr):
        masked_hals_half_W(o, data, mask, W, H, l1W=l1W, l2W=l2W, rule=rule, use_c=use_c)
        loss_hist.append(masked_hals_half_H(o, data, mask, W, H, l1H=l1H, l2H=l2H, rule=rule, use_c=use_c))
    return W, H, np.asarray(loss_hist)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def block_mask(N, T, frac, block, seed):
    """1 = observed.  Runs of `block` held-out entries along time, started with the probability that holds out about `frac` of the entries."""
    rng = np.random.default_rng(seed)
    starts = rng.random((N, T)) < frac / block
    held = np.zeros((N, T), bool)
    for e in range(block):
        held[:, e:] |= starts[:, :T - e]
    return np.asfortranarray(np.where(held, 0.0, 1.0))


def masks(N, T, L, seed=11):
    """The masks of the tests, by name: 30 % speckle, 20 % in blocks of L, one unit entirely held out, one column entirely held out."""
    unit, col = np.ones((N, T)), np.ones((N, T))
    unit[N // 3, :] = 0.0
    col[:, T // 2] = 0.0
    return {"speckle30": block_mask(N, T, 0.3, 1, seed), "blocks20": block_mask(N, T, 0.2, L, seed + 1),
            "unit": np.asfortranarray(unit), "column": np.asfortranarray(col)}


def garbage(data, mask):
    """data with NaN, +Inf, -Inf and 1e30 in turn at the held-out entries"""
    out = np.array(data, dtype=np.float64, order="K", copy=True)  # (the layout of data: numpy's sums follow it)
    held = np.nonzero(~observed(mask))
    out[held] = np.array([np.nan, np.inf, -np.inf, 1e30])[np.arange(held[0].size) % 4]
    return out


# ---- the model of the device's arithmetic (tools/hals_masked_precision.py) -------------------------------------------------------------
def f32_iteration(o, gf, data, mask, W, H, l1W, l2W, l1H, l2H, dtype):
    """One iteration with the contractions (conv, residual, G, P) and the sweeps' state in `dtype` -- float32: the model of the kernels;
    float64: the fresh form above in the Gram-projected sweeps of tests/hals_gram_form.py (gf).  Returns W, H, loss."""
    obs = observed(mask)
    Xm = np.where(obs, data, 0.0)

    def resid(Wc, Hc):
        return np.where(obs, gf.conv_in(Wc, Hc, dtype) - Xm.astype(dtype), dtype(0))

    def proj_w(stage, a):
        if stage == "projections":
            R = resid(a["W"], a["H"])
            a["G"] = (R @ a["Hu"].astype(dtype).T).astype(np.float64)

    def proj_h(stage, a):
        if stage == "projections":
            R = resid(a["W"], a["H"])
            K, N, L = a["W"].shape
            T = R.shape[1]
            P = np.zeros((K, T), dtype)
            Wd = a["W"].astype(dtype)
            for lag in range(min(L, T)):
                P[:, :T - lag] += Wd[:, :, lag] @ R[:, lag:]
            a["P"] = P.astype(np.float64)

    # (w_half / h_half form R from the data they are given: X~ makes it the masked residual in fp64; the hooks replace the projections
    # by the ones contracted in dtype)
    Wn = gf.w_half(o, W, H, impute(o, data, mask, W, H), l1W, l2W, dtype=dtype, corrupt=proj_w)["new"]
    a = gf.h_half(o, Wn, H, impute(o, data, mask, Wn, H), l1H, l2H, dtype=dtype, corrupt=proj_h)
    Hn = a["new"]
    r = resid(Wn, Hn)
    loss = float(np.sqrt(float(np.sum(r.astype(np.float64) ** 2))) / np.linalg.norm(Xm))
    return Wn, Hn, loss
