"""The beta-divergence form of the MU rule, restated literally in numpy (the reference for tests/test_beta_mu_cpu.py,
tests/test_gpu_beta_mu.py, tools/mu_beta_precision.py and tests/golden/make_golden_beta_mu.py).

It is the multiplicative update of the beta-divergence (Fevotte & Idier 2011) written on src/algs/mult.jl:23-58: with
eps = eps(Float64) (src/CMF.jl:20), e = tensor_conv(W, H) + eps, Q = e.^(beta - 1) and P = data .* e.^(beta - 2),

    update_motifs!:        numW[:, :, l] = shift(H, l) P[:, 1+l:T]';  denomW[:, :, l] = shift(H, l) Q[:, 1+l:T]'
                           (mult.jl:32-33 with data -> P, est -> Q)
                           W .*= (numW ./ (((denomW + l1W) + 2 l2W W) + eps)).^gamma;  W = max(eps, W)
    update_feature_maps!:  P, Q from the new W;  numH = transconv(W, P);  denomH = transconv(W, Q);  the same update of H
                           loss = D_beta / (N T),  D_beta = sum over entries of d_beta(data | e)   (e from the new H)
    d_beta(x | y) = (x^beta + (beta - 1) y^beta - beta x y^(beta - 1)) / (beta (beta - 1))
    gamma = 1 / (2 - beta) for beta < 1,  1 for 1 <= beta <= 2,  1 / (beta - 1) for beta > 2

gamma is the majorisation-minimisation exponent: with l1 = l2 = 0 the loss does not increase.  beta = 2 is the squared error
(P = data, Q = e, D = sum (data - e)^2 / 2), beta -> 1 the generalised KL divergence, beta -> 0 Itakura-Saito.

The powers are formed as the device forms them: lg = log2(e) once, then exp2(b lg) for each exponent b.  The loss term is NOT the
three-term formula above, which cancels once a fit is nearly exact (float32: 9e-2 off at beta = 0.9 on the shape of the *_short
fixtures), but d = y^beta phi(r), r = x / y, delta = r - 1 (`terms` below; `terms_direct` is the formula, kept for the tests):

    |delta| < 1/8:  phi = delta^2 / 2 (1 + c1 delta + ... + c6 delta^6),  c_k = 2 (beta - 2) (beta - 3) ... (beta - k - 1) / (k + 2)!
    otherwise:      phi = ((r^beta - 1) - beta delta) / (beta (beta - 1))
    x = 0:          phi = 1 / beta

(the series is the binomial expansion of the second line; cut after delta^6 it is off by at most 1e-7 of the term at |delta| = 1/8).

`cdtype`: the number format the CONTRACTIONS are carried out in.  `edtype`: the number format of the EPILOGUE that forms Q, P and the
loss terms from the conv (the device's is float32; the loss terms are then summed in fp64).  tools/mu_beta_precision.py measures how
far float32 in both drifts from fp64.  Everything else stays fp64.
"""
import math

import numpy as np

from kl_mu_restatement import count_problem, hxt, tensor_conv, tensor_transconv  # noqa: F401  (the contractions, with their cdtype argument)

EPS = float(np.finfo(np.float64).eps)  # eps(): src/CMF.jl:20
BETA_MAX = 4.0
WINDOW = 0.01  # CMF_BETA_WINDOW (include/cmf_hip.h), the `window` line of profiles/mu_beta_precision.txt
SERIES_DELTA = 0.125
SERIES_TERMS = 6
MESSAGE = "the beta-divergence needs finite, non-negative data"


def check_beta(beta, window=None):
    """The accepted set: 0 < beta <= 4 outside a window around 0+ and around 1 (the window's edges are accepted).  Returns beta."""
    window = WINDOW if window is None else window
    b = float(beta)
    if not math.isfinite(b):
        raise ValueError(f"beta must be finite, got {beta!r}")
    if b == 0.0 or b == 1.0:
        raise ValueError(f"beta = {b:g} is CMF_DIV_IS (beta = 0) or CMF_DIV_KL (beta = 1): the beta formula is 0/0 there, use those forms")
    if b < 0.0 or b > BETA_MAX:
        raise ValueError(f"beta must lie in (0, {BETA_MAX:g}], got {b!r}")
    if b < window * (1 - 1e-9) or abs(b - 1.0) < window * (1 - 1e-9):
        raise ValueError(f"beta = {b!r} lies within {window:g} of 0 or 1, where the float32 loss loses its digits to the factor "
                         f"1 / (beta (beta - 1)): use CMF_DIV_IS / CMF_DIV_KL, or a beta at least {window:g} away")
    return b


def gamma(beta):
    """The majorisation-minimisation exponent of the step."""
    return 1.0 / (2.0 - beta) if beta < 1.0 else 1.0 if beta <= 2.0 else 1.0 / (beta - 1.0)


def series_coefficients(beta):
    """c_1 .. c_6 of phi = delta^2 / 2 (1 + sum c_k delta^k)."""
    out, prod = [], 1.0
    for k in range(1, SERIES_TERMS + 1):
        prod *= beta - (k + 1)
        out.append(2.0 * prod / math.factorial(k + 2))
    return out


def check_data(data):
    """What installing the divergence checks: finite and non-negative (an exact zero is legal for beta > 0)."""
    data = np.asarray(data, dtype=np.float64)
    bad = int(np.sum(~(np.isfinite(data) & (data >= 0))))
    if bad:
        raise ValueError(f"{MESSAGE} ({bad} entries are negative, NaN or infinite)")
    return data


def _e(data, W, H, cdtype, edtype):
    return tensor_conv(W, H, cdtype).astype(edtype) + edtype(EPS)


def pq(data, W, H, beta, cdtype=np.float64, edtype=np.float64):
    """(P, Q): lg = log2(e), Q = exp2((beta - 1) lg), P = data .* exp2((beta - 2) lg), e = tensor_conv(W, H) + eps."""
    lg = np.log2(_e(data, W, H, cdtype, edtype))
    Q = np.exp2(edtype(beta - 1.0) * lg)
    x = data.astype(edtype)
    P = np.where(x > 0, x * np.exp2(edtype(beta - 2.0) * lg), edtype(0.0))  # (a select, as on the device)
    return P.astype(np.float64), Q.astype(np.float64)


def terms(x, e, beta, edtype=np.float64):
    """d_beta(x | e) per entry as y^beta phi(x / y), in edtype (the device's composition: the module docstring)."""
    x, e = x.astype(edtype), e.astype(edtype)
    yb = np.exp2(edtype(beta) * np.log2(e))
    r = x / e
    delta = r - edtype(1.0)
    poly = np.zeros_like(delta)
    for c in reversed(series_coefficients(beta)):
        poly = (poly + edtype(c)) * delta
    near = (edtype(0.5) * delta * delta) * (edtype(1.0) + poly)
    rb = np.exp2(edtype(beta) * np.log2(np.where(r > 0, r, edtype(1.0))))
    far = ((rb - edtype(1.0)) - edtype(beta) * delta) * edtype(1.0 / (beta * (beta - 1.0)))
    phi = np.where(x > 0, np.where(np.abs(delta) < edtype(SERIES_DELTA), near, far), edtype(1.0 / beta))
    return yb * phi


def terms_direct(x, e, beta):
    """d_beta(x | e) per entry by the three-term formula (fp64; what `terms` is held against)."""
    return (x ** beta + (beta - 1.0) * e ** beta - beta * x * e ** (beta - 1.0)) / (beta * (beta - 1.0))


def beta_loss(data, W, H, beta, cdtype=np.float64, edtype=np.float64, direct=False):
    """mean over entries of d_beta(data | tensor_conv(W, H) + eps)."""
    e = _e(data, W, H, cdtype, edtype)
    t = terms_direct(data, e.astype(np.float64), beta) if direct else terms(data, e, beta, edtype)
    return float(np.sum(t.astype(np.float64))) / data.size


def _step(x, num, den, g):
    q = num / den
    x *= q if g == 1.0 else q ** g
    np.maximum(x, EPS, out=x)
    return x


def update_motifs(data, W, H, beta, l1W=0.0, l2W=0.0, cdtype=np.float64, edtype=np.float64):
    """update_motifs! of the beta rule.  W in place."""
    L = W.shape[2]
    P, Q = pq(data, W, H, beta, cdtype, edtype)
    numW = hxt(H, P, L, cdtype)  # mult.jl:32 with data -> P
    denomW = hxt(H, Q, L, cdtype)  # mult.jl:33 with est -> Q
    return _step(W, numW, ((denomW + l1W) + (2.0 * l2W) * W) + EPS, gamma(beta))


def update_feature_maps(data, W, H, beta, l1H=0.0, l2H=0.0, cdtype=np.float64, edtype=np.float64):
    """update_feature_maps! of the beta rule.  H in place; returns the loss."""
    P, Q = pq(data, W, H, beta, cdtype, edtype)  # (e from the new W)
    numH = tensor_transconv(W, P, cdtype)
    denomH = tensor_transconv(W, Q, cdtype)
    _step(H, numH, ((denomH + l1H) + (2.0 * l2H) * H) + EPS, gamma(beta))
    return beta_loss(data, W, H, beta, cdtype, edtype)  # (e from the new H)


def fit_beta(data, W_init, H_init, beta, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64, edtype=np.float64,
             window=None):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations."""
    beta = check_beta(beta, window)
    data = check_data(data)
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [beta_loss(data, W, H, beta, cdtype, edtype)]
    for _ in range(int(max_itr)):
        update_motifs(data, W, H, beta, l1W=l1W, l2W=l2W, cdtype=cdtype, edtype=edtype)
        loss_hist.append(update_feature_maps(data, W, H, beta, l1H=l1H, l2H=l2H, cdtype=cdtype, edtype=edtype))
    return W, H, np.asarray(loss_hist)


def load_fixture(path):
    """A tests/golden/mu_beta_*.npz file as float64 arrays: data, W0, H0, W, H, loss_hist, beta, max_itr and the regularisers.  A
    fixture whose W and H would not fit the size agreed for golden files holds their float32 roundings (W32 / H32: 6e-8 relative) or,
    where even those do not fit, their Frobenius norms only: W and H are then recomputed here from the stored inputs, and must
    reproduce the stored loss_hist and norms."""
    g = np.load(path)
    out = {k: np.asarray(g[k], dtype=np.float64) for k in ("data", "W0", "H0", "loss_hist")}
    out["max_itr"] = int(g["max_itr"])
    out["beta"] = float(g["beta"])
    out["reg"] = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")}
    out["exact"] = "W" in g.files
    if "W" in g.files or "W32" in g.files:
        out["W"] = np.asarray(g["W"] if "W" in g.files else g["W32"], dtype=np.float64)
        out["H"] = np.asarray(g["H"] if "H" in g.files else g["H32"], dtype=np.float64)
    else:
        W, H, lh = fit_beta(out["data"], out["W0"], out["H0"], out["beta"], max_itr=out["max_itr"], **out["reg"])
        np.testing.assert_allclose(lh, out["loss_hist"], rtol=1e-10)
        np.testing.assert_allclose([np.linalg.norm(W), np.linalg.norm(H)], [float(g["W_norm"]), float(g["H_norm"])], rtol=1e-10)
        out["W"], out["H"] = W, H
    return out
