"""The KL form of the MU rule, restated literally in fp64 numpy (the reference for tests/test_kl_mu_cpu.py,
tests/test_gpu_kl_mu.py and tests/golden/make_golden_kl_mu.py).

It is the multiplicative update of the generalised Kullback-Leibler divergence (Smaragdis' convolutive NMF) written on
src/algs/mult.jl:23-58: with eps = eps(Float64) (src/CMF.jl:20) and e = tensor_conv(W, H) + eps,

    update_motifs!:        R = data ./ e;  numW[:, :, l] = shift(H, l) R[:, 1+l:T]'      (mult.jl:32 with data -> R)
                           denomW[k, n, l] = sum(H[k, 1:T-l])                             (the same for every n; 0 when l >= T)
                           W .*= numW ./ (((denomW + l1W) + 2 l2W W) + eps);  W = max(eps, W)             (mult.jl:37-38 unchanged)
    update_feature_maps!:  R = data ./ e (e from the new W);  numH = transconv(W, R)
                           denomH[k, t] = sum over l < min(L, T-t+1), over n, of W[k, n, l+1];  the same update of H
                           loss = D(data, e) / sum(data)   (e from the new H)
    D(X, e) = sum over entries of (X > 0 ? X log(X / e) : 0) - X + e                      (a select: 0 log 0 = 0)

denomW and denomH are what mult.jl:33 and :48 give with est replaced by all ones (ones_denominators below computes them that
way, through the contractions; tests/test_kl_mu_cpu.py holds the two forms together).  Where the rule coincides with
oracle/cmf_oracle.py's MU rule -- the contractions, the element-wise update, the order of the additions in the denominator -- the
operations follow it in the same order.

`cdtype`: the number format the CONTRACTIONS (conv, transconv, the numW products) are carried out in; float32 models the device's
arithmetic (tools/mu_kl_precision.py measures how far that drifts from fp64).  `edtype` (ratio, divergence and kl_loss only): the number
format of the EPILOGUE that forms R and the loss terms from the conv, as in tests/is_mu_restatement.py (the terms are then summed in
fp64; tools/mu_divergence_elementwise.py).  Everything else stays fp64.

LITERAL_SLICES: as in tests/masked_mu_restatement.py -- True multiplies the strided slices W[:, :, lag] as they are (the oracle's
operation order, a plain loop), False (default) copies each slice first so that the products run in BLAS.
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


def hxt(H, X, L, cdtype=np.float64):
    """out[:, :, l] = shift_cols(H, l) * X[:, 1+l:T]' (mult.jl:32-33): K x N x L, lags l >= T stay 0."""
    K, T = H.shape
    out = np.zeros((K, X.shape[0], L))
    Hc, Xc = _c(H, cdtype), _c(X, cdtype)
    for lag in range(L):
        if lag < T:
            out[:, :, lag] = Hc[:, : T - lag] @ Xc[:, lag:].T
    return out


def check_data(data):
    """What installing the divergence checks: finite, non-negative, positive sum."""
    data = np.asarray(data, dtype=np.float64)
    if not np.isfinite(data).all():
        raise ValueError("the KL divergence needs finite data")
    if (data < 0).any():
        raise ValueError("the KL divergence needs non-negative data")
    if not data.sum() > 0:
        raise ValueError("the KL divergence needs data with a positive sum")
    return data


def ratio(data, W, H, cdtype=np.float64, edtype=np.float64):
    """R = data ./ (tensor_conv(W, H) + eps)."""
    if edtype is np.float64:
        return data / (tensor_conv(W, H, cdtype) + EPS)
    return (data.astype(edtype) / (tensor_conv(W, H, cdtype).astype(edtype) + edtype(EPS))).astype(np.float64)


def divergence(data, est_eps, edtype=np.float64):
    """D(X, e) = sum of (X > 0 ? X log(X / e) : 0) - X + e (edtype: the terms' format; they are summed in fp64)."""
    pos = data > 0
    if edtype is not np.float64:  # the device's order: x log(q) + (e - x)
        x, e = data.astype(edtype), est_eps.astype(edtype)
        q = np.where(pos, x, edtype(1.0)) / np.where(pos, e, edtype(1.0))
        return float(np.sum((np.where(pos, x * np.log(q), edtype(0.0)) + (e - x)).astype(np.float64)))
    q = np.where(pos, data, 1.0) / np.where(pos, est_eps, 1.0)
    return float(np.sum(np.where(pos, data * np.log(q), 0.0) - data + est_eps))


def kl_loss(data, W, H, cdtype=np.float64, edtype=np.float64):
    """D(data, tensor_conv(W, H) + eps) / sum(data): dimensionless, 0 for a perfect fit."""
    return divergence(data, tensor_conv(W, H, cdtype) + EPS, edtype) / float(np.sum(data))


def denom_W(H, N, L):
    """denomW[k, n, l] = sum(H[k, 1:T-l]), the same for every n; 0 when l >= T."""
    K, T = H.shape
    den = np.zeros((K, N, L))
    for lag in range(L):
        if lag < T:
            den[:, :, lag] = np.sum(H[:, : T - lag], axis=1)[:, None]
    return den


def denom_H(W, T):
    """denomH[k, t] = sum over l < min(L, T-t+1) (t from 1), over n, of W[k, n, l+1]."""
    K, N, L = W.shape
    cum = np.cumsum(np.sum(W, axis=1), axis=1)  # cum[k, j] = sum over l <= j, over n
    nl = np.minimum(L, T - np.arange(T))  # lags that fit behind column t (t from 0)
    return cum[:, nl - 1]


def ones_denominators(W, H, N):
    """(denomW, denomH) as mult.jl:33 and :48 give them with est replaced by all ones, through the contractions above."""
    K, T = H.shape
    ones = np.ones((N, T))
    return hxt(H, ones, W.shape[2]), tensor_transconv(W, ones)


def update_motifs(data, W, H, l1W=0.0, l2W=0.0, cdtype=np.float64):
    """update_motifs! of the KL rule.  W in place."""
    K, N, L = W.shape
    R = ratio(data, W, H, cdtype)
    numW = hxt(H, R, L, cdtype)  # mult.jl:32 with data -> R
    denomW = denom_W(H, N, L)
    den = ((denomW + l1W) + (2.0 * l2W) * W) + EPS  # :37
    W *= numW / den
    np.maximum(W, EPS, out=W)  # :38
    return W


def update_feature_maps(data, W, H, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """update_feature_maps! of the KL rule.  H in place; returns the loss."""
    R = ratio(data, W, H, cdtype)  # (e from the new W)
    numH = tensor_transconv(W, R, cdtype)  # :47 with data -> R
    denomH = denom_H(W, H.shape[1])
    den = ((denomH + l1H) + (2.0 * l2H) * H) + EPS  # :51
    H *= numH / den
    np.maximum(H, EPS, out=H)  # :52
    return kl_loss(data, W, H, cdtype)  # (e from the new H)


def fit_kl(data, W_init, H_init, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations."""
    data = check_data(data)
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [kl_loss(data, W, H, cdtype)]
    for _ in range(int(max_itr)):
        update_motifs(data, W, H, l1W=l1W, l2W=l2W, cdtype=cdtype)
        loss_hist.append(update_feature_maps(data, W, H, l1H=l1H, l2H=l2H, cdtype=cdtype))
    return W, H, np.asarray(loss_hist)


def synthetic(N, T, K, L, seed, zero_frac=0.3, zero_unit=True):
    """Inputs for tests and fixtures: uniform random factors, a sparsified truth, data with up to `zero_frac` exact zeros and (when
    N > 1) one all-zero unit.  Returns (data, W_init, H_init)."""
    rng = np.random.default_rng(seed)
    Wt = rng.random((K, N, L)) * (rng.random((K, N, L)) < 0.5)
    Ht = rng.random((K, T)) * (rng.random((K, T)) < 0.3)
    data = tensor_conv(Wt, Ht) * (0.5 + rng.random((N, T)))
    data[rng.random((N, T)) < zero_frac] = 0.0
    if zero_unit and N > 1:
        data[N // 2, :] = 0.0
    if not data.sum() > 0:
        data[0, 0] = 1.0
    W0 = rng.random((K, N, L)) + 0.1
    H0 = rng.random((K, T)) + 0.1
    return data, W0, H0


def count_problem(N, T, K, L, seed):
    """Inputs that store compactly (fixtures of the larger shapes): data are COUNTS -- Poisson draws around a sparsified truth, with
    exact zeros and one all-zero unit, held as uint8 -- and the initial factors are float16 values on a grid of 64, all exactly representable in
    the device's float32.  Returns (data uint8, W0 float16, H0 float16)."""
    rng = np.random.default_rng(seed)
    Wt = rng.random((K, N, L)) * (rng.random((K, N, L)) < 0.5)
    Ht = rng.random((K, T)) * (rng.random((K, T)) < 0.3)
    rate = tensor_conv(Wt, Ht)
    data = np.minimum(rng.poisson(rate * (6.0 / max(rate.mean(), 1e-300))), 255).astype(np.uint8)
    data[rng.random((N, T)) < 0.1] = 0
    if N > 1:
        data[N // 2, :] = 0
    if not data.any():
        data[0, 0] = 1
    W0 = (rng.integers(0, 64, (K, N, L)) / 64.0 + 0.125).astype(np.float16)  # (a grid of 64 values: compresses, exact in float16)
    H0 = (rng.integers(0, 64, (K, T)) / 64.0 + 0.125).astype(np.float16)
    return data, W0, H0


def load_fixture(path):
    """A tests/golden/mu_kl_*.npz file as float64 arrays: data, W0, H0, W, H, loss_hist, max_itr and the regularisers.  A fixture
    whose W and H would not fit the size agreed for golden files holds their float32 roundings (W32 / H32: 6e-8 relative) or, where
    even those do not fit, their Frobenius norms only: W and H are then recomputed here from the stored inputs, and must reproduce
    the stored loss_hist and norms."""
    g = np.load(path)
    out = {k: np.asarray(g[k], dtype=np.float64) for k in ("data", "W0", "H0", "loss_hist")}
    out["max_itr"] = int(g["max_itr"])
    out["reg"] = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")}
    out["exact"] = "W" in g.files
    if "W" in g.files or "W32" in g.files:
        out["W"] = np.asarray(g["W"] if "W" in g.files else g["W32"], dtype=np.float64)
        out["H"] = np.asarray(g["H"] if "H" in g.files else g["H32"], dtype=np.float64)
    else:
        W, H, lh = fit_kl(out["data"], out["W0"], out["H0"], max_itr=out["max_itr"], **out["reg"])
        np.testing.assert_allclose(lh, out["loss_hist"], rtol=1e-10)
        np.testing.assert_allclose([np.linalg.norm(W), np.linalg.norm(H)], [float(g["W_norm"]), float(g["H_norm"])], rtol=1e-10)
        out["W"], out["H"] = W, H
    return out
