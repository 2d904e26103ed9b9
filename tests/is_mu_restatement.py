"""The Itakura-Saito form of the MU rule, restated literally in fp64 numpy (the reference for tests/test_is_mu_cpu.py,
tests/test_gpu_is_mu.py and tests/golden/make_golden_is_mu.py).

It is the multiplicative update of the Itakura-Saito divergence (beta = 0; Fevotte & Idier 2011) written on src/algs/mult.jl:23-58:
with eps = eps(Float64) (src/CMF.jl:20), e = tensor_conv(W, H) + eps, Q = 1 ./ e and P = (data .* Q) .* Q,

    update_motifs!:        numW[:, :, l] = shift(H, l) P[:, 1+l:T]';  denomW[:, :, l] = shift(H, l) Q[:, 1+l:T]'
                           (mult.jl:32-33 with data -> P, est -> Q)
                           W .*= sqrt.(numW ./ (((denomW + l1W) + 2 l2W W) + eps));  W = max(eps, W)
    update_feature_maps!:  P, Q from the new W;  numH = transconv(W, P);  denomH = transconv(W, Q);  the same update of H
                           loss = D / (N T),  D = sum over entries of (r - 1) - log(r),  r = data ./ e   (e from the new H)

P is written as two multiplications by Q, never as data / (e * e): e * e underflows in the device's float32 where e is near eps.
The exponent 1/2 is the majorisation-minimisation step for beta < 1; with l1 = l2 = 0 the loss does not increase.  The loss is the
mean divergence per entry: dimensionless, unchanged when data and the estimate are scaled together, 0 for a perfect fit.

`cdtype`: the number format the CONTRACTIONS are carried out in.  `edtype`: the number format of the EPILOGUE that forms Q, P and the
loss terms from the conv (the device's is float32; the loss terms are then summed in fp64).  tools/mu_is_precision.py measures how far
float32 in both drifts from fp64.  Everything else stays fp64.
"""
import numpy as np

from kl_mu_restatement import hxt, tensor_conv, tensor_transconv  # noqa: F401  (the contractions, with their cdtype argument)

EPS = float(np.finfo(np.float64).eps)  # eps(): src/CMF.jl:20
MESSAGE = "Itakura-Saito divergence needs finite, strictly positive data"


def check_data(data):
    """What installing the divergence checks: finite and strictly positive (an exact zero has infinite divergence)."""
    data = np.asarray(data, dtype=np.float64)
    bad = int(np.sum(~(np.isfinite(data) & (data > 0))))
    if bad:
        raise ValueError(f"{MESSAGE} ({bad} entries are zero, negative, NaN or infinite): add a small floor to the spectrogram")
    return data


def pq(data, W, H, cdtype=np.float64, edtype=np.float64):
    """(P, Q): Q = 1 ./ e, P = (data .* Q) .* Q, e = tensor_conv(W, H) + eps."""
    e = tensor_conv(W, H, cdtype).astype(edtype) + edtype(EPS)
    Q = edtype(1.0) / e
    P = (data.astype(edtype) * Q) * Q
    return P.astype(np.float64), Q.astype(np.float64)


def is_loss(data, W, H, cdtype=np.float64, edtype=np.float64):
    """mean over entries of (r - 1) - log(r), r = data ./ (tensor_conv(W, H) + eps)."""
    e = tensor_conv(W, H, cdtype).astype(edtype) + edtype(EPS)
    r = data.astype(edtype) * (edtype(1.0) / e) if edtype is not np.float64 else data / e  # (the device multiplies by Q)
    terms = (r - edtype(1.0)) - np.log(r)
    return float(np.sum(terms.astype(np.float64))) / data.size


def _step(x, num, den):
    x *= np.sqrt(num / den)
    np.maximum(x, EPS, out=x)
    return x


def update_motifs(data, W, H, l1W=0.0, l2W=0.0, cdtype=np.float64, edtype=np.float64):
    """update_motifs! of the Itakura-Saito rule.  W in place."""
    L = W.shape[2]
    P, Q = pq(data, W, H, cdtype, edtype)
    numW = hxt(H, P, L, cdtype)  # mult.jl:32 with data -> P
    denomW = hxt(H, Q, L, cdtype)  # mult.jl:33 with est -> Q
    return _step(W, numW, ((denomW + l1W) + (2.0 * l2W) * W) + EPS)


def update_feature_maps(data, W, H, l1H=0.0, l2H=0.0, cdtype=np.float64, edtype=np.float64):
    """update_feature_maps! of the Itakura-Saito rule.  H in place; returns the loss."""
    P, Q = pq(data, W, H, cdtype, edtype)  # (e from the new W)
    numH = tensor_transconv(W, P, cdtype)
    denomH = tensor_transconv(W, Q, cdtype)
    _step(H, numH, ((denomH + l1H) + (2.0 * l2H) * H) + EPS)
    return is_loss(data, W, H, cdtype, edtype)  # (e from the new H)


def fit_is(data, W_init, H_init, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64, edtype=np.float64):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations."""
    data = check_data(data)
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [is_loss(data, W, H, cdtype, edtype)]
    for _ in range(int(max_itr)):
        update_motifs(data, W, H, l1W=l1W, l2W=l2W, cdtype=cdtype, edtype=edtype)
        loss_hist.append(update_feature_maps(data, W, H, l1H=l1H, l2H=l2H, cdtype=cdtype, edtype=edtype))
    return W, H, np.asarray(loss_hist)


def positive_problem(N, T, K, L, seed):
    """Inputs that store compactly: a power-spectrogram-like positive array -- a sparsified truth times a unit-mean exponential
    (the Itakura-Saito noise model), floored and held as uint8 values in 1 .. 255 (never 0) -- and float16 initial factors on a grid
    of 64, all exactly representable in the device's float32.  Returns (data uint8, W0 float16, H0 float16)."""
    rng = np.random.default_rng(seed)
    Wt = rng.random((K, N, L)) * (rng.random((K, N, L)) < 0.5)
    Ht = rng.random((K, T)) * (rng.random((K, T)) < 0.3)
    power = tensor_conv(Wt, Ht) * rng.exponential(1.0, (N, T))
    data = np.clip(np.rint(power * (40.0 / max(power.mean(), 1e-300))) + 1.0, 1, 255).astype(np.uint8)
    W0 = (rng.integers(0, 64, (K, N, L)) / 64.0 + 0.125).astype(np.float16)
    H0 = (rng.integers(0, 64, (K, T)) / 64.0 + 0.125).astype(np.float16)
    return data, W0, H0


def load_fixture(path):
    """A tests/golden/mu_is_*.npz file as float64 arrays: data, W0, H0, W, H, loss_hist, max_itr and the regularisers.  A fixture
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
        W, H, lh = fit_is(out["data"], out["W0"], out["H0"], max_itr=out["max_itr"], **out["reg"])
        np.testing.assert_allclose(lh, out["loss_hist"], rtol=1e-10)
        np.testing.assert_allclose([np.linalg.norm(W), np.linalg.norm(H)], [float(g["W_norm"]), float(g["H_norm"])], rtol=1e-10)
        out["W"], out["H"] = W, H
    return out
