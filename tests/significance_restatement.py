"""seqNMF's significance test of components on held-out data (test_significance.m), restated in fp64 numpy.

The definition (include/cmf_hip.h: cmf_null_shifts, cmf_null_moments):

  shifts     draw 0 is the identity; for d >= 1
                 s(d, k, n) = ((bits(base(seed, 0x5157), ((d - 1) K + k) N + n) >> 32) * L) >> 32      (64-bit integers)
             with base / bits of csrc/cmf_rng.h (restated below: mix, base, bits)
  null motif Wnull_d[k, n, l] = W[k, n, (l - s(d, k, n)) mod L]                                           (circshift(W(n, k, :), s))
  overlap    v_d = tensor_transconv(Wnull_d, X)   (common.jl:71-81: v[k, t] = sum_{n, l, t + l < T'} Wnull[k, n, l] X[n, t + l])
  moments    S1 = sum_t v, S2 = sum_t v^2, S3 = sum_t v^3 per (draw, component)
  host       mu = S1 / T', m2 = S2 / T' - mu^2, m3 = S3 / T' - 3 mu S2 / T' + 2 mu^3, skew = m3 / m2^1.5   (MATLAB's skewness(., 1, 2))
             excluded (pval = inf): every entry of W[k] <= eps(Float64); max_n Wflat[k, n]^2 > 0.999 sum_n Wflat[k, n]^2; m2 of the
             component's own overlap <= 0
             pval[k] = (1 + #{d >= 1: skewnull[k, d] > skew[k]}) / nnull;  significant where pval <= p / K_kept

`contraction` selects the arithmetic of the overlap: float64 (the definition) or float32 (the model of the device: an fp32 contraction,
widened to fp64 before it is squared and cubed).  `mutation` breaks the definition in one of five ways a kernel could (MUTATIONS); the
CPU tests show that each moves a power sum on the exact problems, so that the bit-for-bit GPU test would see it.
"""
import math

import numpy as np

EPS = 2.220446049250313e-16
STREAM = 0x5157
U = np.uint64

MUTATIONS = ("reversed", "per_component", "zero_fill", "last_block_lost", "seam_next_draw")


def mix(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def base(seed, stream):
    with np.errstate(over="ignore"):
        return mix(np.asarray(seed & (2**64 - 1), dtype=U) + U(0x632BE59BD9B4E019) * U(stream + 1))


def bits(b, i):
    with np.errstate(over="ignore"):
        return mix(b + (np.asarray(i, dtype=U) + U(1)) * U(0x9E3779B97F4A7C15))


def null_shifts(seed, draws, K, N, L):
    """(N, K, len(draws)) int64: s(d, k, n)."""
    draws = np.asarray(draws, dtype=np.int64)
    b = base(seed, STREAM)
    out = np.zeros((N, K, len(draws)), dtype=np.int64)
    n = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    for j, d in enumerate(draws):
        if d == 0:
            continue
        ctr = ((int(d) - 1) * K + k) * N + n
        with np.errstate(over="ignore"):
            out[:, :, j] = (((bits(b, ctr.astype(U)) >> U(32)) * U(L)) >> U(32)).astype(np.int64)
    return out


def hashed_ints(seed, stream, shape, m):
    """Integers in {0 .. m-1} as float64, a pure function of (seed, stream, position)."""
    n = int(np.prod(shape))
    return ((bits(base(seed, stream), np.arange(n, dtype=U)) >> U(33)) % U(m)).astype(np.float64).reshape(shape)


def null_motif(W, s, mutation=None):
    """Wnull[k, n, l] = W[k, n, (l - s[n, k]) mod L] for the (N, K) shift table s of one draw."""
    K, N, L = W.shape
    s = np.asarray(s, dtype=np.int64).T  # (K, N)
    if mutation == "per_component":
        s = np.repeat(s[:, :1], N, axis=1)
    l = np.arange(L, dtype=np.int64)[None, None, :]
    src = l + s[:, :, None] if mutation == "reversed" else l - s[:, :, None]
    out = np.take_along_axis(W, np.mod(src, L), axis=2)
    if mutation == "zero_fill":
        out = np.where(src >= 0, out, 0.0)
    return out


def transconv(W, X, dtype=np.float64):
    """v[k, t] = sum_{n, l, t + l < T} W[k, n, l] X[n, t + l] (common.jl:71-81), accumulated in `dtype`."""
    K, N, L = W.shape
    T = X.shape[1]
    Wc, Xc = W.astype(dtype), X.astype(dtype)
    v = np.zeros((K, T), dtype=dtype)
    for l in range(min(L, T)):
        v[:, : T - l] += Wc[:, :, l] @ Xc[:, l:]
    return v


def power_sums(v):
    v = v.astype(np.float64)
    v2 = v * v
    return np.stack([v.sum(axis=1), v2.sum(axis=1), (v2 * v).sum(axis=1)])  # (3, K)


def null_moments(W, X, seed, draws, contraction=np.float64, mutation=None):
    """(3, K, len(draws)): the raw power sums of every draw."""
    K, N, L = W.shape
    T = X.shape[1]
    draws = list(draws)
    out = np.zeros((3, K, len(draws)))
    for j, d in enumerate(draws):
        Wd = null_motif(W, null_shifts(seed, [d], K, N, L)[:, :, 0], mutation)
        if mutation == "seam_next_draw":
            # packed columns c = d K + k in blocks of 32: the columns of a draw that lie in a block starting at or behind the draw's first
            # column (c >= 32) are read from the next draw
            Wn = null_motif(W, null_shifts(seed, [d + 1], K, N, L)[:, :, 0])
            for k in range(K):
                c = d * K + k
                if c >= 32 and c % 32 <= k:
                    Wd[k] = Wn[k]
        v = transconv(Wd, X, contraction)
        if mutation == "last_block_lost":
            v = v[:, : 128 * ((T + 127) // 128 - 1)]
        out[:, :, j] = power_sums(v)
    return out


def skew_from_sums(sums, T):
    """The skewness from raw power sums along axis 0; (skew, m2).  m2 <= 0 gives NaN."""
    T = float(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = sums[0] / T
        m2 = sums[1] / T - mu * mu
        m3 = sums[2] / T - 3.0 * mu * (sums[1] / T) + 2.0 * mu * mu * mu
        return np.where(m2 > 0.0, m3 / np.where(m2 > 0.0, m2, 1.0) ** 1.5, np.nan), m2


def skew_two_pass(v):
    """MATLAB's skewness(v, 1, 2) the textbook way: centred moments."""
    v = np.asarray(v, dtype=np.float64)
    c = v - v.mean(axis=1, keepdims=True)
    m2 = (c * c).mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m2 > 0.0, (c * c * c).mean(axis=1) / np.where(m2 > 0.0, m2, 1.0) ** 1.5, np.nan)


def excluded_components(W, m2_own):
    K = W.shape[0]
    floor = W.reshape(K, -1).max(axis=1) <= EPS
    wflat2 = W.sum(axis=2) ** 2
    one_unit = wflat2.max(axis=1) > 0.999 * wflat2.sum(axis=1)
    flat = ~(np.asarray(m2_own) > 0.0)
    return floor | one_unit | flat


def decide(W, sums, T, p=0.05):
    """From the (3, K, 1 + nnull) sums of draws 0 .. nnull: dict of pvals, is_significant, skew, skewnull, excluded."""
    K = W.shape[0]
    nnull = sums.shape[2] - 1
    sk, m2 = skew_from_sums(sums, T)
    skew, skewnull = sk[:, 0], sk[:, 1:]
    excluded = excluded_components(W, m2[:, 0])
    kept = int((~excluded).sum())
    pvals = np.full(K, np.inf)
    sig = np.zeros(K, dtype=bool)
    for k in range(K):
        if excluded[k]:
            continue
        pvals[k] = (1 + int(np.sum(skewnull[k] > skew[k]))) / nnull
        sig[k] = pvals[k] <= p / kept
    return {"pvals": pvals, "is_significant": sig, "skew": skew, "skewnull": skewnull, "excluded": excluded}


def default_nnull(K, p):
    return 2 * int(math.ceil(K / p))


def evaluate(W, X, p=0.05, nnull=None, seed=0, contraction=np.float64):
    nnull = default_nnull(W.shape[0], p) if nnull is None else nnull
    return decide(W, null_moments(W, X, seed, range(1 + nnull), contraction), X.shape[1], p)


# ---- the problems of the tests ------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(6, 5, 3, 8), (7, 130, 1, 1), (13, 300, 5, 7), (40, 257, 33, 20), (24, 200, 32, 33), (130, 700, 16, 20)]  # (N, T', K, L)
EXACT_DRAWS = 13  # draws 0 .. 12
EXACT_SEED = 20261021


def exact_problem(shape, which=0):
    """X: hashed integers in {0..3}, W: hashed integers in {0, 1, 2} (`which` selects one of several W).  Every overlap is an integer
    below 2^24, so the fp32 contraction is exact in any order, and with T' vmax^3 < 2^53 so are the fp64 power sums."""
    N, T, K, L = shape
    X = np.asfortranarray(hashed_ints(EXACT_SEED, 1, (N, T), 4))
    W = np.asfortranarray(hashed_ints(EXACT_SEED, 2 + which, (K, N, L), 3))
    return W, X


def assert_exact_precondition(W, X, sums):
    """From the arrays: the largest overlap any null motif can reach, vmax <= sum_n (sum_l W[k, n, l]) max_t X[n, t] ... bounded here by
    the cruder max X * max_k sum_{n, l} W, stays below 2^24 and T' vmax^3 below 2^53."""
    vmax = float(X.max()) * float(W.sum(axis=(1, 2)).max())
    assert vmax < 2**24, vmax
    assert X.shape[1] * vmax**3 < 2**53, (X.shape[1], vmax)
    assert np.all(sums == np.round(sums))


PLANTED_SHAPE = (30, 600, 3, 8)  # (N, T', K, L): two planted sequences and one unstructured component
PLANTED_SEED = 7
PLANTED_NNULL = 120


def planted_problem():
    """Held-out data with two planted sequences (component 0 sweeps units 0 .. 14 forwards through the lags, component 1 units 15 .. 29
    backwards) plus noise, and an unstructured component: random weights on every unit and lag that the data holds no events of."""
    N, T, K, L = PLANTED_SHAPE
    u = lambda stream, shape: ((bits(base(PLANTED_SEED, stream), np.arange(int(np.prod(shape)), dtype=U)) >> U(11)).astype(np.float64) * 2.0**-53).reshape(shape)
    W = np.zeros((K, N, L))
    for n in range(15):
        W[0, n, (n * L) // 15] = 1.0
        W[1, 15 + n, L - 1 - (n * L) // 15] = 1.0
    W[:2] += 0.02 * u(1, (2, N, L))
    W[2] = u(2, (N, L)) * (2.0 / L)
    H = np.where(u(3, (K, T)) < 0.03, 0.5 + u(4, (K, T)), 0.0)
    H[2] = 0.0
    X = np.zeros((N, T))
    for l in range(L):
        X[:, l:] += np.einsum("kn,kt->nt", W[:, :, l], H[:, : T - l])
    X += 0.1 * u(5, (N, T))
    return np.asfortranarray(W), np.asfortranarray(X)


SPLIT_SHAPE = (40, 600, 5, 10)  # (N, T', K, L): the last quarter of a gen_synthetic recording of three sequences, fitted with K = 5
SPLIT_SEED = 4321
SPLIT_T = 2400
SPLIT_ITERS = 30


def split_problem(oracle):
    """(W, test) on the CPU: gen_synthetic (datasets/synthetic.jl:29-61) with three sequences, the MU rule of the oracle for 30
    iterations on the first three quarters with K = 5, the last quarter held out.  The GPU test fits the same split on the device."""
    N, Tt, K, L = SPLIT_SHAPE
    data = oracle.c_gen_synthetic(N=N, T=SPLIT_T, K=3, L=L, seed=SPLIT_SEED)[0]
    train, test = data[:, : SPLIT_T - Tt], data[:, SPLIT_T - Tt :]
    W0, H0 = oracle.c_init_rand(np.asfortranarray(train), L, K, SPLIT_SEED)
    W = oracle.c_fit_mult(np.asfortranarray(train), W0, H0, max_itr=SPLIT_ITERS, check_convergence=False)[0]
    return np.asfortranarray(W), np.asfortranarray(test)
