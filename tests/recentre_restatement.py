"""seqNMF's re-centring of motifs (shiftFactors.m), restated in fp64 numpy.

The definition (include/cmf_hip.h: cmf_recentre_shifts, cmf_recentre, cmf_mu_set_recentre), in 0-based lags, for
component k of a K x N x L W and a K x T H:

  mass     c_l = sum_n W[k, n, l] (n ascending, from 0.0),  m0 = sum_l c_l,  m1 = sum_l (l + 1) c_l (lags ascending, from 0.0); fp64
  shift    c = max(floor(m1 / m0), 1) (capped at 2^30),  centre = max(floor(L / 2), 1),  s_k = centre - c
           s_k = 0 where L == 1, where m0 is zero or m0, m1 are not finite, where no entry of W[k] lies above the MU clamp floor
  move     W'[k, n, l] = W[k, n, l - s_k] where 0 <= l - s_k < L,  H'[k, t] = H[k, t + s_k] where 0 <= t + s_k < T,
           every vacated entry = the clamp floor eps(Float64)
  place    in an MU iteration (mult.jl:42-58): behind the element-wise update of H (:51-52), in front of the loss conv (:55-57)

`mutation` breaks the definition in one of five ways an implementation could (MUTATIONS); tests/test_recentre_cpu.py shows that each
fails the exact comparison on a stated shape.  `fit_mu_recentred` is the oracle's MU iteration with the step placed as above; with
dtype=np.float32 it is the model of the device the precision tool uses: float32 factors, float32 contractions and element-wise
updates, the masses still summed in fp64 from the float32 W.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cmf_oracle as orc  # noqa: E402

EPS = 2.220446049250313e-16
C_MAX = 1 << 30

MUTATIONS = ("h_same_way", "w_wrapped", "zero_based_m1", "rounded", "no_dead_rule")


def masses(W):
    """(m0, m1, live): the fp64 sums of the definition, in its order, and whether a component has an entry above the floor."""
    W = np.asarray(W, dtype=np.float64)
    K, N, L = W.shape
    c = np.zeros((K, L))
    for n in range(N):  # n ascending, from 0.0
        c += W[:, n, :]
    m0, m1 = np.zeros(K), np.zeros(K)
    for l in range(L):  # lags ascending, from 0.0
        m0 += c[:, l]
        m1 += float(l + 1) * c[:, l]
    return m0, m1, (W > EPS).any(axis=(1, 2))


def ratios(W):
    """m1 / m0 per component (nan where the definition does not divide)."""
    m0, m1, _ = masses(W)
    with np.errstate(all="ignore"):
        return np.where((m0 != 0) & np.isfinite(m0) & np.isfinite(m1), m1 / np.where(m0 != 0, m0, 1.0), np.nan)


def shifts(W, mutation=None):
    """The K shifts of the definition (int64)."""
    W = np.asarray(W, dtype=np.float64)
    K, N, L = W.shape
    m0, m1, live = masses(W)
    if mutation == "zero_based_m1":
        m1 = m1 - m0
    if mutation == "no_dead_rule":
        live = np.ones(K, dtype=bool)
    centre = max(L // 2, 1)
    s = np.zeros(K, dtype=np.int64)
    for k in range(K):
        if L == 1 or not live[k] or m0[k] == 0.0 or not math.isfinite(m0[k]) or not math.isfinite(m1[k]):
            continue
        r = m1[k] / m0[k]
        r = math.floor(r + 0.5) if mutation == "rounded" else math.floor(r)
        s[k] = centre - (C_MAX if r >= C_MAX else max(int(r), 1))
    return s


def move(W, H, s, mutation=None, circular_H=False, fill=EPS):
    """W and H moved by the shifts s (new arrays).  circular_H: seqNMF's own form of the H shift (circshift)."""
    W, H = np.asarray(W), np.asarray(H)
    K, N, L = W.shape
    T = H.shape[1]
    W2, H2 = np.full_like(W, fill), np.full_like(H, fill)
    for k in range(K):
        sk = int(s[k])
        if mutation == "w_wrapped":
            W2[k] = np.roll(W[k], sk, axis=1)
        else:
            lo, hi = max(sk, 0), min(L + sk, L)
            if hi > lo:
                W2[k, :, lo:hi] = W[k, :, lo - sk:hi - sk]
        sh = -sk if mutation == "h_same_way" else sk
        if circular_H:
            H2[k] = np.roll(H[k], -sh)
        else:
            lo, hi = max(-sh, 0), min(T - sh, T)
            if hi > lo:
                H2[k, lo:hi] = H[k, lo + sh:hi + sh]
    return W2, H2


def recentre(W, H, mutation=None, circular_H=False):
    """One step: (W', H', shifts)."""
    s = shifts(W, mutation)
    W2, H2 = move(W, H, s, mutation, circular_H)
    return W2, H2, s


# ---- the MU iteration with the step in place ---------------------------------------------------------------------------------------
def _update_motifs(data, W, H, dtype):
    """mult.jl:23-39 in `dtype` (the oracle's update_motifs, lag by lag)."""
    K, N, L = W.shape
    T = H.shape[1]
    est = orc.tensor_conv(W, H, out=np.zeros(data.shape, dtype=dtype))
    num, den = np.zeros(W.shape, dtype=dtype), np.zeros(W.shape, dtype=dtype)
    for lag in range(min(L, T)):
        num[:, :, lag] = H[:, : T - lag] @ data[:, lag:].T
        den[:, :, lag] = H[:, : T - lag] @ est[:, lag:].T
    W *= num / (den + dtype(EPS))
    np.maximum(W, dtype(EPS), out=W)


def _update_h(data, W, H, dtype):
    """mult.jl:44-52 in `dtype`."""
    est = orc.tensor_conv(W, H, out=np.zeros(data.shape, dtype=dtype))
    num = orc.tensor_transconv(W, data, out=np.zeros(H.shape, dtype=dtype))
    den = orc.tensor_transconv(W, est, out=np.zeros(H.shape, dtype=dtype))
    H *= num / (den + dtype(EPS))
    np.maximum(H, dtype(EPS), out=H)


def fit_mu_recentred(data, W_init, H_init, n_iter, shift=True, dtype=np.float64, eval_mode=False):
    """n_iter iterations of the MU rule with the re-centring step between the H update and the loss conv.
    Returns dict(W, H, loss_hist (n_iter + 1), shifts (n_iter x K), moved (K), ratios (n_iter x K: m1 / m0 in front of every step))."""
    data64 = np.asarray(data, dtype=np.float64)
    data = data64.astype(dtype)
    W, H = np.array(W_init, dtype=dtype, copy=True), np.array(H_init, dtype=dtype, copy=True)
    K = W.shape[0]
    norm = np.linalg.norm(data64)

    def loss():
        est = orc.tensor_conv(W, H, out=np.zeros(data.shape, dtype=dtype))
        return float(np.linalg.norm(est.astype(np.float64) - data64) / norm)

    hist, all_s, all_r, moved = [loss()], [], [], np.zeros(K, dtype=np.int64)
    for _ in range(n_iter):
        if dtype is np.float64 and not eval_mode:
            rule = orc.MultUpdate(data, W, H)
            orc.update_motifs(rule, data, W, H)  # (the oracle's own, in place)
        elif not eval_mode:
            _update_motifs(data, W, H, dtype)
        _update_h(data, W, H, dtype)
        if shift and not eval_mode:
            all_r.append(ratios(W))
            s = shifts(W)
            if s.any():
                W[...], H[...] = move(W, H, s, fill=dtype(EPS))
            all_s.append(s)
            moved += np.abs(s)
        hist.append(loss())
    return dict(W=W, H=H, loss_hist=np.asarray(hist), shifts=np.asarray(all_s, dtype=np.int64).reshape(-1, K), moved=moved,
                ratios=np.asarray(all_r).reshape(-1, K))


def shift_cases():
    """name -> (W, expected shifts or None): the stated cases of the shift decision.  Every entry is an integer or the floor, so every
    sum is exact and a float32 copy holds the same values."""
    rng = np.random.default_rng(20261021)
    out = {}
    out["L1"] = (rng.integers(1, 9, size=(2, 5, 1)).astype(np.float64), np.zeros(2, dtype=np.int64))
    W = rng.integers(0, 9, size=(33, 7, 9)).astype(np.float64)
    for k in range(33):
        W[k, :, k % 9] += 40.0  # a peak at a lag of the component's own
    out["K33"] = (W, None)
    for L in (7, 8):
        centre = L // 2
        W = np.zeros((2, 3, L))
        W[0, :, 0] = 5.0       # all mass at lag 0: c = 1
        W[1, :, L - 1] = 3.0   # all mass at lag L - 1: c = L
        out[f"ends_L{L}"] = (W, np.array([centre - 1, centre - L]))
        out[f"dead_L{L}"] = (np.full((2, 4, L), EPS), np.zeros(2, dtype=np.int64))  # uniform and dead: m1 / m0 = (L + 1) / 2
    W = np.zeros((3, 2, 6))
    W[0, :, 1] = W[0, :, 3] = 4.0   # m1 / m0 = (2 + 4) / 2 = 3 exactly
    W[1, :, 1] = W[1, :, 2] = 4.0   # 2.5: floor 2, rounding 3
    W[2, :, 4] = 1.0                # 5
    out["integer_ratio"] = (W, np.array([0, 1, -2]))
    W = np.zeros((3, 2, 6))
    W[0, 0, 1], W[0, 1, 4] = 1.0, -1.0  # live, m0 = 0
    W[2, :, 5] = 2.0                    # (component 1 all zero: m0 = 0 and dead)
    out["m0_zero"] = (W, np.array([0, 0, -3]))
    return out


def centre_of_mass(W):
    """The 1-based centre of mass m1 / m0 per component."""
    return ratios(W)


# ---- problems of the GPU tests (tests/test_gpu_recentre.py), portable: every number comes from exact_problems._hash ------------------
def _u(shape, salt, levels=1024):
    """Hashed multiples of 1 / levels in [0, 1): exact in float32."""
    import exact_problems as ep

    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return (ep._hash(idx, salt=salt) % np.uint64(levels)).astype(np.float64) / levels


def exact_step_problem(shape):
    """(W, H) for the bit-for-bit test of one step: integers and the floor only, so the masses are exact in any order.  Component k
    follows pattern k mod 6: all mass at lag 0 (the largest shift up), all mass at lag L - 1 (the largest shift down), all mass at the
    centre (no shift), dead, an exactly integer ratio off the centre, dense."""
    import exact_problems as ep

    N, T, K, L = shape
    k, n, l = np.meshgrid(np.arange(K), np.arange(N), np.arange(L), indexing="ij")
    dense = 1.0 + (ep._hash(k, n, l, salt=77) % np.uint64(3)).astype(np.float64)
    W = np.zeros((K, N, L))
    centre = max(L // 2, 1)
    for kk in range(K):
        p = kk % 6
        if p == 0:
            W[kk, :, 0] = dense[kk, :, 0]
        elif p == 1:
            W[kk, :, L - 1] = dense[kk, :, L - 1]
        elif p == 2:
            W[kk, :, min(centre - 1, L - 1)] = dense[kk, :, 0]
        elif p == 3:
            W[kk] = EPS
        elif p == 4:
            W[kk, :, 0] = W[kk, :, min(2, L - 1)] = 2.0  # m1 / m0 = 2 at L >= 3
        else:
            W[kk] = dense[kk]
    kk, tt = np.meshgrid(np.arange(K), np.arange(T), indexing="ij")
    H = 1.0 + (ep._hash(kk, tt, salt=78) % np.uint64(4)).astype(np.float64)
    return np.asfortranarray(W), np.asfortranarray(H)


def sequence_data(N, T, K, L, seed, width=None, rate=24, noise=1.0 / 16):
    """(data, W_true, H_true): K planted sequences (unit n of motif k fires once, at a lag that grows with n, within `width` lags),
    sparse hashed event times, plus hashed noise; all values multiples of 2^-10."""
    import exact_problems as ep

    width = width or L
    W = np.zeros((K, N, L))
    for k in range(K):
        for n in range(N):
            W[k, n, ((n + 3 * k) * width // N) % width] = 1.0
    kk, tt = np.meshgrid(np.arange(K), np.arange(T), indexing="ij")
    H = (ep._hash(kk, tt, salt=seed * 8 + 1) % np.uint64(rate) == 0).astype(np.float64)
    data = orc.tensor_conv(W, H) + noise * _u((N, T), seed * 8 + 2)
    return np.asfortranarray(data), np.asfortranarray(W), np.asfortranarray(H)


# the whole-fit fixtures (tests/golden/mu_recentre_<name>.npz, made by tests/golden/make_golden_recentre.py; admitted by
# tools/mu_recentre_precision.py): name -> (N, T, K, L, seed, iterations)
FIXTURES = {"few": (130, 700, 3, 8, 1, 12), "general": (40, 600, 32, 5, 2, 10)}


def fixture_problem(name):
    """(data, W_init, H_init, n_iter) of a fixture: planted sequences, hashed initial factors in [1/16, 1 + 1/16)."""
    N, T, K, L, seed, n_iter = FIXTURES[name]
    data, _, _ = sequence_data(N, T, min(K, 3), L, seed)
    W0 = np.asfortranarray(1.0 / 16 + _u((K, N, L), seed * 8 + 3))
    H0 = np.asfortranarray(1.0 / 16 + _u((K, T), seed * 8 + 4))
    return data, W0, H0, n_iter


BEHAVIOUR = dict(N=20, T=300, K=1, L=10, width=8, displaced=4, seed=5, n_iter=60)


def behaviour_problem():
    """(data, W_init, H_init, n_iter): one planted sequence 8 lags wide in a 10-lag window; the fit starts from the planted motif
    displaced by 4 lags towards the end of the window (what passes the end is cut off) with its H moved to match."""
    b = BEHAVIOUR
    data, Wt, Ht = sequence_data(b["N"], b["T"], b["K"], b["L"], b["seed"], width=b["width"])
    d = b["displaced"]
    W0, H0 = np.full(Wt.shape, EPS), np.full(Ht.shape, EPS)
    W0[:, :, d:] = np.maximum(Wt[:, :, : b["L"] - d], EPS)
    H0[:, : b["T"] - d] = np.maximum(Ht[:, d:], EPS)  # the events d columns earlier: W0 * H0 places the motif where the data have it
    return data, np.asfortranarray(W0), np.asfortranarray(H0), b["n_iter"]
