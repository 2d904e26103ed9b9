"""seqNMF's cross-orthogonality penalties on the MU rule, restated literally in fp64 numpy (the reference for
tests/test_xortho_mu_cpu.py, tests/test_gpu_xortho_mu.py, tools/mu_xortho_precision.py and the fixtures tests/golden/mu_xortho_*.npz,
which `write_fixtures` below writes).

Indices as in the reference: W[k, n, l], H[k, t], data[n, t].  With

    S(A)[k, t]   = sum of A[k, t'] over |t' - t| <= L - 1, 0 <= t' < T     (seqNMF's conv2(A, ones(1, 2L-1), 'same'))
    off(A)[k, :] = sum of A[k', :] over k' != k
    A = tensor_transconv(W, data)  (the rule's numH),   G = off(S(H)),   Wflat[k, n] = sum_l W[k, n, l]

the objective is 1/2 |data - tensor_conv(W, H)|^2 + lam sum_{i != j} (A S H')_ij + lamH / 2 sum_{i != j} (H S H')_ij
+ lamW / 2 sum_{i != j} (Wflat' Wflat)_ij, and the rule is src/algs/mult.jl:23-58 with each denominator enlarged BEFORE the regularisers:

    xW[k, n, l] = sum_t G[k, t] data[n, t + l]     (mult.jl:32 with G in H's place)         oW[k, n, l] = off(Wflat)[k, n]
    W <- max(eps, W .* (numW ./ ((((denomW + (lam xW + lamW oW)) + l1W) + (2 l2W) W) + eps)))
    xH = off(S(A))  (A from the NEW W: the numH of the same call)                            oH = G  (from the H being updated)
    H <- max(eps, H .* (numH ./ ((((denomH + (lam xH + lamH oH)) + l1H) + (2 l2H) H) + eps)))

loss_hist stays norm(est - data) / norm(data).  S and off are direct sums of the terms (no differences of running sums).  With all
weights 0 every operation is the oracle's MU rule (oracle/cmf_oracle.py) in the oracle's order: tests/test_xortho_mu_cpu.py holds
the two together bit for bit.

`cdtype`: the number format of the CONTRACTIONS and of the element-wise epilogue (S, off, the denominators, the quotient), float32
in tools/mu_xortho_precision.py's model of the device; everything is fp64 otherwise.
"""
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)  # eps(): src/CMF.jl:20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _c(a, cdtype):
    return a if cdtype is np.float64 else a.astype(cdtype)


def tensor_conv(W, H, cdtype=np.float64):
    """tensor_conv!: src/common.jl:24-34 (the oracle's loop)."""
    K, N, L = W.shape
    T = H.shape[1]
    est = np.zeros((N, T))
    Wc, Hc = _c(W, cdtype), _c(H, cdtype)
    for lag in range(min(L, T)):
        est[:, lag:] += Wc[:, :, lag].T @ Hc[:, : T - lag]
    return est


def tensor_transconv(W, X, cdtype=np.float64):
    """tensor_transconv!: src/common.jl:71-81 (the oracle's loop)."""
    K, N, L = W.shape
    T = X.shape[1]
    res = np.zeros((K, T))
    Wc, Xc = _c(W, cdtype), _c(X, cdtype)
    for lag in range(min(L, T)):
        res[:, : T - lag] += Wc[:, :, lag] @ Xc[:, lag:]
    return res


def hxt(H, X, L, cdtype=np.float64):
    """out[:, :, l] = shift_cols(H, l) * X[:, 1+l:T]' (mult.jl:32-33), one GEMM per lag; lags l >= T stay 0."""
    K, T = H.shape
    out = np.zeros((K, X.shape[0], L))
    Hc, Xc = _c(H, cdtype), _c(X, cdtype)
    for lag in range(L):
        if lag < T:
            out[:, :, lag] = Hc[:, : T - lag] @ Xc[:, lag:].T
    return out


def smooth(A, L):
    """S(A): the box sum of width 2L - 1 along t, cut at both ends, as a direct sum of the terms."""
    K, T = A.shape
    out = np.zeros((K, T), dtype=A.dtype)
    for t in range(T):
        for tp in range(max(0, t - (L - 1)), min(T, t + L)):
            out[:, t] += A[:, tp]
    return out


def off(A):
    """off(A): for every component the sum over the OTHER components (along axis 0), as a direct sum of the terms."""
    out = np.zeros_like(A)
    K = A.shape[0]
    for k in range(K):
        for kp in range(K):
            if kp != k:
                out[k] += A[kp]
    return out


def terms(data, W, H, cdtype=np.float64):
    """(xW, xH, oH, oW): the four unweighted denominator terms for the factors as they are, in the shapes of W, H, H and W."""
    K, N, L = W.shape
    G = off(smooth(_c(H, cdtype), L)).astype(np.float64)
    xW = hxt(G, data, L, cdtype)
    xH = off(smooth(_c(tensor_transconv(W, data, cdtype), cdtype), L)).astype(np.float64)
    oW = np.repeat(off(_c(W, cdtype).sum(axis=2))[:, :, None], L, axis=2).astype(np.float64)
    return xW, xH, G, oW


def costs(data, W, H):
    """(xortho, ortho_H, ortho_W): the three penalty sums without their weights and without the 1/2."""
    L = W.shape[2]
    A = tensor_transconv(W, data)
    G = off(smooth(H, L))
    Wf = W.sum(axis=2)
    return float(np.sum(A * G)), float(np.sum(H * G)), float(np.sum(Wf * off(Wf)))


def costs_literal(data, W, H):
    """The same three sums as the objective states them: off-diagonal sums of A S H', H S H' and Wflat' Wflat (for the tests)."""
    L = W.shape[2]
    A = tensor_transconv(W, data)
    SH = smooth(H, L)
    Wf = W.sum(axis=2)

    def offdiag(M):
        return float(np.sum(M) - np.trace(M))

    return offdiag(A @ SH.T), offdiag(H @ SH.T), offdiag(Wf @ Wf.T)


def penalty(data, W, H, lam=0.0, lamH=0.0, lamW=0.0):
    """The penalty part of the objective: lam xortho + lamH / 2 ortho_H + lamW / 2 ortho_W."""
    x, oh, ow = costs_literal(data, W, H)
    return lam * x + 0.5 * lamH * oh + 0.5 * lamW * ow


def compute_loss(data, W, H, cdtype=np.float64):
    """compute_loss: src/common.jl:54-59."""
    return np.linalg.norm(tensor_conv(W, H, cdtype) - data) / np.linalg.norm(data)


def update_motifs(data, W, H, lam=0.0, lamH=0.0, lamW=0.0, l1W=0.0, l2W=0.0, cdtype=np.float64):
    """update_motifs! with the penalties.  W in place."""
    K, N, L = W.shape
    est = tensor_conv(W, H, cdtype)  # :28
    numW = hxt(H, data, L, cdtype)  # :32
    denomW = hxt(H, est, L, cdtype)  # :33
    if lam != 0.0 or lamW != 0.0:
        xW = hxt(off(smooth(_c(H, cdtype), L)).astype(np.float64), data, L, cdtype) if lam != 0.0 else 0.0
        oW = off(_c(W, cdtype).sum(axis=2)).astype(np.float64)[:, :, None] if lamW != 0.0 else 0.0
        denomW = denomW + (lam * xW + lamW * oW)
    den = ((denomW + l1W) + (2.0 * l2W) * W) + EPS  # :37
    W *= numW / den
    np.maximum(W, EPS, out=W)  # :38
    return W


def update_feature_maps(data, W, H, lam=0.0, lamH=0.0, lamW=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64):
    """update_feature_maps! with the penalties.  H in place; returns the loss."""
    L = W.shape[2]
    est = tensor_conv(W, H, cdtype)  # :44 (est with the new W)
    numH = tensor_transconv(W, data, cdtype)  # :47
    denomH = tensor_transconv(W, est, cdtype)  # :48
    if lam != 0.0 or lamH != 0.0:
        xH = off(smooth(_c(numH, cdtype), L)).astype(np.float64) if lam != 0.0 else 0.0
        oH = off(smooth(_c(H, cdtype), L)).astype(np.float64) if lamH != 0.0 else 0.0
        denomH = denomH + (lam * xH + lamH * oH)
    den = ((denomH + l1H) + (2.0 * l2H) * H) + EPS  # :51
    H *= numH / den
    np.maximum(H, EPS, out=H)  # :52
    return np.linalg.norm(tensor_conv(W, H, cdtype) - data) / np.linalg.norm(data)  # :55-57


def fit(data, W_init, H_init, lam=0.0, lamH=0.0, lamW=0.0, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, eval_mode=False,
        cdtype=np.float64):
    """alternating.jl:16-71 without the stop tests: (W, H, loss_hist) after exactly max_itr iterations."""
    data = np.asarray(data, dtype=np.float64)
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [compute_loss(data, W, H, cdtype)]
    for _ in range(int(max_itr)):
        if not eval_mode:
            update_motifs(data, W, H, lam, lamH, lamW, l1W=l1W, l2W=l2W, cdtype=cdtype)
        loss_hist.append(update_feature_maps(data, W, H, lam, lamH, lamW, l1H=l1H, l2H=l2H, cdtype=cdtype))
    return W, H, np.asarray(loss_hist)


def component_norms(W, H):
    """The Frobenius norm of every component's reconstruction tensor_conv(W[k], H[k])."""
    return np.array([np.linalg.norm(tensor_conv(W[k : k + 1], H[k : k + 1])) for k in range(W.shape[0])])


def dead_components(W, H, rel=1e-6):
    """How many components' reconstruction norms lie below `rel` of the largest."""
    n = component_norms(W, H)
    return int(np.sum(n < rel * n.max()))


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)  # (the regularisers of mu_small_reg.npz)
LAM = 0.02  # the fixtures' lambda (on the planted problems the x-ortho cost then ends below a quarter of the lambda = 0 fit's: the tests)
WEIGHT_SETS = {"x": (LAM, 0.0, 0.0), "all": (LAM, 0.005, 0.05)}
SHAPE_LAM = {"k33": 0.001, "k32": 0.001, "l40": 0.002}  # the penalty grows with the number of other components: LAM would kill all 32 at once


def weights_of(shape_name, wset):
    """(lam, lamH, lamW) of a fixture: WEIGHT_SETS, scaled to the shape's lambda where SHAPE_LAM names one."""
    f = SHAPE_LAM.get(shape_name, LAM) / LAM
    return tuple(f * w for w in WEIGHT_SETS[wset])


SWEEP_LAMBDAS = (0.0, 0.005, 0.02)  # xortho_sweep on `small`: the loss rises and the x-ortho cost falls, strictly, along these
# name, (N, T, K, L), planted sequences, regularisers, how W and H are stored, the count asked for (the beta shapes and l1, k1, edge)
SHAPES = [("small", (48, 300, 4, 8), 2, {}, False, 100), ("small_reg", (48, 300, 4, 8), 2, REG, False, 20),
          ("k5", (70, 257, 5, 10), 2, {}, False, 100), ("k33", (70, 300, 33, 6), 3, {}, True, 20),
          ("k32", (96, 1000, 32, 12), 3, {}, "norms", 20), ("short", (20, 7, 2, 10), 1, {}, False, 20),
          ("l40", (45, 130, 16, 40), 2, {}, True, 20),
          ("l1", (30, 200, 4, 1), 2, {}, False, 20), ("k1", (30, 200, 1, 8), 1, {}, False, 20), ("edge", (24, 14, 3, 8), 1, {}, False, 20)]
CASES = [(f"mu_xortho_{s}_{w}", s, w) for s, *_ in SHAPES for w in WEIGHT_SETS]
PLANTED = "mu_xortho_small_x"  # the fixture the behavioural tests run on


def shape_row(shape_name):
    for row in SHAPES:
        if row[0] == shape_name:
            return row
    raise KeyError(shape_name)


def planted_problem(N, T, K, L, planted, seed):
    """Inputs that store compactly: data from the project's portable generator (oracle.c_gen_synthetic: `planted` sequences of length L
    in noise) rounded to a grid of 1/32 and held as uint8, initial factors float16 values on a grid of 64 -- all exactly representable
    in the device's float32.  K is the number of components FITTED, above the planted count.  Returns (data uint8, W0, H0 float16)."""
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import cmf_oracle as oc

    data, _, _ = oc.c_gen_synthetic(N=N, T=T, K=planted, L=L, seed=seed)
    q = np.clip(np.rint(np.asarray(data) * 32.0), 0, 255).astype(np.uint8)
    if not q.any():
        q[0, 0] = 32
    rng = np.random.default_rng(seed)
    W0 = (rng.integers(0, 64, (K, N, L)) / 64.0 + 0.125).astype(np.float16)
    H0 = (rng.integers(0, 64, (K, T)) / 64.0 + 0.125).astype(np.float16)
    return q, W0, H0


def inputs(shape_name):
    """(data, W0, H0, regularisers) of a fixture shape as float64 arrays (data on its grid of 1/32)."""
    _, shape, planted, reg, _, _ = shape_row(shape_name)
    q, W0, H0 = planted_problem(*shape, planted, seed=5)
    return q.astype(np.float64) / 32.0, W0.astype(np.float64), H0.astype(np.float64), reg


def admitted(path=None):
    path = path or os.path.join(os.path.dirname(GOLDEN), os.pardir, "profiles", "mu_xortho_precision.txt")
    out = {}
    for line in open(path):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


def load_fixture(path):
    """A tests/golden/mu_xortho_*.npz file as float64 arrays: data, W0, H0, W, H, loss_hist, the weights (lam, lamH, lamW), max_itr and
    the regularisers.  A fixture whose W and H would not fit the size agreed for golden files holds their float32 roundings (W32 /
    H32) or their Frobenius norms only: W and H are then recomputed here and must reproduce the stored loss_hist and norms."""
    g = np.load(path)
    out = {"data": np.asarray(g["data8"], dtype=np.float64) / 32.0, "W0": np.asarray(g["W0"], dtype=np.float64),
           "H0": np.asarray(g["H0"], dtype=np.float64), "loss_hist": np.asarray(g["loss_hist"], dtype=np.float64)}
    out["max_itr"] = int(g["max_itr"])
    out["weights"] = tuple(float(g[k]) for k in ("lam", "lamH", "lamW"))
    out["reg"] = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")}
    out["costs"] = tuple(float(v) for v in g["costs"])
    if "W" in g.files or "W32" in g.files:
        out["W"] = np.asarray(g["W"] if "W" in g.files else g["W32"], dtype=np.float64)
        out["H"] = np.asarray(g["H"] if "H" in g.files else g["H32"], dtype=np.float64)
    else:
        W, H, lh = fit(out["data"], out["W0"], out["H0"], *out["weights"], max_itr=out["max_itr"], **out["reg"])
        np.testing.assert_allclose(lh, out["loss_hist"], rtol=1e-10)
        np.testing.assert_allclose([np.linalg.norm(W), np.linalg.norm(H)], [float(g["W_norm"]), float(g["H_norm"])], rtol=1e-10)
        out["W"], out["H"] = W, H
    return out


def write_fixtures(admit=None):
    """Writes tests/golden/mu_xortho_*.npz: every shape at both weight sets, at the count the shape asks for or, where
    profiles/mu_xortho_precision.txt admits fewer (the fp32 model leaves the fp64 run where components die), at the admitted count."""
    admit = admitted() if admit is None else admit
    for name, s, wset in CASES:
        _, shape, planted, reg, r32, want = shape_row(s)
        q, W0, H0 = planted_problem(*shape, planted, seed=5)
        lam, lamH, lamW = weights_of(s, wset)
        itr = min(want, admit[name])
        assert itr >= 1, f"profiles/mu_xortho_precision.txt admits no iteration on {name}"
        data = q.astype(np.float64) / 32.0
        W, H, lh = fit(data, W0.astype(np.float64), H0.astype(np.float64), lam, lamH, lamW, max_itr=itr, **reg)
        r = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
        r.update(reg)
        out = (dict(W_norm=np.linalg.norm(W), H_norm=np.linalg.norm(H)) if r32 == "norms"
               else dict(W32=W.astype(np.float32), H32=H.astype(np.float32)) if r32 else dict(W=W, H=H))
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, data8=q, W0=W0, H0=H0, loss_hist=lh, max_itr=itr, lam=lam, lamH=lamH, lamW=lamW,
                            costs=np.asarray(costs(data, W, H)), **out, **r)
        print(name, data.shape, "K, N, L =", W0.shape, "loss", lh[0], "->", lh[-1], "dead", dead_components(W, H), os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 250_000


if __name__ == "__main__":
    write_fixtures()
