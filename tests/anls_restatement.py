"""fp64 numpy restatement of the reference's ANLS rule (src/algs/anls.jl) on the HEAD layout: data (N, T), W (K, N, L),
H (K, T), stacked row index l*K + k (shift_and_stack, common.jl:133-142).  anls.jl itself is written for the old L x N x K
layout of W; the arithmetic is restated, not the indexing.

The NNLS solver is block principal pivoting (Kim & Park, SIAM J. Sci. Comput. 33(6), 2011) on the normal equations
G x = c, restated from the paper: it stands for nonneg_lsq(A, B; alg=:pivot, tol=1e-5) of NonNegLeastSquares.jl, whose
source is not available here.  Assumptions: `tol` is an absolute threshold on x_i (i in the passive set P)
and on y_i = (G x - c)_i (i off P); entries off P are returned as exact zeros and entries in P are clipped at zero.

Two modes of the same computation:
  - "literal": anls.jl statement by statement -- Hstk' and data' handed to the solver (:47-57); the residual kept and
    edited window by window, the unfolded W cut to the window's rows (:63-94, :101-137).
  - "gram": the rewriting the GPU path uses -- G and C of the W step lag by lag without Hstk; for the H step
    B = transconv(W, data) and the lag-Grams A_Lt(e), c = B[:, t] - sum_{e != 0} A_Lt(e) H[:, t+e]; no residual is carried
    and the loss is norm(conv(W, H) - data) / norm(data), computed once after the sweep.

`stats` (a dict, optional) receives: exchanges (pivoting rounds summed over the problems), backup (problems that took the
backup rule), capped (problems that hit the cap on rounds; their answer is not to be used), near (a boolean array shaped
like the factor: entries the solver itself calls near-degenerate -- a zero with |y| < 1e-6 max|c| or a positive entry
below 1e-6 max|x| of its problem).
"""
import numpy as np

NNLS_TOL = 1e-5  # anls.jl:18
NEAR = 1e-6


def conv(W, H):
    """tensor_conv (common.jl:21-32): est[n, t] = sum_l W[:, n, l]' H[:, t-l]."""
    return stack_W(W).T @ shift_and_stack(H, W.shape[2])


def shift_and_stack(H, L):
    K, T = H.shape
    S = np.zeros((L * K, T))
    for l in range(min(L, T)):
        S[l * K:(l + 1) * K, l:] = H[:, :T - l]
    return S


def stack_W(W):
    K, N, L = W.shape
    return W.transpose(2, 0, 1).reshape(L * K, N)


def fold_W(X, K, N, L):
    """fold_W (anls.jl:150-157) on the HEAD layout: W[k, n, l] = X[l*K+k, n]."""
    return np.ascontiguousarray(X.reshape(L, K, N).transpose(1, 2, 0))


def unfold_W(W):
    """_unfold_W (anls.jl:140-143): row l*N + n, column k."""
    K, N, L = W.shape
    return W.transpose(2, 1, 0).reshape(L * N, K)


def round_cap(n, backup_only=False):
    """Hard cap on pivoting rounds of one problem of n unknowns (the device uses the same figure)."""
    return 50 * n + 50 if backup_only else 5 * n + 10


# ---- block principal pivoting ---------------------------------------------------------------------------------------------------
def nnls_bpp(G, C, tol=NNLS_TOL, backup_only=False, stats=None):
    """min_{x >= 0} |A x - b| for every column of C = A'B, G = A'A (n x n), by block principal pivoting.
    Returns (X, Y): X (n x m) >= 0, Y = G X - C off the passive set (zero on it)."""
    C = np.asarray(C, dtype=float)
    one = C.ndim == 1
    if one:
        C = C[:, None]
    n, m = C.shape
    P = np.zeros((n, m), dtype=bool)
    X = np.zeros((n, m))
    Y = -C.copy()
    ninf = np.full(m, n + 1)
    p = np.full(m, 3)
    rounds = np.zeros(m, dtype=np.int64)
    backup = np.zeros(m, dtype=bool)
    capped = np.zeros(m, dtype=bool)
    cap = round_cap(n, backup_only)
    rows = np.arange(n)[:, None]
    while True:
        V = np.where(P, X < -tol, Y < -tol)
        V[:, capped] = False
        nv = V.sum(axis=0)
        over = (nv > 0) & (rounds >= cap)
        if over.any():
            capped |= over
            V[:, over] = False
            nv = V.sum(axis=0)
        act = np.flatnonzero(nv > 0)
        if act.size == 0:
            break
        rounds[act] += 1
        na = nv[act]
        if backup_only:
            single = np.ones(act.size, dtype=bool)
        else:
            better = na < ninf[act]
            retry = ~better & (p[act] >= 1)
            single = ~better & ~retry
            ninf[act] = np.where(better, na, ninf[act])
            p[act] = np.where(better, 3, np.where(retry, p[act] - 1, p[act]))
        Va = V[:, act]
        if single.any():
            backup[act[single]] = True
            top = np.where(Va, rows, -1).max(axis=0)
            Va[:, single] = rows == top[single]
        P[:, act] ^= Va
        # x_P = G_PP^{-1} c_P, the columns grouped by passive set (what variant=:comb does)
        keys = np.packbits(P[:, act], axis=0).T
        _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        for g, f in enumerate(first):
            cols = act[inv == g]
            idx = np.flatnonzero(P[:, act[f]])
            X[:, cols] = 0.0
            if idx.size:
                X[np.ix_(idx, cols)] = np.linalg.solve(G[np.ix_(idx, idx)], C[np.ix_(idx, cols)])
        Ya = G @ X[:, act] - C[:, act]
        Ya[P[:, act]] = 0.0
        Y[:, act] = Ya
    if stats is not None:
        stats["exchanges"] = stats.get("exchanges", 0) + int(rounds.sum())
        stats["backup"] = stats.get("backup", 0) + int(backup.sum())
        stats["capped"] = stats.get("capped", 0) + int(capped.sum())
    X = np.where(P, np.maximum(X, 0.0), 0.0)
    return (X[:, 0], Y[:, 0]) if one else (X, Y)


def _bpp1(G, c, tol, backup_only, st):
    """nnls_bpp for one right-hand side, without the grouping machinery (the sequential H sweep calls it T times)."""
    n = c.shape[0]
    P = np.zeros(n, dtype=bool)
    x = np.zeros(n)
    y = -c
    ninf, p, rounds, cap = n + 1, 3, 0, round_cap(n, backup_only)
    used_backup = False
    while True:
        V = np.where(P, x < -tol, y < -tol)
        nv = int(np.count_nonzero(V))
        if nv == 0:
            break
        if rounds >= cap:
            st[2] += 1
            break
        rounds += 1
        if backup_only:
            single = True
        elif nv < ninf:
            ninf, p, single = nv, 3, False
        elif p >= 1:
            p, single = p - 1, False
        else:
            single = True
        if single:
            used_backup = True
            i = int(np.flatnonzero(V)[-1])
            P[i] = not P[i]
        else:
            P ^= V
        idx = np.flatnonzero(P)
        x = np.zeros(n)
        if idx.size:
            x[idx] = np.linalg.solve(G[np.ix_(idx, idx)], c[idx])
        y = G @ x - c
        y[P] = 0.0
    st[0] += rounds
    st[1] += used_backup
    return np.where(P, np.maximum(x, 0.0), 0.0), y


def near_degenerate(X, Y, C):
    """Entries whose side of the complementarity the solver's own numbers leave open (see the module docstring)."""
    cmax = np.abs(C).max(axis=0, keepdims=True)
    xmax = np.abs(X).max(axis=0, keepdims=True)
    return ((X == 0) & (np.abs(Y) < NEAR * cmax)) | ((X > 0) & (X < NEAR * xmax))


def _put(stats, st, near):
    if stats is not None:
        stats["exchanges"] = stats.get("exchanges", 0) + int(st[0])
        stats["backup"] = stats.get("backup", 0) + int(st[1])
        stats["capped"] = stats.get("capped", 0) + int(st[2])
        stats["near"] = near


# ---- W step (anls.jl:22-24, :47-57) ---------------------------------------------------------------------------------------------------
def w_normal_equations(data, H, L, mode="gram"):
    """G = Hstk*Hstk' (LK x LK) and C = Hstk*data' (LK x N)."""
    K, T = H.shape
    if mode == "literal":
        A, B = shift_and_stack(H, L).T, data.T  # t(H_unfold), t(data) (:52)
        return A.T @ A, A.T @ B
    G = np.zeros((L * K, L * K))
    C = np.zeros((L * K, data.shape[0]))
    for l in range(min(L, T)):
        C[l * K:(l + 1) * K] = H[:, :T - l] @ data[:, l:].T
        for lp in range(l + 1):
            blk = H[:, :T - l] @ H[:, l - lp:T - lp].T  # sum_t H[k, t-l] H[k', t-lp]
            G[l * K:(l + 1) * K, lp * K:(lp + 1) * K] = blk
            G[lp * K:(lp + 1) * K, l * K:(l + 1) * K] = blk.T
    return G, C


def update_motifs(data, H, L, mode="gram", tol=NNLS_TOL, backup_only=False, stats=None):
    """update_motifs!(rule::ANLSUpdate, data, W, H): W <- argmin_{W >= 0} |data - conv(W, H)|.  Returns W (K, N, L)."""
    K = H.shape[0]
    N = data.shape[0]
    G, C = w_normal_equations(data, H, L, mode)
    st = {}
    X, Y = nnls_bpp(G, C, tol, backup_only, st)
    _put(stats, (st["exchanges"], st["backup"], st["capped"]), fold_W(near_degenerate(X, Y, C), K, N, L))
    return fold_W(X, K, N, L)


# ---- H step (anls.jl:26-36, :63-137) --------------------------------------------------------------------------------------------------
def transconv(W, data):
    """B[k, t] = sum_n sum_{l, t+l < T} W[k, n, l] data[n, t+l]."""
    K, N, L = W.shape
    T = data.shape[1]
    B = np.zeros((K, T))
    for l in range(min(L, T)):
        B[:, :T - l] += W[:, :, l] @ data[:, l:]
    return B


def lag_grams(W):
    """A[Lt-1, e+L-1][k, k'] = sum_{l < Lt, 0 <= l-e < L} <W[k, :, l], W[k', :, l-e]> for Lt = 1..L, e = -(L-1)..L-1."""
    K, N, L = W.shape
    Wl = np.ascontiguousarray(W.transpose(2, 0, 1))  # (L, K, N)
    P = np.einsum("lkn,mjn->lmkj", Wl, Wl)  # P[l, l'][k, k']
    A = np.zeros((L, 2 * L - 1, K, K))
    for l in range(L):
        if l:
            A[l] = A[l - 1]
        for lp in range(L):
            A[l, l - lp + L - 1] += P[l, lp]
    return A


def _literal_column(resids, Wunf, W, H, t, tol, backup_only, st, near):
    """anls.jl:72-93 for one column (0-based t)."""
    K, N, L = W.shape
    T = H.shape[1]
    last = min(t + L, T)
    bs = last - t
    for k in range(K):  # :77-79
        resids[:, t:last] -= H[k, t] * W[k, :, :bs]
    U = Wunf[:bs * N]  # :81
    b = resids[:, t:last].reshape(-1, order="F")  # :82
    G, c = U.T @ U, U.T @ (-b)
    x, y = _bpp1(G, c, tol, backup_only, st)
    near[:, t] = near_degenerate(x[:, None], y[:, None], c[:, None])[:, 0]
    H[:, t] = x  # :85-87
    for k in range(K):  # :90-92
        resids[:, t:last] += H[k, t] * W[k, :, :bs]


def _gram_column(Hf, Bt, Acat, A0, t, L, tol, backup_only, st, near):
    """Hf: the padded H as (T + 2L-2, K) rows; row t + L-1 is column t."""
    c = Bt[t] - Acat @ Hf[t:t + 2 * L - 1].reshape(-1)
    x, y = _bpp1(A0, c, tol, backup_only, st)
    near[:, t] = near_degenerate(x[:, None], y[:, None], c[:, None])[:, 0]
    Hf[t + L - 1] = x


def _acat(A_Lt):
    """(2L-1, K, K) -> K x (2L-1)K with the e = 0 block zeroed: one product gives sum_{e != 0} A(e) H[:, t+e]."""
    nl, K, _ = A_Lt.shape
    A = A_Lt.copy()
    A[nl // 2] = 0.0
    return np.ascontiguousarray(A.transpose(1, 0, 2).reshape(K, nl * K))


def update_feature_maps(data, W, H, variant="basic", mode="gram", tol=NNLS_TOL, backup_only=False, stats=None):
    """update_feature_maps!(rule::ANLSUpdate, data, W, H; variant) -> (H, loss).  H is not modified; the new one is returned."""
    variant = str(variant).lstrip(":")
    if variant not in ("basic", "block"):
        raise ValueError(f"variant must be :basic or :block, got {variant!r}")
    K, N, L = W.shape
    T = data.shape[1]
    if variant == "block" and T < L:
        raise ValueError(f"variant=:block needs T >= L (anls.jl:136 indexes T-L+2:T); T = {T}, L = {L}")
    H = np.array(H, dtype=float)
    st = [0, 0, 0]
    near = np.zeros((K, T), dtype=bool)
    dnorm = np.linalg.norm(data)
    tail = range(T) if variant == "basic" else range(T - L + 1, T)
    if mode == "literal":
        resids = conv(W, H) - data  # :27
        Wunf = unfold_W(W)
        if variant == "block":
            for l in range(L):  # :105-134
                inds = np.arange(l, T - L + 1, L)
                if inds.size == 0:
                    continue
                for t in inds:  # :109-113
                    for k in range(K):
                        resids[:, t:t + L] -= H[k, t] * W[k]
                Bm = np.stack([resids[:, t:t + L].reshape(-1, order="F") for t in inds], axis=1)  # :117-121
                G, C = Wunf.T @ Wunf, Wunf.T @ (-Bm)
                s2 = {}
                X, Y = nnls_bpp(G, C, tol, backup_only, s2)  # :124-126
                st[0] += s2["exchanges"]; st[1] += s2["backup"]; st[2] += s2["capped"]
                near[:, inds] = near_degenerate(X, Y, C)
                H[:, inds] = X
                for t in inds:  # :129-133
                    for k in range(K):
                        resids[:, t:t + L] += H[k, t] * W[k]
        for t in tail:
            _literal_column(resids, Wunf, W, H, t, tol, backup_only, st, near)
        _put(stats, st, near)
        return H, np.linalg.norm(resids) / dnorm  # :35
    A = lag_grams(W)
    Bt = np.ascontiguousarray(transconv(W, data).T)
    Hf = np.zeros((T + 2 * L - 2, K))
    Hf[L - 1:L - 1 + T] = H.T
    acat = [_acat(A[i]) for i in range(L)]
    if variant == "block":
        win = np.arange(2 * L - 1)
        for l in range(L):
            inds = np.arange(l, T - L + 1, L)
            if inds.size == 0:
                continue
            C = (Bt[inds] - Hf[inds[:, None] + win].reshape(inds.size, -1) @ acat[L - 1].T).T
            s2 = {}
            X, Y = nnls_bpp(A[L - 1, L - 1], C, tol, backup_only, s2)
            st[0] += s2["exchanges"]; st[1] += s2["backup"]; st[2] += s2["capped"]
            near[:, inds] = near_degenerate(X, Y, C)
            Hf[inds + L - 1] = X.T
    for t in tail:
        Lt = min(L, T - t)
        _gram_column(Hf, Bt, acat[Lt - 1], A[Lt - 1, L - 1], t, L, tol, backup_only, st, near)
    H = np.ascontiguousarray(Hf[L - 1:L - 1 + T].T)
    _put(stats, st, near)
    return H, np.linalg.norm(conv(W, H) - data) / dnorm


def fit(data, W, H, iters, variant="basic", mode="gram", tol=NNLS_TOL):
    """The alternating loop of fit (alternating.jl): loss_hist[0] is the loss of the initial factors."""
    L = W.shape[2]
    hist = [np.linalg.norm(conv(W, H) - data) / np.linalg.norm(data)]
    for _ in range(iters):
        W = update_motifs(data, H, L, mode=mode, tol=tol)
        H, loss = update_feature_maps(data, W, H, variant=variant, mode=mode, tol=tol)
        hist.append(loss)
    return W, H, np.array(hist)


# ---- the shapes the tests, the fixture script and tools/anls_precision.py share -------------------------------------------------------
# name: (N, T, K, L, steps): steps "wh" = a W call then H calls from its result, "h" = H calls only from a random W (shapes
# with fewer columns than K*L unknowns, where the W problem is rank-deficient by construction); variants: the H variants run.
CASES = {
    "k4": (40, 600, 4, 7, "wh", ("basic", "block")),
    "k1": (16, 200, 1, 6, "wh", ("basic", "block")),
    "l1": (18, 250, 4, 1, "wh", ("basic", "block")),
    "kl128": (40, 1500, 4, 32, "wh", ("basic", "block")),
    "k33": (40, 400, 33, 3, "wh", ("basic", "block")),
    "t_lt_l": (12, 5, 2, 7, "h", ("basic",)),
    "t_eq_l": (10, 6, 2, 6, "h", ("basic", "block")),
    "t_prime": (14, 211, 3, 5, "wh", ("basic", "block")),
    "n1": (1, 300, 1, 6, "wh", ("basic", "block")),  # (the last column has N*1 equations: N >= K everywhere)
}
FIG = (250, 50000, 5, 20)  # figures/fast_bcd/synthetic_comparison.jl:58-67
EPS = np.finfo(float).eps


def problem(N, T, K, L, seed, noise=0.3, density=0.3):
    """Noisy sparse synthetic data (H not too sparse, noise in every entry: the passive-set Grams stay moderately
    conditioned) and random non-negative starting factors, as Fortran arrays."""
    rng = np.random.default_rng(seed)
    W = rng.random((K, N, L))
    H = rng.random((K, T)) * (rng.random((K, T)) < density)
    data = conv(W, H) + noise * rng.random((N, T))
    return np.asfortranarray(data), np.asfortranarray(rng.random((K, N, L))), np.asfortranarray(rng.random((K, T)))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def bar(floor, ceiling):
    """The bar on a GPU-vs-restatement difference: 1000 x the literal-vs-Gram difference of the same call (three decades for a
    third, unrelated summation order), where that difference counts as at least one ulp (two orders of summation that
    happen to agree bit for bit promise nothing about a third), and never looser than `ceiling`."""
    return min(ceiling, 1000.0 * max(floor, EPS))


def check_step(name, Xl, Xg, sl, sg, X12, tight):
    """What every committed shape must satisfy on the CPU (asserted by the tests and by make_golden_anls.py): the two modes
    agree to 1e-10 with identical zero patterns; no problem is capped; at most 1 % of the entries are near-degenerate by the
    restatement's own account; and tol = 1e-5 and tol = 1e-12 end on the same passive sets with values within `tight`.
    Returns the literal-vs-Gram floor."""
    floor = rel(Xl, Xg)
    assert floor <= 1e-10, (name, floor)
    assert np.array_equal(Xl > 0, Xg > 0), name
    assert sl["capped"] == 0 and sg["capped"] == 0, name
    assert sg["near"].sum() <= 0.01 * Xg.size, (name, int(sg["near"].sum()), Xg.size)
    assert np.array_equal(X12 > 0, Xg > 0), (name, "tol = 1e-12 ends on other passive sets")
    assert rel(X12, Xg) <= tight, (name, rel(X12, Xg))
    return floor
