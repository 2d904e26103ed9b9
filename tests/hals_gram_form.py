"""TEST INFRASTRUCTURE: numpy statement of the Gram-projected HALS sweeps the GPU kernels implement
(cmf.jl_amd/csrc/cmf_kernels.h, "HALS rule").  tests/test_oracle.py checks it against the literal
residual-form restatement of src/algs/hals.jl in the oracle."""
import numpy as np


def w_sweep(o, W, H, data, l1, l2):
    """hals.jl:90-112 on G = resid * H_unfold' and HH = H_unfold * H_unfold'."""
    K, N, L = W.shape
    R = o.tensor_conv(W, H) - data
    Hu = o.shift_and_stack(H, L)  # row = l*K + k
    G = R @ Hu.T                  # (= denomW - numW of the MU path)
    HH = Hu @ Hu.T
    W = W.copy()
    for k in range(K):
        for l in range(L):
            j = l * K + k
            wo = W[k, :, l].copy()
            v = G[:, j] - wo * HH[j, j]
            wn = np.maximum((-v - l1) / (HH[j, j] + o.EPS + l2), 0.0)
            G += np.outer(wn - wo, HH[j])
            W[k, :, l] = wn
    return W


def h_sweep(o, W, H, data, l1, l2):
    """hals.jl:121-154 on P = transconv(W, resid) and the lag-Gram taps of W."""
    K, N, L = W.shape
    T = H.shape[1]
    R = o.tensor_conv(W, H) - data
    P = o.tensor_transconv(W, R)  # (= denomH - numH of the MU path)
    PW = np.einsum("knl,jnm->lmkj", W, W)  # PW[l, l', k, k'] = <W[k,:,l], W[k',:,l']>

    def taps(k, Lt):  # g[k', e+L-1] = sum_{l < Lt} PW[l, l-e, k, k']
        g = np.zeros((K, 2 * L - 1))
        for e in range(-(L - 1), L):
            for l in range(Lt):
                if 0 <= l - e < L:
                    g[:, e + L - 1] += PW[l, l - e, k, :]
        return g

    H = H.copy()
    for k in range(K):
        full = taps(k, L)
        D = np.zeros(T)
        gs = {}
        for t in range(T):
            Lt = min(L, T - t)
            g = full if Lt == L else gs.setdefault(t, taps(k, Lt))
            nrm = g[k, L - 1]
            ho = H[k, t]
            hn = max((ho * nrm - P[k, t] - l1) / (nrm + o.EPS + l2), 0.0)
            D[t] = hn - ho
            H[k, t] = hn
            for e in range(1, L):           # same row, later columns
                if t + e < T:
                    P[k, t + e] += D[t] * g[k, e + L - 1]
        for t in range(T):                   # later rows
            Lt = min(L, T - t)
            g = full if Lt == L else gs[t]
            for e in range(-(L - 1), L):
                if 0 <= t + e < T:
                    P[k + 1:, t + e] += D[t] * g[k + 1:, e + L - 1]
    return H


def h_sweep_pull_pipeline(o, W, H, data, l1, l2, block=8, seed=0):
    """The same H sweep in the form of the persistent pipeline (hals_h_persist_kernel): rows advance in blocks of
    `block` columns; before row k sweeps block b, the cross-row terms of that block are PULLED from the changes D of all
    rows above (one writer per block of P), which is allowed as soon as row k-1 has finished block b+1 (L-1 <= block);
    which eligible (row, block) runs next is drawn at random: any order the flags permit must give the same H."""
    K, N, L = W.shape
    T = H.shape[1]
    assert L - 1 <= block
    R = o.tensor_conv(W, H) - data
    P = o.tensor_transconv(W, R)
    PW = np.einsum("knl,jnm->lmkj", W, W)

    def taps(k, Lt):
        g = np.zeros((K, 2 * L - 1))
        for e in range(-(L - 1), L):
            for l in range(Lt):
                if 0 <= l - e < L:
                    g[:, e + L - 1] += PW[l, l - e, k, :]
        return g

    tap_cache = {}

    def tap(k, t):  # taps of source column t of row k: truncated window at the right edge (hals.jl:136)
        Lt = min(L, T - t)
        key = (k, Lt)
        if key not in tap_cache:
            tap_cache[key] = taps(k, Lt)
        return tap_cache[key]

    H = H.copy()
    D = np.zeros((K, T))
    nblk = -(-T // block)
    done = [0] * K      # blocks swept per row (the sweeper's progress flag)
    rng = np.random.default_rng(seed)
    while min(done) < nblk:
        ready = [k for k in range(K) if done[k] < nblk and (k == 0 or done[k - 1] >= min(done[k] + 2, nblk))]
        k = int(rng.choice(ready))
        b = done[k]
        t0, t1 = b * block, min((b + 1) * block, T)
        for k2 in range(k):  # the pull: sources of rows above within L-1 columns of the block, in row order
            for tp in range(t0, t1):
                for e in range(-(L - 1), L):
                    t = tp - e
                    if 0 <= t < T:
                        P[k, tp] += D[k2, t] * tap(k2, t)[k, e + L - 1]
        for t in range(t0, t1):  # the sweep of the block (same-row terms pushed ahead as before)
            g = tap(k, t)
            nrm = g[k, L - 1]
            ho = H[k, t]
            hn = max((ho * nrm - P[k, t] - l1) / (nrm + o.EPS + l2), 0.0)
            D[k, t] = hn - ho
            H[k, t] = hn
            for e in range(1, L):
                if t + e < T:
                    P[k, t + e] += D[k, t] * g[k, e + L - 1]
        done[k] += 1
    return H


def hh_from_lag_correlations(o, H, L):
    """HH = H_unfold * H_unfold' (hals.jl:56-60) the way compute_hh / hals_hh_kernel form it: from the lag correlations
    C[d][a][b] = sum_t H[a][t-d] * H[b][t] of H with itself, minus the terms the shift cuts off at the right end."""
    K, T = H.shape
    C = np.zeros((L, K, K))
    for d in range(L):
        C[d] = H[:, : T - d] @ H[:, d:].T if d < T else 0.0
    HH = np.zeros((L * K, L * K))
    for l in range(L):
        for lp in range(L):
            d = abs(l - lp)
            cut = min(l, lp)
            for k in range(K):
                for kp in range(K):
                    a, b = (k, kp) if l >= lp else (kp, k)  # a: the row with the larger lag
                    v = C[d][a][b] if d < T else 0.0
                    for u in range(max(T - cut, d), T):
                        v -= H[a, u - d] * H[b, u]
                    HH[l * K + k, lp * K + kp] = v
    return HH


# ---- the same sweeps with their intermediates kept (tests/exact_problems.py, HALS section) --------------------------------------
def conv_in(W, H, dtype):
    """tensor_conv(W, H) accumulated in `dtype`, lag by lag."""
    K, N, L = W.shape
    T = H.shape[1]
    Wd, Hd = W.astype(dtype), H.astype(dtype)
    est = np.zeros((N, T), dtype)
    for lag in range(min(L, T)):
        est[:, lag:] += Wd[:, :, lag].T @ Hd[:, : T - lag]
    return est


def loss_in(W, H, data, dtype):
    """norm(tensor_conv(W, H) - data) / norm(data) (hals.jl:41) with the conv, the residual and the 64 x 64 tile sums of its squares in
    `dtype`, the tile sums added in double: the model of the conv epilogue's loss."""
    r = conv_in(W, H, dtype) - data.astype(dtype)
    N, T = r.shape
    ss = 0.0
    for n0 in range(0, N, 64):
        for t0 in range(0, T, 64):
            tile = np.ascontiguousarray(r[n0:n0 + 64, t0:t0 + 64]).ravel()
            ss += float(np.sum(tile * tile, dtype=dtype))
    return float(np.sqrt(ss) / np.linalg.norm(data))


def w_half(o, W, H, data, l1, l2, dtype=np.float64, corrupt=None, eps=None):
    """w_sweep with its intermediates kept: a dict of R, G, HH (formed in fp64), and per element of W the value before its step (old),
    the value before the clamp (pre), scale = max(|pre|, |old|), the step's squared norm HH[j, j] (diag) and the updated value (new), all (K, N, L).  dtype: the type the sweep's
    state (G, HH, W, l1, l2, eps) is held and every operation of the recurrence is rounded in -- float64 is the reference (w_sweep bit
    for bit), float32 the model of a kernel.  eps: the o.EPS of the denominator (the mutation tests leave it out).
    corrupt(stage, arrays): "projections" once G and HH exist; "step" in front of every step with a dict of s, k, l, j, row (the row
    HH[j] that the step adds to G -- replace it to damage the update) and row_unit (None, or (n, row) for ONE unit's update)."""
    K, N, L = W.shape
    eps = o.EPS if eps is None else eps
    R = o.tensor_conv(W, H) - data
    Hu = o.shift_and_stack(H, L)
    a = dict(W=W, H=H, R=R, Hu=Hu, G=R @ Hu.T, HH=Hu @ Hu.T, dtype=dtype)
    if corrupt:
        corrupt("projections", a)
    G, HH, Ws = a["G"].astype(dtype), a["HH"].astype(dtype), W.astype(dtype)
    l1, l2, eps = dtype(l1), dtype(l2), dtype(eps)
    old, pre, diag = np.zeros(W.shape), np.zeros(W.shape), np.zeros(W.shape)
    s = 0
    for k in range(K):
        for l in range(L):
            j = l * K + k
            wo = Ws[k, :, l].copy()
            v = G[:, j] - wo * HH[j, j]
            with np.errstate(invalid="ignore", divide="ignore"):
                p = (-v - l1) / (HH[j, j] + eps + l2)
            wn = np.where(p > 0, p, dtype(0))  # (fmaxf: a NaN gives 0, and pre keeps it)
            step = dict(s=s, k=k, l=l, j=j, row=HH[j], row_unit=None)
            if corrupt:
                corrupt("step", step)
            upd = np.outer(wn - wo, step["row"])
            if step["row_unit"] is not None:
                n, row = step["row_unit"]
                upd[n] = (wn[n] - wo[n]) * row.astype(dtype)
            G += upd
            Ws[k, :, l] = wn
            old[k, :, l], pre[k, :, l], diag[k, :, l] = wo, p, HH[j, j]
            s += 1
    a.update(old=old, pre=pre, diag=diag, scale=np.maximum(np.abs(pre), np.abs(old)), new=Ws.astype(np.float64))
    return a


def lag_gram(W):
    """PW[l, k, l', k'] = <W[k, :, l], W[k', :, l']> as one matrix product."""
    K, N, L = W.shape
    Wm = np.ascontiguousarray(W.transpose(2, 0, 1)).reshape(L * K, N)
    return (Wm @ Wm.T).reshape(L, K, L, K)


def window_taps(PW, k):
    """taps[Lt - 1][k', e + L - 1] = sum_{l < Lt} PW[l, k, l - e, k'] for every window length Lt = 1 ... L (h_sweep's taps(k, Lt), the
    terms added in its order)."""
    L, K = PW.shape[:2]
    out = np.zeros((L, K, 2 * L - 1))
    for e in range(-(L - 1), L):
        ls = np.arange(max(0, e), min(L, L + e))
        c = np.zeros((L, K))
        c[ls] = PW[ls, k, ls - e, :]
        out[:, :, e + L - 1] = np.cumsum(c, axis=0)
    return out


def h_half(o, W, H, data, l1, l2, dtype=np.float64, corrupt=None, eps=None):
    """h_sweep with its intermediates kept: a dict of R, P (as it was before the sweep), PW (lag_gram), and per element of H old, pre,
    scale, diag (the window's squared norm) and new as in w_half, all (K, T), and loss: the loss after the update (loss_in, in dtype).  dtype, eps: as in w_half (float64:
    h_sweep bit for bit where the taps are exact).
    corrupt(stage, arrays): "projections" once P and PW exist; "row" in front of row k's sweep with a dict of k, Lt (the window length
    of every column, T entries: change one to take a truncated window at another length, its norm and its taps), skip_push (a set of
    (t, e): same-row terms D[t] g[k, e] never added to P[k, t + e]) and lose (a set of (k', t, e): cross-row terms D[t] g[k', e] of
    this row never added to P[k', t + e])."""
    K, N, L = W.shape
    T = H.shape[1]
    eps = o.EPS if eps is None else eps
    R = o.tensor_conv(W, H) - data
    a = dict(W=W, H=H, R=R, P=o.tensor_transconv(W, R), PW=lag_gram(W), dtype=dtype)
    if corrupt:
        corrupt("projections", a)
    P, Hs = a["P"].astype(dtype), H.astype(dtype)
    l1, l2, eps = dtype(l1), dtype(l2), dtype(eps)
    old, pre, diag = H.astype(np.float64), np.zeros(H.shape), np.zeros(H.shape)
    te0 = max(0, T - L + 1)
    for k in range(K):
        tap = window_taps(a["PW"], k).astype(dtype)
        row = dict(k=k, Lt=np.minimum(L, T - np.arange(T)), skip_push=set(), lose=set())
        if corrupt:
            corrupt("row", row)
        Lt, skip = row["Lt"], row["skip_push"]
        D = np.zeros(T, dtype)
        Pk, Hk = P[k], Hs[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            for t in range(T):
                g = tap[Lt[t] - 1, k]
                nrm, ho = g[L - 1], Hk[t]
                p = (ho * nrm - Pk[t] - l1) / (nrm + eps + l2)
                hn = p if p > 0 else dtype(0)
                d = hn - ho
                D[t], Hk[t], pre[k, t], diag[k, t] = d, hn, p, nrm
                n = min(L - 1, T - 1 - t)
                if n > 0:
                    push = d * g[L:L + n]
                    for (ts, e) in skip:
                        if ts == t and 1 <= e <= n:
                            push[e - 1] = 0
                    Pk[t + 1:t + 1 + n] += push
        if k + 1 < K:  # later rows: per target column the sources in ascending order, as h_sweep adds them
            full = tap[L - 1]
            tapE = tap[Lt[te0:] - 1]  # (ne, K, 2L - 1): the edge sources' own taps
            for e in range(L - 1, -L, -1):
                t_lo, t_hi = max(0, -e), min(T, T - e)
                if t_lo >= t_hi:
                    continue
                contrib = full[k + 1:, e + L - 1][:, None] * D[None, t_lo:t_hi]
                e_lo = max(t_lo, te0)
                if e_lo < t_hi:
                    contrib[:, e_lo - t_lo:] = tapE[e_lo - te0:t_hi - te0, k + 1:, e + L - 1].T * D[None, e_lo:t_hi]
                for (kt, ts, el) in row["lose"]:
                    if el == e and t_lo <= ts < t_hi:
                        contrib[kt - k - 1, ts - t_lo] = 0
                P[k + 1:, t_lo + e:t_hi + e] += contrib
    new = Hs.astype(np.float64)
    a.update(old=old, pre=pre, diag=diag, scale=np.maximum(np.abs(pre), np.abs(old)), new=new, P_after=P)
    a["loss"] = loss_in(W, Hs, data, dtype)
    return a
