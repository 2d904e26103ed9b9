"""fp64 numpy restatement of the reference's ADMM rule (src/algs/admm.jl), line by line.

Two modes of the same computation:
  - "literal": forms what admm.jl forms -- the stacked Hstk (common.jl:133-142), wh / whc = conj(fft(W padded to T)) and one
    K x K Gram per frequency (precompute_solveH, admm.jl:229-247), the FFT solve of fastsolveH! (:249-272) and the
    FFT-based circular convolution of tesnor_circconv! (common.jl:36-50).  Small shapes only.
  - "rewritten": the exact rewritings the GPU path uses ("The ADMM rule"): no K x N x T tensor, the per-frequency
    Gram as the transform of 2L-1 lag matrices A(d), the right-hand side as one FFT of a circular transconv, only the
    frequencies 0..T//2 solved, the circular convolution as a direct sum.

`contract` (rewritten mode only) is applied to the result of every contraction (the Gram, Hstk*X, the convolutions and
transconvolutions): the identity by default; `np.float32`-rounding it models an fp32 contraction (profiles/admm_precision.txt).

Array conventions follow the package: data (N, T), W (K, N, L), H (K, T), all float64.
Every call returns (factor, loss_or_None, iters, reverts).
"""
import numpy as np
import scipy.linalg as sla


def _ident(x):
    return x


def conv(W, H):
    """tensor_conv (common.jl:21-32): est[n, t] = sum_l W[:, n, l]' H[:, t-l] (zero for t < l), as one product with the
    stacked H (common.jl:133-142) -- no N x T temporaries per lag, so that config 2's shape runs in seconds."""
    return stack_W(W).T @ shift_and_stack(H, W.shape[2])


def circconv(W, H):
    """Circular form: est[n, t] = sum_l W[:, n, l]' H[:, (t-l) mod T]."""
    return stack_W(W).T @ np.concatenate([np.roll(H, l, axis=1) for l in range(W.shape[2])])


def circtransconv(W, X):
    """y[k, s] = sum_n sum_l W[k, n, l] X[n, (s+l) mod T]: the L products W_l X at once, then the K x T rows shifted."""
    K, N, L = W.shape
    P = stack_W(W) @ X
    y = np.zeros((K, X.shape[1]))
    for l in range(L):
        y += np.roll(P[l * K:(l + 1) * K], -l, axis=1)
    return y


def shift_and_stack(H, L):
    """common.jl:133-142: row l*K+k holds H[k, t-l]."""
    K, T = H.shape
    S = np.zeros((L * K, T))
    for l in range(min(L, T)):
        S[l * K:(l + 1) * K, l:] = H[:, :T - l]
    return S


def fold_W(Z3, K, N, L):
    """admm.jl:114-120: W[k, n, l] = Z3[l*K+k, n]."""
    return np.ascontiguousarray(Z3.reshape(L, K, N).transpose(1, 2, 0))


def stack_W(W):
    K, N, L = W.shape
    return W.transpose(2, 0, 1).reshape(L * K, N)


def _w_gram(H, L, contract):
    """G = Hstk*Hstk' from lag correlations of the rows of H (no Hstk)."""
    K, T = H.shape
    G = np.zeros((L * K, L * K))
    for l in range(L):
        for lp in range(L):
            m = max(l, lp)
            if m >= T:
                continue
            # sum over t >= max(l, l') of H[:, t-l] H[:, t-l']'
            G[l * K:(l + 1) * K, lp * K:(lp + 1) * K] = H[:, m - l:T - l] @ H[:, m - lp:T - lp].T
    return contract(G)


def _w_rhs(H, X, L, contract):
    """Hstk * X for X (T, N): row l*K+k is sum_s H[k, s] X[s+l, :] (views of X, no shifted copies)."""
    K, T = H.shape
    out = np.zeros((L * K, X.shape[1]))
    for l in range(min(L, T)):
        out[l * K:(l + 1) * K] = H[:, :T - l] @ X[l:]
    return contract(out)


def update_motifs(data, H, L, rhow=10.0, maxiter=30, tol=1e-4, nonneg=True, mode="rewritten", contract=None, loss_trace=None,
                  stats=None):
    """update_motifs!(::ADMMUpdate) (admm.jl:24-121).  Reads H only; returns (W, None, iters, reverts).
    `stats` (a dict) receives "cond_G", "scaled_cols" (per iteration, the number of columns the w[n] >= 1 rule rescaled) and
    "Wstk" (the last primal iterate, which the reverts of Z3 do not touch)."""
    contract = contract or _ident
    N, T = data.shape
    K = H.shape[0]
    LK = L * K
    datanorm = np.linalg.norm(data)
    dataT = np.ascontiguousarray(data.T)
    Wstk = np.zeros((LK, N))
    Z1 = np.zeros((T, N))
    Z2 = np.zeros((LK, N))
    Z3 = np.zeros((LK, N))
    U1 = np.zeros((T, N))
    U2 = np.zeros((LK, N))
    U3 = np.zeros((LK, N))
    if mode == "literal":
        Hstk = shift_and_stack(H, L)
        G = Hstk @ Hstk.T + 2 * np.eye(LK)                      # :53
    else:
        G = _w_gram(H, L, contract) + 2 * np.eye(LK)
    fact = sla.cho_factor(G, lower=True)
    if stats is not None:
        stats["cond_G"] = np.linalg.cond(G)
        stats["scaled_cols"] = []

    if mode != "literal":
        Hstk = shift_and_stack(H, L)

    def est_of(Wcols):  # Hstk' * Wstk = conv(fold(Wstk), H)', (T, N)
        if mode == "literal":
            return Hstk.T @ Wcols
        return contract(Hstk.T @ Wcols)

    loss_hist, iters, reverts = [], 0, 0
    c1, c2 = 1 / (1 + 1 / rhow), 1 / rhow
    for _ in range(maxiter):
        iters += 1
        rhs = (Hstk @ (Z1 - U1)) if mode == "literal" else _w_rhs(H, Z1 - U1, L, contract)   # :63
        Wstk = sla.cho_solve(fact, rhs + Z2 - U2 + Z3 - U3)     # :65
        estT = est_of(Wstk)                                     # :68
        Z1 = c1 * ((estT + U1) + c2 * dataT)                    # :69
        V2 = Wstk + U2                                          # :72-78
        w = np.sum(V2 ** 2, axis=0)
        big = w >= 1
        if stats is not None:
            stats["scaled_cols"].append(int(big.sum()))
        Z2 = Z2.copy()
        Z2[:, big] = V2[:, big] / np.sqrt(w[big])
        Z3_last = Z3                                            # :81-86
        Z3 = np.maximum(0, Wstk + U3) if nonneg else Wstk + U3
        U1 = U1 + (estT - Z1)                                   # :89-91
        U2 = U2 + (Wstk - Z2)
        U3 = U3 + (Wstk - Z3)
        loss_hist.append(np.linalg.norm(dataT - est_of(Z3)) / datanorm)   # :93-96
        if loss_trace is not None:
            loss_trace.append(loss_hist[-1])
        if len(loss_hist) > 1:                                  # :99-107
            diff = loss_hist[-2] - loss_hist[-1]
            if diff < 0:
                Z3 = Z3_last
                loss_hist.pop()
                reverts += 1
            if diff < tol:
                break
    if stats is not None:
        stats["Wstk"] = Wstk
    return fold_W(Z3, K, N, L), None, iters, reverts


def _h_grams_literal(W, T):
    """precompute_solveH(W, 1, T) (admm.jl:229-247): whc and the T factorised Grams."""
    K, N, L = W.shape
    wh = np.zeros((K, N, T), dtype=complex)
    wh[:, :, :L] = W
    wh = np.fft.fft(wh, axis=2)
    whc = np.conj(wh)
    facts = [sla.cho_factor(whc[:, :, t] @ whc[:, :, t].conj().T + 2 * np.eye(K), lower=True) for t in range(T)]
    return whc, facts


def lag_grams(W):
    """A[d + L-1][k, k'] = sum_n sum_{l - l' = d} W[k, n, l] W[k', n, l'] for d = -(L-1) .. L-1."""
    K, N, L = W.shape
    A = np.zeros((2 * L - 1, K, K))
    for l in range(L):
        for lp in range(L):
            A[l - lp + L - 1] += W[:, :, l] @ W[:, :, lp].T
    return A


def _h_grams_rewritten(W, T, contract):
    """Gram_t = sum_d A(d) exp(+2 pi i t d / T) + 2I for t = 0..T//2 (covers T < 2L-1, where lags alias)."""
    K, N, L = W.shape
    A = contract(lag_grams(W))
    F = T // 2 + 1
    d = np.arange(-(L - 1), L)
    t = np.arange(F)
    ph = np.exp(2j * np.pi * ((np.outer(t, d) % T) / T))      # (F, 2L-1), angle from (t*d mod T) in integers
    Gr = np.einsum("fd,dij->fij", ph, A) + 2 * np.eye(K)[None]
    return np.linalg.cholesky(Gr)  # (F, K, K), lower: Gram_f = L_f L_f^H


def update_feature_maps(data, W, rhoh=10.0, maxiter=30, l1H=0.0, tol=1e-4, nonneg=True, mode="rewritten", contract=None,
                        loss_trace=None):
    """update_feature_maps!(::ADMMUpdate) (admm.jl:124-226).  Reads W only; returns (H, loss, iters, reverts)."""
    contract = contract or _ident
    data = np.ascontiguousarray(data)
    N, T = data.shape
    K, _, L = W.shape
    assert T >= L
    datanorm = np.linalg.norm(data)
    est = np.zeros((N, T))
    Z1 = np.zeros((N, T))
    Z2 = np.zeros((K, T))
    Z3 = np.zeros((K, T))
    Q1 = np.zeros((N, T))
    Q2 = np.zeros((K, T))
    Q3 = np.zeros((K, T))
    if mode == "literal":
        whc, facts = _h_grams_literal(W, T)
    else:
        facts = _h_grams_rewritten(W, T, contract)
    F = T // 2 + 1

    def solve(B, V1, V2):
        if mode == "literal":  # fastsolveH! (:249-272)
            bh, v1h, v2h = np.fft.fft(B, axis=1), np.fft.fft(V1, axis=1), np.fft.fft(V2, axis=1)
            hh = np.zeros((K, T), dtype=complex)
            for t in range(T):
                beta = whc[:, :, t] @ bh[:, t] + (v1h[:, t] + v2h[:, t])
                hh[:, t] = sla.cho_solve(facts[t], beta)
            return np.real(np.fft.ifft(hh, axis=1))
        r = np.fft.fft(contract(circtransconv(W, B)) + V1 + V2, axis=1)
        hh = np.zeros((K, T), dtype=complex)
        y = np.linalg.solve(facts, r[:, :F].T[:, :, None])                              # L_f y = r_f
        hh[:, :F] = np.linalg.solve(np.conj(np.swapaxes(facts, 1, 2)), y)[:, :, 0].T   # L_f^H h = y
        hh[:, T - np.arange(1, T - F + 1)] = np.conj(hh[:, 1:T - F + 1])
        return np.real(np.fft.ifft(hh, axis=1))

    def circ_est(Hc):
        if mode == "literal":  # tesnor_circconv! (common.jl:36-50)
            hh = np.fft.fft(Hc, axis=1)
            esth = np.einsum("knt,kt->nt", np.conj(whc), hh)
            return np.real(np.fft.ifft(esth, axis=1))
        return contract(circconv(W, Hc))

    lin = (lambda Hc: conv(W, Hc)) if mode == "literal" else (lambda Hc: contract(conv(W, Hc)))
    loss_hist, iters, reverts = [], 0, 0
    c1, c2 = 1 / (1 + 1 / rhoh), 1 / rhoh
    for _ in range(maxiter):
        iters += 1
        H = solve(Z1 - Q1, Z2 - Q2, Z3 - Q3)                    # :180-182
        est = circ_est(H)                                       # :185
        Z1 = c1 * ((est + Q1) + c2 * data)                      # :186
        V = H + Q2                                              # :189
        Z2 = np.sign(V) * np.maximum(0, np.abs(V) - l1H / rhoh)
        Z3_last = Z3                                            # :192-197
        Z3 = np.maximum(0, H + Q3) if nonneg else H + Q3
        loss_hist.append(np.linalg.norm(lin(Z3) - data) / datanorm)   # :199-200
        if loss_trace is not None:
            loss_trace.append(loss_hist[-1])
        if len(loss_hist) > 1:                                  # :203-211
            diff = loss_hist[-2] - loss_hist[-1]
            if diff < 0:
                Z3 = Z3_last
                loss_hist.pop()
                reverts += 1
            if diff < tol:
                break
        Q1 = Q1 + (est - Z1)                                    # :214-216
        Q2 = Q2 + (H - Z2)
        Q3 = Q3 + (H - Z3)
    H = Z3                                                      # :219
    return H, np.linalg.norm(lin(H) - data) / datanorm, iters, reverts


def decision_margins(trace, tol):
    """Smallest |diff - tol| and |diff| over the decisions one call's loss trace implies (`trace` holds every loss pushed,
    including reverted ones, in order).  Replays the pop rule of admm.jl:99-107 / :203-211."""
    hist, m_tol, m_zero = [], np.inf, np.inf
    for x in trace:
        hist.append(x)
        if len(hist) > 1:
            diff = hist[-2] - hist[-1]
            m_tol, m_zero = min(m_tol, abs(diff - tol)), min(m_zero, abs(diff))
            if diff < 0:
                hist.pop()
    return m_tol, m_zero


def fit(data, W0, H0, max_itr, **kw):
    """The reference's fit loop (alternating.jl:44-67) with this rule, no convergence check; returns (W, H, loss_hist, counts)
    where counts lists (W iters, W reverts, H iters, H reverts) per outer iteration.  loss_hist[0] is the initial loss."""
    W, H = np.array(W0, dtype=float), np.array(H0, dtype=float)
    L = W.shape[2]
    wkw = {k: kw[k] for k in ("rhow", "tol", "nonneg", "mode", "contract") if k in kw}
    hkw = {k: kw[k] for k in ("rhoh", "l1H", "tol", "nonneg", "mode", "contract") if k in kw}
    loss_hist = [np.linalg.norm(conv(W, H) - data) / np.linalg.norm(data)]
    counts = []
    for _ in range(max_itr):
        W, _, wi, wr = update_motifs(data, H, L, maxiter=kw.get("admm_W_maxiter", 30), **wkw)
        H, loss, hi, hr = update_feature_maps(data, W, maxiter=kw.get("admm_H_maxiter", 30), **hkw)
        loss_hist.append(loss)
        counts.append((wi, wr, hi, hr))
    return W, H, np.array(loss_hist), counts
