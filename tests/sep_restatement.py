"""fp64 numpy restatement of the reference's separable ("LCS") fit (src/algs/separable.jl) on the HEAD layout: data (N, T),
W (K, N, L) with W[k, n, l] = V[n, groups[k][l]], H (K, T).  separable.jl itself is written for the old L x N x K layout of W and
is not included by src/CMF.jl; the arithmetic is restated statement by statement, not the indexing.  Indices are 0-based here.

Two modes of the same computation:
  - "literal": separable.jl as written -- the projector (I - w w'/|w|^2) formed and multiplied into the residual (:315), the
    sequential findsetmax (:403-419), svd for `pre` (:323-333), cosL on slices of the rows of G (:374-385).
  - "rewritten": what the GPU path does -- resid[:, t] -= w (w' resid[:, t] / |w|^2) with the column norms of the result;
    findsetmax from the strict prefix-maximum records (findsetmax_records); `pre` from the eigen-decomposition of X X';
    every cosine from the lagged products P[a, b, l] = sum_t G[a, t] G[b, t+l] and head[a, l] = |G[a, :T-l]| (shift_table).
Their difference on a given input is the floor of that input.

Every stage ends in a discrete decision, and every decision reports its margin (`margins`, a dict of lists):
  thresh     the least |col1 - thresh| / thresh over the columns (which columns are zeroed, :287-291)
  spa_out    per round: the least distance of a column norm OUTSIDE the band (anchor - sqrt(eps), anchor + sqrt(eps)] from the
             band's edges, relative to the anchor it was compared with (every comparison of the scan counts, also the ones
             against earlier anchors)
  spa_in     per round: for the columns INSIDE the band, the least (sqrt(eps) - |x - anchor|) / sqrt(eps): 1 for an exact copy
             of the anchor, 0 at the edge.  The band is 1.5e-8 wide, so "relative to the anchor" cannot reach 1e-6 for a
             column inside it; a column whose norm differs from the anchor's by rounding only sits at 1 - 1e-8, and that is
             what counts as margin for it (required: >= 0.5)
  spa_col2   per round with several members: relative gap between the two largest col2 among them
  pick       find_groups: relative gap between the `sims` of every pick and the best `sims` of a candidate that does not end
             up in the same group.  (Rows of one component are shifted copies of each other, so on noise-free data their
             similarities are all 1 up to rounding and which of them is picked first hangs on the last bits by construction;
             the pick order inside a group is erased by sort_group as long as its weights are distinct -- `sort` below.)
  sort       sort_group: the least gap between the sorted weights of a group (integers): >= 1 means no tie, so the order
             does not depend on the order the group was picked in
  eigengap   spectral: the least gap between consecutive eigenvalues from the largest down to the one below the K-th,
             relative to the largest
  orient     spectral: | |max v| - |min v| | / max|v| of every eigenvector used (the sign it is given)
  priority   spectral: gap between the L-th and the (L+1)-th priority of each group
  shift      arg_shift_max: relative gap between the winning cosine and the best cosine at any other shift, per pair
check_problem asserts all of them >= 1e-6 in both modes, identical decisions in both, and the NNLS conditions of
anls_restatement.check_step.

The NNLS solver is anls_restatement.nnls_bpp (block principal pivoting, standing for nonneg_lsq(V, data, alg=:pivot,
variant=:comb), :26).  The package's default `tol` is not known here; the restatement uses 1e-8 and check_problem shows that
1e-12 ends on the same passive sets (off the entries the solver itself calls near-degenerate), so no committed input depends
on it.
"""
import itertools

import numpy as np

import anls_restatement as A

EPS = np.finfo(float).eps
SQRT_EPS = EPS ** 0.5  # findsetmax's thresh (:403)
NNLS_TOL = 1e-8
MARGIN = 1e-6


def _note(margins, key, value):
    if margins is not None:
        margins.setdefault(key, []).append(float(value))


# ---- helpers (:340-391) ---------------------------------------------------------------------------------------------------------------
def colnorms(A_, p=2):
    """colnorms (:352)."""
    return np.abs(A_).sum(axis=0) if p == 1 else np.linalg.norm(A_, axis=0)


def diagscale(c):
    """The diagonal of diagscale (:389-391): c + (c < eps)."""
    return c + (c < EPS)


def row_normalize(H):
    """row_normalize (:422-424)."""
    return H * (1.0 / diagscale(np.abs(H).sum(axis=1)))[:, None]


def renormalize(V, G):
    """renormalize! (:340-348): the rows of G to l1-norm 1, the columns of V scaled back.  Returns new (V, G)."""
    d = diagscale(np.abs(G).sum(axis=1))
    return V * d[None, :], G * (1.0 / d)[:, None]


# ---- findsetmax (:403-419) ------------------------------------------------------------------------------------------------------------
def findsetmax(x, thresh=SQRT_EPS):
    """The sequential scan as written: the anchor `maxval` is the first member of the set, not its maximum."""
    maxval, members = x[0], [0]
    for i in range(1, len(x)):
        if x[i] > maxval + thresh:
            maxval, members = x[i], [i]
        elif x[i] > maxval - thresh:
            members.append(i)
    return maxval, members


def _anchor_walk(x, thresh):
    """The anchor can only move at a strict prefix-maximum record: the running maximum never exceeds anchor + thresh (a member
    is at most anchor + thresh, a larger element becomes the anchor), so an element that is not above every earlier one is not
    above anchor + thresh either.  Walks the records in order; returns the (index, value) of every anchor the scan has had."""
    x = np.asarray(x, dtype=float)
    pm = np.maximum.accumulate(x)
    rec = np.flatnonzero(x[1:] > pm[:-1]) + 1
    anchors = [(0, x[0])]
    for i in rec:
        if x[i] > anchors[-1][1] + thresh:
            anchors.append((int(i), x[i]))
    return anchors


def findsetmax_records(x, thresh=SQRT_EPS):
    """findsetmax in the parallel form the GPU uses: the final anchor (a, i_a) from the records, then the set is
    {i_a} u {i > i_a : x[i] > a - thresh}."""
    x = np.asarray(x, dtype=float)
    ia, a = _anchor_walk(x, thresh)[-1]
    return a, [ia] + (np.flatnonzero(x[ia + 1:] > a - thresh) + ia + 1).tolist()


def _band_margins(x, thresh, margins):
    """Margins of every comparison of the scan: element i against the anchor in force when the scan reaches it."""
    if margins is None:
        return
    x = np.asarray(x, dtype=float)
    anchors = _anchor_walk(x, thresh)
    if len(x) < 2:
        return
    before = np.empty_like(x)  # the anchor element i is compared with: elements (i_j, i_j+1] meet anchor j
    pos = [i for i, _ in anchors] + [len(x) - 1]
    for (i, a), nxt in zip(anchors, pos[1:]):
        before[i + 1:nxt + 1] = a
    d, before = np.abs(x - before)[1:], before[1:]  # (element 0 is compared with nothing)
    inside = d < thresh
    scale = np.maximum(np.abs(before), 1e-300)
    out = ((d - thresh) / scale)[~inside]
    _note(margins, "spa_out", out.min() if out.size else 1.0)
    _note(margins, "spa_in", ((thresh - d[inside]) / thresh).min() if inside.any() else 1.0)


# ---- SPA (:280-333) -------------------------------------------------------------------------------------------------------------------
def spa_scale(data, thresh=0):
    """:281-291: (X, col1, col2) -- the columns scaled to l1-norm 1 (data * inv(DX): a product with the reciprocal), the ones
    with col1 < thresh zeroed."""
    col1, col2 = colnorms(data, 1), colnorms(data, 2)
    X = data * (1.0 / diagscale(col1))[None, :]
    X[:, col1 < thresh] = 0.0
    return X, col1, col2


def orient(U):
    """SPA is invariant under the sign of a singular vector (a row of the projected matrix changes sign; norms, inner products
    and the projector do not).  The sign is fixed only so that two runs can be compared: the entry of largest magnitude of
    every column is made positive."""
    s = np.sign(U[np.abs(U).argmax(axis=0), np.arange(U.shape[1])])
    return U * np.where(s == 0, 1.0, s)[None, :]


def pre_projection(XXt, R, pre):
    """The R x N matrix `proj` with pre(X) = proj @ X, from the eigen-decomposition of X X' (rewritten mode and the GPU host):
    :svd -> U' (= Diagonal(S) * Vt), :svdcond -> S^-1 U' (= Vt)."""
    lam, U = np.linalg.eigh(XXt)
    lam, U = lam[::-1][:R], orient(U[:, ::-1][:, :R])
    if pre == "svd":
        return np.ascontiguousarray(U.T)
    if not (lam > 0).all():
        raise ValueError("pre=:svdcond needs R positive singular values")
    return U.T / np.sqrt(lam)[:, None]


def _pre_name(pre):
    name = pre.lstrip(":") if isinstance(pre, str) else pre
    if name not in (None, "svd", "svdcond"):
        raise ValueError(f"pre must be None, ':svd' or ':svdcond', got {pre!r}")
    return name


def spa(data, R, thresh=0, pre=None, mode="rewritten", margins=None):
    """SPA (:280-319) -> the sorted vertices (0-based)."""
    pre = _pre_name(pre)
    N, T = data.shape
    if not 1 <= R <= min(N, T):
        raise ValueError(f"SPA needs 1 <= R <= min(N, T) (R = {R}, N = {N}, T = {T})")
    X, col1, col2 = spa_scale(data, thresh)
    if thresh > 0:
        _note(margins, "thresh", np.abs(col1 - thresh).min() / thresh)
    if pre is not None:
        if mode == "literal":
            _, S, Vt = np.linalg.svd(X, full_matrices=False)  # :323-333
            X = Vt[:R] if pre == "svdcond" else S[:R, None] * Vt[:R]
        else:
            X = pre_projection(X @ X.T, R, pre) @ X
    resid = X
    vertices = []
    for _ in range(R):
        if mode == "literal":
            norms = colnorms(resid)
            _, jset = findsetmax(norms)
        else:
            norms = np.sqrt(np.einsum("nt,nt->t", resid, resid))
            _, jset = findsetmax_records(norms)
        _band_margins(norms, SQRT_EPS, margins)
        if len(jset) == 1:
            j = jset[0]
        else:  # break ties (:308-311): the first maximum of col2
            c = col2[jset]
            j = jset[int(np.argmax(c))]
            top = np.sort(c)[::-1]
            _note(margins, "spa_col2", (top[0] - top[1]) / top[0])
        vertices.append(int(j))
        w = resid[:, j].copy()
        wn2 = np.linalg.norm(w) ** 2
        if not wn2 > 0:
            raise ValueError("SPA: the residual vanished (the data has fewer than R independent columns)")
        if mode == "literal":
            resid = (np.eye(len(w)) - np.outer(w, w) / wn2) @ resid  # :315
        else:
            resid = resid - np.outer(w, (w @ resid) / wn2)
    return sorted(vertices)


# ---- step 2 (:23-27) ------------------------------------------------------------------------------------------------------------------
def nnls_step(data, vertices, mode="rewritten", tol=NNLS_TOL, stats=None):
    """V = data[:, vertices]; G = nonneg_lsq(V, data); renormalize!(V, G).  Returns (V, G); stats receives the solver's
    counters and `near` (anls_restatement.near_degenerate)."""
    V = np.array(data[:, vertices], dtype=float)
    if mode == "literal":
        Gram, C = V.T @ V, V.T @ data
    else:
        Gram, C = np.einsum("nr,ns->rs", V, V), np.einsum("nr,nt->rt", V, data)
    st = {}
    X, Y = A.nnls_bpp(Gram, C, tol, False, st)
    if stats is not None:
        stats.update(st)
        stats["near"] = A.near_degenerate(X, Y, C)
    return renormalize(V, X)


# ---- shift cosines (:364-385), the table the GPU builds ---------------------------------------------------------------------------------
def shift_table(G, L):
    """P[a, b, l] = sum_t G[a, t] G[b, t+l] and head[a, l] = |G[a, :T-l]| (summed directly, not as total minus tail)."""
    R, T = G.shape
    if L > T:
        raise ValueError(f"the shift cosines need L <= T (L = {L}, T = {T})")
    zero = np.flatnonzero(~(G != 0).any(axis=1))
    if zero.size:
        raise ValueError(f"row {int(zero[0])} of G is zero: its shift cosines are 0/0")
    P = np.empty((R, R, L))
    head = np.empty((R, L))
    for l in range(L):
        P[:, :, l] = G[:, :T - l] @ G[:, l:].T
        head[:, l] = np.sqrt(np.einsum("rt,rt->r", G[:, :T - l], G[:, :T - l]))
    return P, head


def _cos_ab(P, head, a, b):
    """(left, right)[l] = cosL(G[a], G[b], l, "a" / "b") from the table."""
    return P[a, b, :] / (head[a, :] * head[b, 0]), P[b, a, :] / (head[a, 0] * head[b, :])


def cosL(a, b, l, mode="both"):
    """cosL (:374-385) on slices."""
    n = len(a)
    if mode == "both":
        return max(cosL(a, b, l, "a"), cosL(a, b, l, "b"))
    if mode == "a":
        return a[:n - l] @ b[l:] / (np.linalg.norm(a[:n - l]) * np.linalg.norm(b))
    return a[l:] @ b[:n - l] / (np.linalg.norm(a) * np.linalg.norm(b[:n - l]))


def similarity(G, L, mode="rewritten", table=None):
    """dmat of shift_cluster (:144-150)."""
    R = G.shape[0]
    dmat = np.zeros((R, R))
    if mode == "literal":
        for r in range(R):
            for p in range(r, R):
                m = 0.0
                for l in range(L):  # shift_cos (:364-370)
                    m = max(m, cosL(G[r], G[p], l))
                dmat[r, p] = dmat[p, r] = m
        return dmat
    P, head = table if table is not None else shift_table(G, L)
    for r in range(R):
        for p in range(r, R):
            left, right = _cos_ab(P, head, r, p)
            dmat[r, p] = dmat[p, r] = max(0.0, left.max(), right.max())
    return dmat


# ---- grouping (:191-270) ----------------------------------------------------------------------------------------------------------------
def find_groups(dmat, K, L, margins=None):
    """find_groups (:191-211): pop! takes the LAST ungrouped row, findmax the first maximum."""
    groups = [[] for _ in range(K)]
    ungrouped = list(range(K * L))
    for k in range(K):
        groups[k].append(ungrouped.pop())
        picks = []
        while len(groups[k]) < L:
            sims = dmat[np.ix_(groups[k], ungrouped)].sum(axis=0)
            i = int(np.argmax(sims))
            picks.append((sims[i], list(ungrouped), sims))
            groups[k].append(ungrouped.pop(i))
        for best, cand, sims in picks:  # the margin of a pick: against the best candidate that never joins this group
            rest = [s for c, s in zip(cand, sims) if c not in groups[k]]
            if rest:
                _note(margins, "pick", (best - max(rest)) / abs(best))
    return groups


def find_groups_spectral(simat, K, L, margins=None):
    """find_groups_spectral (:214-270) with binarize=false."""
    R = K * L
    simat = np.maximum(0.0, simat - simat.sum() / R ** 2)
    lam, V = np.linalg.eigh(simat)  # ascending, as eigen of a symmetric matrix
    if R > 1:
        gaps = np.diff(lam)[max(R - K - 1, 0):]
        _note(margins, "eigengap", gaps.min() / abs(lam[-1]))
    free = np.ones(R, dtype=bool)
    groups = []
    for k in range(K):
        v = V[:, R - 1 - k].copy()
        _note(margins, "orient", abs(abs(v.max()) - abs(v.min())) / np.abs(v).max())
        if abs(v.max()) < abs(v.min()):
            v = -v  # reorient (:242-244)
        rows = np.flatnonzero(free)
        priority = rows[np.argsort(-v[rows], kind="stable")]
        if len(priority) > L:
            _note(margins, "priority", (v[priority[L - 1]] - v[priority[L]]) / np.abs(v).max())
        groups.append([int(r) for r in priority[:L]])
        free[priority[:L]] = False
    return groups


# ---- sort step (:96-131) ----------------------------------------------------------------------------------------------------------------
def arg_shift_max(left, right, margins=None):
    """arg_shift_max (:112-131) from the two lists of cosines: strict `>`, "a" before "b"."""
    arg, best = 0, 0.0
    for l in range(len(left)):
        if left[l] > best:
            best, arg = left[l], l
        if right[l] > best:
            best, arg = right[l], -l
    if margins is not None and best > 0:
        by_shift = {}
        for l in range(len(left)):
            by_shift[l] = max(by_shift.get(l, 0.0), left[l])
            by_shift[-l] = max(by_shift.get(-l, 0.0), right[l])
        other = max([v for s, v in by_shift.items() if s != arg], default=0.0)
        _note(margins, "shift", (best - other) / best)
    return arg


def sort_group(group, G, L, mode="rewritten", table=None, margins=None):
    """sort_group (:96-109): the rows of a group by descending summed arg-shift, a stable sort."""
    n = len(group)
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if mode == "literal":
                h1, h2 = G[group[i]], G[group[j]]
                left = [cosL(h1, h2, l, "a") for l in range(L)]
                right = [cosL(h1, h2, l, "b") for l in range(L)]
            else:
                left, right = _cos_ab(table[0], table[1], group[i], group[j])
            M[i, j] = arg_shift_max(left, right, margins)
    weight = M.sum(axis=1)
    if n > 1:
        _note(margins, "sort", np.diff(np.sort(weight)).min())
    return [group[i] for i in np.argsort(-weight, kind="stable")]


def construct_WH(V, G, groups):
    """construct_WH (:59-87) with average_H=true, as written: the divisor is min(T, t+L) - t + 1 in the reference's 1-based t,
    which is L + 1 (not L) away from the end of the recording and the number of terms only in the last L columns."""
    K, L = len(groups), len(groups[0])
    N, T = V.shape[0], G.shape[1]
    W = np.zeros((K, N, L))
    H = np.zeros((K, T))
    for k in range(K):
        W[k] = V[:, groups[k]]
        for l in range(L):
            H[k, :T - l] += G[groups[k][l], l:]
    t = np.arange(T)
    return W, H / (np.minimum(T, t + L + 1) - t)[None, :]


# ---- the fit (:14-56) -------------------------------------------------------------------------------------------------------------------
def fit(data, K, L, thresh=0, refit_H=False, refit_W=False, refit_H_itr=10, spectral=False, pre=None, mode="rewritten", tol=NNLS_TOL,
        margins=None, out=None):
    """Separable.fit -> (W, H).  `out` (a dict) receives every stage: vertices, V, G, near, P, head, dmat, groups, W0, H0 (the
    factors before the refits)."""
    data = np.asarray(data, dtype=float)
    R = K * L
    vertices = spa(data, R, thresh=thresh, pre=pre, mode=mode, margins=margins)
    st = {}
    V, G = nnls_step(data, vertices, mode=mode, tol=tol, stats=st)
    table = shift_table(G, L)
    dmat = similarity(G, L, mode=mode, table=table)
    groups = (find_groups_spectral if spectral else find_groups)(dmat, K, L, margins)
    groups = [sort_group(g, G, L, mode=mode, table=table, margins=margins) for g in groups]
    W, H = construct_WH(V, G, groups)
    if out is not None:
        out.update(vertices=vertices, V=V, G=G, near=st["near"], capped=st["capped"], P=table[0], head=table[1], dmat=dmat, groups=groups,
                   W0=W.copy(), H0=H.copy())
    if refit_W:  # :41-43
        W = A.update_motifs(data, H, L, mode="literal" if mode == "literal" else "gram")
    if refit_H:  # :46-52, the H sweep of the HALS rule with l1H = l2H = 0
        from oracle import cmf_oracle

        rule = cmf_oracle.HALSUpdate(data, W, H)
        for _ in range(refit_H_itr):
            cmf_oracle.hals_update_feature_maps(rule, data, W, H, 0.0, 0.0)
    return W, H


# ---- data and evaluation (datasets/sep.jl:4-39; :432-483) -------------------------------------------------------------------------------
def gen_sep_data(N, T, K, L, H_sparsity=0.75, rng=None):
    """gen_sep_data -> (data, W, H): random factors with two isolated events per component planted, so that every column of
    every motif occurs alone in some column of the data."""
    rng = np.random.default_rng(rng)
    if T < 3 * K * L:
        raise ValueError("T too small")
    W = 0.5 + rng.random((K, N, L))
    H = rng.random((K, T)) * (rng.random((K, T)) > H_sparsity)
    hL = L // 2
    free = np.ones(T - L, dtype=bool)
    for k in range(K):
        for down, up in ((-L, hL), (-hL, L)):  # left and right side of the sequence
            t = int(rng.choice(np.flatnonzero(free)))
            t1, t2 = max(0, t + down), min(T - 1, t + up)
            H[:, t1:t2 + 1] = 0.0
            H[k, t] = 0.5 + rng.random()
            free[t1:min(t2, T - L - 1) + 1] = False
    return A.conv(W, H), W, H


def cos_score(trueH, estH):
    """cos_score (:432-441)."""
    return float(np.mean([trueH[k] @ estH[k] / (np.linalg.norm(trueH[k]) * np.linalg.norm(estH[k])) for k in range(trueH.shape[0])]))


def permute_factors(trueH, estH):
    """permute_factors (:444-449): the permutation p maximising cos_score(estH[p], trueH), the first one on a tie."""
    perms = list(itertools.permutations(range(trueH.shape[0])))
    return list(perms[int(np.argmax([cos_score(estH[list(p)], trueH) for p in perms]))])


def is_separable(H, L):
    """is_separable (:452-483): does the block form of H contain a scaled permuted identity?"""
    K, T = H.shape
    G = np.zeros((K * L, T))
    for l in range(L):
        G[l * K:(l + 1) * K, l:] = H[:, :T - l]
    nz = G != 0
    alone = nz.sum(axis=0) == 1
    return bool(nz[:, alone].any(axis=1).all())


# ---- the condition on every committed input -----------------------------------------------------------------------------------------------
DECISIONS = ("thresh", "spa_out", "spa_col2", "pick", "sort", "eigengap", "orient", "priority", "shift")


def check_problem(name, data, K, L, noise_free=False, **kw):
    """What every committed input must satisfy on the CPU: both modes take the same decisions with every margin >= 1e-6
    (spa_in >= 0.5); no NNLS problem is capped; tol = 1e-8 and tol = 1e-12 end on the same passive sets off the near-degenerate
    entries, which are at most 1 % of G.  Returns (literal stages, rewritten stages, floors) with floors[x] = rel difference of
    stage x between the modes.

    The vertex columns are not counted in the 1 %: data[:, vertices[r]] IS column r of V, the residual of that problem is zero
    and all R - 1 zeros of its solution e_r have y = 0 up to rounding, whatever the seed (R (R-1) entries: 5.6 % of G at the
    reference's own test shape).
    noise_free: data that is exactly V G for the planted G has a zero residual at the solution, so y = (V'V x - V'data)_i is
    zero up to rounding for EVERY inactive i of every problem: the whole complement of the planted support is near-degenerate
    by construction and no seed can bring that under 1 %.  For such inputs the cap is not applied (the share is reported);
    the values of those entries are rounding noise and are held by the value bars like every other entry."""
    ml, mr, ol, orw, o12 = {}, {}, {}, {}, {}
    kw = {k: v for k, v in kw.items() if k not in ("refit_H", "refit_W", "refit_H_itr")}
    fit(data, K, L, mode="literal", margins=ml, out=ol, **kw)
    fit(data, K, L, mode="rewritten", margins=mr, out=orw, **kw)
    fit(data, K, L, mode="rewritten", tol=1e-12, out=o12, **kw)
    assert ol["vertices"] == orw["vertices"] == o12["vertices"], (name, "vertices")
    assert ol["groups"] == orw["groups"] == o12["groups"], (name, "groups", ol["groups"], orw["groups"])
    for m in (ml, mr):
        for key in DECISIONS:
            assert min(m.get(key, [1.0])) >= MARGIN, (name, key, min(m[key]))
        assert min(m.get("spa_in", [1.0])) >= 0.5, (name, "spa_in", min(m["spa_in"]))
    assert ol["capped"] == 0 and orw["capped"] == 0 and o12["capped"] == 0, name
    near = orw["near"] | ol["near"]
    others = np.setdiff1d(np.arange(near.shape[1]), orw["vertices"])
    if not noise_free:
        assert near[:, others].sum() <= 0.01 * near[:, others].size, (name, int(near[:, others].sum()), near[:, others].size)
    for o in (ol, o12):
        assert not (((o["G"] > 0) != (orw["G"] > 0)) & ~near).any(), (name, "passive sets differ off the near-degenerate entries")
    floors = {x: A.rel(ol[x], orw[x]) for x in ("V", "G", "W0", "H0")}
    floors["P"] = A.rel(shift_table(ol["G"], L)[0], orw["P"])
    for x, f in floors.items():
        assert f <= 1e-10, (name, x, f)
    assert A.rel(o12["G"], orw["G"]) <= A.bar(floors["G"], 1e-8), (name, "tol")
    return ol, orw, floors, {"literal": ml, "rewritten": mr}


# name: (N, T, K, L, noise_level, thresh, seed): the inputs the GPU tests, the fixture and the tools share.  thresh None = the rule of
# test/sep_test.jl:17 (0.2 N - noise_level) for noisy data and 0 for noise-free data.
CASES = {
    "ref_clean": (100, 250, 3, 5, 0.0, None, 1),
    "ref_noisy": (100, 250, 3, 5, 0.1, None, 1),
    "k1": (40, 120, 1, 6, 0.1, None, 1),
    "l1": (30, 120, 4, 1, 0.1, None, 1),
    "r128": (160, 1200, 4, 32, 0.1, None, 1),
    "t_prime": (60, 211, 3, 4, 0.1, None, 1),
}
FIG = (250, 50000, 5, 20)  # the figure shape (figures/sep)


def case_data(name):
    """(data, trueW, trueH, K, L, thresh) of a named case."""
    N, T, K, L, noise, thresh, seed = CASES[name] if name in CASES else name
    rng = np.random.default_rng(seed)
    data, W, H = gen_sep_data(N, T, K, L, rng=rng)
    if noise:
        data = data + noise * rng.random((N, T))  # sep_test.jl:14-15
    if thresh is None:
        thresh = 0.2 * N - noise if noise else 0.0
    return np.asfortranarray(data), W, H, K, L, thresh
