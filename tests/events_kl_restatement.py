"""The KL form of the MU rule on an event list, restated in fp64 numpy in EVENT form (the reference for tests/test_events_kl_cpu.py,
tests/test_gpu_events_kl.py and tools/mu_kl_events_precision.py).  No N x T array is ever formed.

tests/kl_mu_restatement.py stays the definition: a fit on the event list of `data` is the fit fit_kl(data, ...) describes, with the
sums over the data taken over its non-zero entries (tests/test_events_kl_cpu.py holds the two together at 1e-12).  An event list is
(unit, time, count): data[unit[j], time[j]] = count[j] > 0, sorted by (unit, time); with eps = eps(Float64),

    e_j = sum over l <= min(L-1, t_j), over k, of W[k, n_j, l] H[k, t_j - l] + eps;   r_j = x_j / e_j
    update_motifs!:        numW[k, n, l] = sum over the events of unit n with t_j >= l of r_j H[k, t_j - l];  denomW, the update: kl_mu_restatement
    update_feature_maps!:  r_j from the new W;  numH[k, t] = sum over the events with t <= t_j <= t + L - 1 of W[k, n_j, t_j - t] r_j
    loss = (sum_j x_j log(x_j / e_j) - sum_j x_j + sum_all e) / sum_j x_j
    sum_all e = sum_k sum_{l < min(L, T)} (sum_n W[k, n, l]) (sum_{t < T - l} H[k, t]) + N T eps       (sum_all_est)

Every gathered sum goes lag by lag through np.add.at.  `cdtype`: the number format of the gathered sums (est at the events, numW, numH),
as in kl_mu_restatement; float32 models the device (tools/mu_kl_events_precision.py).  Everything else stays fp64.
"""
import numpy as np

import kl_mu_restatement as kr

EPS = kr.EPS


def from_dense(data):
    """(unit, time, count, (N, T)) of the non-zero entries of `data`, sorted by (unit, time)."""
    data = np.asarray(data, dtype=np.float64)
    unit, time = np.nonzero(data)  # (row-major: sorted by (unit, time))
    return unit.astype(np.int64), time.astype(np.int64), data[unit, time], data.shape


def to_dense(ev):
    unit, time, count, shape = ev
    a = np.zeros(shape)
    a[unit, time] = count
    return a


def est_at_events(ev, W, H, cdtype=np.float64):
    """e_j without eps, in cdtype."""
    unit, time, _, (N, T) = ev
    K, _, L = W.shape
    Wc, Hc = W.astype(cdtype, copy=False), H.astype(cdtype, copy=False)
    e = np.zeros(unit.size, dtype=cdtype)
    for lag in range(min(L, T)):
        sel = np.nonzero(time >= lag)[0]
        e[sel] += np.einsum("kj,kj->j", Wc[:, unit[sel], lag], Hc[:, time[sel] - lag])
    return e


def ratio(ev, W, H, cdtype=np.float64):
    """r_j = x_j / (e_j + eps)."""
    return ev[2] / (est_at_events(ev, W, H, cdtype).astype(np.float64) + EPS)


def num_W(ev, r, H, L, cdtype=np.float64):
    unit, time, _, (N, T) = ev
    K = H.shape[0]
    Hc, rc = H.astype(cdtype, copy=False), r.astype(cdtype)
    out = np.zeros((L, N, K), dtype=cdtype)
    for lag in range(min(L, T)):
        sel = np.nonzero(time >= lag)[0]
        np.add.at(out[lag], unit[sel], (Hc[:, time[sel] - lag] * rc[sel]).T)
    return np.ascontiguousarray(out.transpose(2, 1, 0)).astype(np.float64)


def num_H(ev, r, W, cdtype=np.float64):
    unit, time, _, (N, T) = ev
    K, _, L = W.shape
    Wc, rc = W.astype(cdtype, copy=False), r.astype(cdtype)
    out = np.zeros((T, K), dtype=cdtype)
    for lag in range(min(L, T)):
        sel = np.nonzero(time >= lag)[0]
        np.add.at(out, time[sel] - lag, (Wc[:, unit[sel], lag] * rc[sel]).T)
    return np.ascontiguousarray(out.T).astype(np.float64)


def sum_all_est(W, H, N):
    """The sum of tensor_conv(W, H) + eps over ALL N x T entries, in closed form."""
    K, T = H.shape
    L = W.shape[2]
    wsum = np.sum(W, axis=1)  # K x L
    hcum = np.concatenate([np.zeros((K, 1)), np.cumsum(H, axis=1)], axis=1)  # hcum[k, m] = the sum of the first m columns
    lags = np.arange(min(L, T))
    return float(np.sum(wsum[:, lags] * hcum[:, T - lags])) + N * T * EPS


def kl_loss(ev, W, H, cdtype=np.float64):
    count, (N, T) = ev[2], ev[3]
    e = est_at_events(ev, W, H, cdtype).astype(np.float64) + EPS
    return (float(np.sum(count * np.log(count / e))) - float(np.sum(count)) + sum_all_est(W, H, N)) / float(np.sum(count))


def update_motifs(ev, W, H, l1W=0.0, l2W=0.0, cdtype=np.float64):
    K, N, L = W.shape
    numW = num_W(ev, ratio(ev, W, H, cdtype), H, L, cdtype)
    den = ((kr.denom_W(H, N, L) + l1W) + (2.0 * l2W) * W) + EPS  # mult.jl:37
    W *= numW / den
    np.maximum(W, EPS, out=W)  # :38
    return W


def update_feature_maps(ev, W, H, l1H=0.0, l2H=0.0, cdtype=np.float64):
    numH = num_H(ev, ratio(ev, W, H, cdtype), W, cdtype)  # (r from the new W)
    den = ((kr.denom_H(W, H.shape[1]) + l1H) + (2.0 * l2H) * H) + EPS  # :51
    H *= numH / den
    np.maximum(H, EPS, out=H)  # :52
    return kl_loss(ev, W, H, cdtype)


def fit_events(ev, W_init, H_init, max_itr=100, l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0, cdtype=np.float64, eval_mode=False):
    """(W, H, loss_hist) after exactly max_itr iterations (alternating.jl:16-71 without the stop tests)."""
    W = np.array(W_init, dtype=np.float64, copy=True)
    H = np.array(H_init, dtype=np.float64, copy=True)
    loss_hist = [kl_loss(ev, W, H, cdtype)]
    for _ in range(int(max_itr)):
        if not eval_mode:
            update_motifs(ev, W, H, l1W=l1W, l2W=l2W, cdtype=cdtype)
        loss_hist.append(update_feature_maps(ev, W, H, l1H=l1H, l2H=l2H, cdtype=cdtype))
    return W, H, np.asarray(loss_hist)


# --------------------------------------------------------------------------------------------------------------------------
# problems
# --------------------------------------------------------------------------------------------------------------------------
def _sorted_events(unit, time, count, shape):
    key = np.asarray(unit, dtype=np.int64) * shape[1] + np.asarray(time, dtype=np.int64)
    key, first = np.unique(key, return_index=True)
    return key // shape[1], key % shape[1], np.asarray(count, dtype=np.float64)[first], tuple(shape)


def _factors(rng, N, T, K, L):
    return rng.random((K, N, L)) + 0.1, rng.random((K, T)) + 0.1


def sparse_problem(N, T, K, L, density, seed, skewed=False):
    """Counts 1 .. 5 at about `density` of the entries.  skewed (needs N >= 5, T > 6 L): unit 1 has an event in EVERY column (more than
    any chunk), units 0, N // 2 and N - 1 have none, columns [T // 3, T // 3 + 3 L) and [T - 2 L, T - 1) are empty but for unit 1 --
    stretches longer than L --, and events sit at t = 0 and t = T - 1.  Returns (events, W0, H0)."""
    rng = np.random.default_rng(seed)
    nnz = max(1, int(round(density * N * T)))
    unit, time = rng.integers(0, N, nnz), rng.integers(0, T, nnz)
    if skewed:
        keep = ~np.isin(unit, (0, 1, N // 2, N - 1))
        keep &= ~((time >= T // 3) & (time < T // 3 + 3 * L)) & ~((time >= T - 2 * L) & (time < T - 1))
        unit, time = unit[keep], time[keep]
        unit = np.concatenate([unit, np.full(T, 1), [2, 2]])
        time = np.concatenate([time, np.arange(T), [0, T - 1]])
    count = rng.integers(1, 6, unit.size).astype(np.float64)
    ev = _sorted_events(unit, time, count, (N, T))
    return (ev,) + _factors(rng, N, T, K, L)


def scattered_problem(N, T, K, L, nnz, seed):
    """`nnz` events (before duplicates go) scattered over a large N x T: most units and columns hold none."""
    rng = np.random.default_rng(seed)
    ev = _sorted_events(rng.integers(0, N, nnz), rng.integers(0, T, nnz), rng.integers(1, 9, nnz).astype(np.float64), (N, T))
    return (ev,) + _factors(rng, N, T, K, L)


def integer_problem(N, T, K, L, seed, unit_block=64, column_block=8, chunks=(64,)):
    """Every term exactly representable: W and H hold 0 .. 3 (sparse), so est is a small integer; events lie where est > 0 with counts
    x_j = est_j 2^i, i in {-1, 0, 1, 2}: every r_j is a power of two (in fp32: est + eps rounds to est) and every numerator a sum of
    small dyadic numbers.  Unit 0 has an event wherever its est > 0 -- more than every chunk in `chunks` --, the first and the last
    column hold events, and so do the units and columns either side of every multiple of unit_block / column_block.
    Returns (events, W, H)."""
    rng = np.random.default_rng(seed)
    W = (rng.integers(0, 4, (K, N, L)) * (rng.random((K, N, L)) < 0.5)).astype(np.float64)
    H = (rng.integers(0, 4, (K, T)) * (rng.random((K, T)) < 0.4)).astype(np.float64)
    W[0, :, 0] = 1.0  # (est > 0 wherever H[0] > 0 ...
    H[0, ::2] = 1.0   # ... which is at least every other column, for every unit)
    H[0, [0, T - 1]] = 1.0
    H[0, [t for t in range(column_block - 1, T, column_block)]] = 1.0
    H[0, [t for t in range(column_block, T, column_block)]] = 1.0
    est = kr.tensor_conv(W, H)  # (a small dense array: this generator is for small shapes only)
    assert np.array_equal(est, np.round(est)) and est.max() < 2 ** 12
    pick = (rng.random((N, T)) < 0.3) & (est > 0)
    pick[0] = est[0] > 0
    edge_cols = sorted({0, T - 1} | {t for b in range(column_block, T, column_block) for t in (b - 1, b)})
    edge_units = sorted({0, N - 1} | {n for b in range(unit_block, N, unit_block) for n in (b - 1, b)})
    pick[:, edge_cols] |= est[:, edge_cols] > 0
    pick[edge_units, :] |= (est[edge_units, :] > 0) & (rng.random((len(edge_units), T)) < 0.6)
    pick[N // 2] = False  # (a unit without events)
    assert pick[0].sum() > max(chunks) and all(pick[:, t].any() for t in edge_cols) and all(pick[n].any() for n in edge_units if n != N // 2)
    unit, time = np.nonzero(pick)
    count = est[unit, time] * 2.0 ** rng.integers(-1, 3, unit.size)
    return (unit.astype(np.int64), time.astype(np.int64), count, (N, T)), W, H


# The sparse problems tests/test_gpu_events_kl.py fits and tools/mu_kl_events_precision.py admits: (name, generator, arguments, iterations,
# regularisers).  (1, 50, 1, 1) is regularised: one unit, one component and one lag fit ANY data exactly after one unregularised iteration,
# the loss is then 0 up to rounding and a relative bar on it says nothing; l1H and l2W keep the fixed point away from the exact fit.
# (9, 64, 16, 40) has 640 entries of W for 576 entries of data: at half density the loss after 20 iterations is still 7e-3; with a few
# events only the fit becomes exact and the loss a difference of nearly equal numbers.
PROBLEMS = [("skewed(40,4000,3,12)", sparse_problem, dict(N=40, T=4000, K=3, L=12, density=0.02, seed=11, skewed=True), 20, {}),
            ("sparse(1,50,1,1)", sparse_problem, dict(N=1, T=50, K=1, L=1, density=0.3, seed=12), 20, dict(l1H=0.5, l2W=0.1)),
            ("sparse(9,64,16,40)", sparse_problem, dict(N=9, T=64, K=16, L=40, density=0.5, seed=13), 20, {}),
            ("sparse(250,20000,5,20)", sparse_problem, dict(N=250, T=20000, K=5, L=20, density=0.01, seed=14), 5, {})]
MEMORY_PROBLEM = ("scattered(3000,200000,3,10)", scattered_problem, dict(N=3000, T=200000, K=3, L=10, nnz=10000, seed=15), 2, {})
