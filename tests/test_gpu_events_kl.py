"""GPU tests of the KL form of the MU rule on event lists (cmf_events_*, EventKLUpdate, fit_cnmf on EventData) against the fixtures
tests/golden/mu_kl_*.npz and the event-form fp64 restatement tests/events_kl_restatement.py, at the project's bars:

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_kl_events_precision.txt (tools/mu_kl_events_precision.py: the restatement
with float32 gathered sums against its fp64 run; a count is admitted while that modelled drift stays within a third of the bar).  No
case is skipped or held to another bar.

Element by element (test_terms_bit_for_bit): on an integer problem every r_j is a power of two and every numerator a sum of small dyadic
numbers, exact in fp32 in ANY order, so cmf_events_terms must return float32(restatement) bit for bit under every chunking.  The
denominators are fp64 sums rounded once to fp32 (kl_den_w_kernel, kl_den_h_kernel): on integers they are exact too, and are held to
one fp32 rounding, 2^-23 relative.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import events_kl_restatement as er
import kl_mu_restatement as kr

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_k33", "mu_kl_k32", "mu_kl_short", "mu_kl_l40"]
UNREGULARISED = [n for n in FIXTURES if n != "mu_kl_small_reg"]
EPS = float(np.finfo(np.float64).eps)
SPARSE = er.PROBLEMS  # (name in profiles/mu_kl_events_precision.txt, generator, arguments, iterations, regularisers)
MEMORY = er.MEMORY_PROBLEM


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def admitted():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_kl_events_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


_loaded = {}


def load(name):
    """The fixture with its data as an event list (read once, shared, never written)."""
    if name not in _loaded:
        g = kr.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        g["ev"] = er.from_dense(g["data"])
        _loaded[name] = g
    g = _loaded[name]
    assert g["max_itr"] <= admitted()[name], f"{name} is fitted for more iterations than profiles/mu_kl_events_precision.txt admits"
    return g


_refs = {}


def sparse_case(name, gen, kw, iters, reg):
    """(events, W0, H0, the restatement's fit): computed once per problem."""
    if name not in _refs:
        ev, W0, H0 = gen(**kw)
        _refs[name] = (ev, W0, H0, er.fit_events(ev, W0, H0, max_itr=iters, **reg))
    assert iters <= admitted()[name], f"{name}: {iters} iterations are more than profiles/mu_kl_events_precision.txt admits"
    return _refs[name]


def events_of(cmf, ev):
    return cmf.EventData(ev[0], ev[1], ev[2], ev[3])


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def gpu_fit(cmf, ev, W0, H0, iters, reg=None, options=None, how="iterate", eval_mode=False):
    reg = reg or {}
    rule = cmf.EventKLUpdate(events_of(cmf, ev), W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        if how == "iterate":
            lh = [rule.compute_loss()] + list(rule.iterate(iters, eval_mode=eval_mode, **reg))
        else:  # call by call
            lh = [rule.compute_loss()]
            for _ in range(iters):
                if not eval_mode:
                    rule.update_motifs(l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
                lh.append(rule.update_feature_maps(l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0)))
        W, H = rule.download()
        return W, H, np.asarray(lh)
    finally:
        rule.close()


def check_against(got, ref, what=""):
    (Wg, Hg, lg), (Wr, Hr, lr) = got, ref
    print(what, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "max rel loss", float(np.max(np.abs(lg - lr) / lr)))
    np.testing.assert_allclose(lg, lr, rtol=REL_LOSS)
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS


@pytest.mark.parametrize("name", FIXTURES)
def test_single_calls(cmf, name):
    """compute_loss, one update_motifs!, one update_feature_maps!, the loss again, from the fixture's initial factors."""
    g = load(name)
    reg, data = g["reg"], g["data"]
    rule = cmf.EventKLUpdate(events_of(cmf, g["ev"]), g["W0"], g["H0"])
    try:
        l0 = rule.compute_loss()
        rule.update_motifs(l1W=reg["l1W"], l2W=reg["l2W"])
        Wg, _ = rule.download()
        Wc, Hc = np.zeros_like(Wg), np.zeros((Wg.shape[0], data.shape[1]), order="F")
        loss = rule.update_feature_maps(None, Wc, Hc, l1H=reg["l1H"], l2H=reg["l2H"])
        Wg2, Hg = rule.download()
        l1 = rule.compute_loss()
    finally:
        rule.close()
    Wr, Hr = g["W0"].copy(), g["H0"].copy()
    lr0 = kr.kl_loss(data, Wr, Hr)
    kr.update_motifs(data, Wr, Hr, l1W=reg["l1W"], l2W=reg["l2W"])
    relW = frob_rel(Wg, Wr)
    lr = kr.update_feature_maps(data, Wr, Hr, l1H=reg["l1H"], l2H=reg["l2H"])
    print(name, "relW", relW, "relH", frob_rel(Hg, Hr), "rel loss", abs(l0 - lr0) / lr0, abs(loss - lr) / lr)
    assert relW < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS
    np.testing.assert_array_equal(Wg, Wg2)
    np.testing.assert_array_equal(Wc, Wg2)  # update_feature_maps wrote both factors into the caller's arrays
    np.testing.assert_array_equal(Hc, Hg)
    assert abs(l0 - lr0) <= REL_LOSS * lr0 and abs(loss - lr) <= REL_LOSS * lr and abs(l1 - lr) <= REL_LOSS * lr
    assert l1 == loss  # (the same pass over the same factors)
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_fit_three_ways(cmf, name):
    """Call by call, cmf_events_iterate and fit_cnmf each meet the committed fixture (W, H, every loss_hist entry) and agree bit for bit."""
    g = load(name)
    ref = (g["W"], g["H"], g["loss_hist"])
    a = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], g["max_itr"], g["reg"], how="calls")
    check_against(a, ref, f"{name} calls")
    b = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], g["max_itr"], g["reg"], how="iterate")
    check_against(b, ref, f"{name} iterate")
    K, N, L = g["W0"].shape
    events = events_of(cmf, g["ev"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(events, L=L, K=K, alg=":mult", divergence=":kl", max_itr=g["max_itr"], check_convergence=False, W_init=g["W0"],
                           H_init=g["H0"], l1_W=g["reg"]["l1W"], l2_W=g["reg"]["l2W"], l1_H=g["reg"]["l1H"], l2_H=g["reg"]["l2H"])
    assert res.data is events and len(res.loss_hist) == g["max_itr"] + 1
    c = (res.W, res.H, res.loss_hist)
    check_against(c, ref, f"{name} fit_cnmf")
    for other in (b, c):
        for x, y in zip(a, other):
            np.testing.assert_array_equal(x, y)
    ev_loss = cmf.evaluate_divergence(res)
    assert abs(ev_loss - res.loss_hist[-1]) <= 1e-6 * res.loss_hist[-1], (ev_loss, res.loss_hist[-1])
    assert cmf.compute_loss(events, res.W, res.H) == ev_loss


def test_fit_cnmf_on_a_duck_typed_sparse_matrix_with_the_loop_options(cmf):
    g = load("mu_kl_k5")
    unit, time, count, shape = g["ev"]

    class Coo:
        row, col, data = unit, time, count

    Coo.shape = shape

    class Sparse:
        def tocoo(self):
            return Coo

    K, N, L = g["W0"].shape
    res = cmf.fit_cnmf(Sparse(), L=L, K=K, alg=":mult", divergence=":kl", max_itr=3, check_convergence=False, W_init=g["W0"], H_init=g["H0"],
                       options={"unit_chunk": 16})
    ref = er.fit_events(g["ev"], g["W0"], g["H0"], max_itr=3)
    check_against((res.W, res.H, res.loss_hist), ref, "tocoo")
    assert isinstance(res.data, cmf.EventData)
    # eval_mode through fit_cnmf: W stays what it was given, bit for bit; max_time = 0 stops after the first iteration (alternating.jl:45)
    res = cmf.fit_cnmf(Sparse(), L=L, K=K, alg=":mult", divergence=":kl", max_itr=3, check_convergence=False, W_init=g["W0"], H_init=g["H0"],
                       eval_mode=True)
    np.testing.assert_array_equal(res.W, np.asarray(g["W0"], dtype=np.float32).astype(np.float64))
    assert len(cmf.fit_cnmf(Sparse(), L=L, K=K, divergence=":kl", max_itr=50, max_time=0.0, seed=3).loss_hist) == 2
    # a seeded fit starts from init_rand_events
    W0, H0 = cmf.init_rand_events(Sparse(), L, K, seed=3)
    seeded = cmf.fit_cnmf(Sparse(), L=L, K=K, divergence=":kl", max_itr=1, check_convergence=False, seed=3)
    check_against((seeded.W, seeded.H, seeded.loss_hist), er.fit_events(g["ev"], W0, H0, max_itr=1), "seeded")
    # ... which takes the draws of init_rand for that seed: the two initialisations differ by one scalar
    Wd, Hd = cmf.init_rand(g["data"], L=L, K=K, seed=3)
    np.testing.assert_allclose(Wd / W0, (Wd / W0).flat[0], rtol=1e-12)
    np.testing.assert_allclose(Hd / H0, (Wd / W0).flat[0], rtol=1e-12)


@pytest.mark.parametrize("name,gen,kw,iters,reg", SPARSE, ids=[s[0] for s in SPARSE])
def test_sparse_problems(cmf, name, gen, kw, iters, reg):
    ev, W0, H0, ref = sparse_case(name, gen, kw, iters, reg)
    got = gpu_fit(cmf, ev, W0, H0, iters, reg)
    check_against(got, ref, name)
    assert all(np.isfinite(x).all() for x in got)
    if kw.get("skewed"):
        N = kw["N"]
        rule = cmf.EventKLUpdate(events_of(cmf, ev), W0, H0)
        assert rule.counter("unit_split") >= 1 and rule.counter("unit_chunk") < kw["T"]  # unit 1 holds more events than a chunk
        rule.close()
        for n in (0, N // 2, N - 1):
            assert np.all(got[0][:, n, :] == EPS)  # a unit without events: its motif entries fall to eps


def integer_case(cmf):
    """The integer problem, sized by the block sizes the handle reports (never hard-coded)."""
    probe = cmf.EventKLUpdate(cmf.EventData([0], [0], [1.0], (1, 1)), np.ones((1, 1, 1)), np.ones((1, 1)))
    ub, cb = probe.counter("w_block_units"), probe.counter("h_block_columns")
    defaults = (probe.counter("unit_chunk"), probe.counter("time_chunk"))
    probe.close()
    key = (ub, cb, defaults)
    if key not in _refs:
        N, T, K, L = ub + 6, max(300, 2 * defaults[0] + 44), 3, 6
        ev, W, H = er.integer_problem(N, T, K, L, seed=21, unit_block=ub, column_block=cb, chunks=(64, defaults[0]))
        r = er.ratio(ev, W, H)
        _refs[key] = (ev, W, H, r, er.num_W(ev, r, H, L), er.num_H(ev, r, W), kr.denom_W(H, N, L), kr.denom_H(W, T))
    return (ub, cb, defaults) + _refs[key]


@pytest.mark.parametrize("chunks", [None, (64, 64), (1, 1), (64, 1), (1, 64)])
def test_terms_bit_for_bit(cmf, chunks):
    ub, cb, defaults, ev, W, H, r, numW, numH, denW, denH = integer_case(cmf)
    unit, time, count, (N, T) = ev
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    # what the problem promises: powers of two, events on the first and the last column and either side of every block and chunk boundary
    assert np.all(np.isin(f32(r), (0.5, 1.0, 2.0, 4.0)))
    cols, units = set(time.tolist()), set(unit.tolist())
    assert {0, T - 1} <= cols and all({b - 1, b} <= cols for b in range(cb, T, cb)) and all({b - 1, b} <= units for b in range(ub, N, ub))
    per_unit = np.bincount(unit, minlength=N)
    assert per_unit.max() > max(64, defaults[0]) and per_unit.min() == 0
    rule = cmf.EventKLUpdate(events_of(cmf, ev), W, H)
    try:
        if chunks is not None:
            rule.set_option("unit_chunk", chunks[0])
            rule.set_option("time_chunk", chunks[1])
            assert rule.counter("unit_split") > 0 and rule.counter("time_split") > 0  # both split paths run
        else:
            assert rule.counter("unit_split") > 0  # (a unit with more events than the default chunk)
        uc = rule.counter("unit_chunk")
        assert per_unit.max() > uc  # events sit either side of a chunk boundary: the unit's list is cut after its uc-th event
        g_r, g_numW, g_numH, g_denW, g_denH = rule.terms()
    finally:
        rule.close()
    np.testing.assert_array_equal(g_r, f32(r))
    np.testing.assert_array_equal(g_numW, f32(numW))
    np.testing.assert_array_equal(g_numH, f32(numH))
    np.testing.assert_allclose(g_denW, denW, rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(g_denH, denH, rtol=2.0 ** -23, atol=0)


def test_results_do_not_depend_on_the_chunk_options_or_on_keep_ratio(cmf):
    """On the integer problem every gathered sum is exact, so update_motifs! and update_feature_maps! from the integer factors give
    bitwise the same W and H under every chunking (the loss is an fp64 sum of block sums, block by block: equal to 1e-13).
    keep_ratio = 0 recomputes the r_j the loss pass left, which changes nothing anywhere."""
    ev, W, H = integer_case(cmf)[3:6]

    def one_step(opts):
        rule = cmf.EventKLUpdate(events_of(cmf, ev), W, H)
        try:
            for k, v in opts.items():
                rule.set_option(k, v)
            rule.update_motifs()
            Wn, _ = rule.download()
            rule.upload(W, H)
            loss = rule.update_feature_maps()
            return Wn, rule.download()[1], loss
        finally:
            rule.close()

    base = one_step({})
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all() and base[2] > 0
    for opts in (dict(unit_chunk=64, time_chunk=64), dict(unit_chunk=1, time_chunk=1), dict(unit_chunk=7, time_chunk=5), dict(keep_ratio=0)):
        got = one_step(opts)
        np.testing.assert_array_equal(got[0], base[0])
        np.testing.assert_array_equal(got[1], base[1])
        assert abs(got[2] - base[2]) <= 1e-13 * base[2]
    g = load("mu_kl_k5")
    a = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], 4, how="calls")
    for how in ("calls", "iterate"):
        b = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], 4, options=dict(keep_ratio=0), how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    rule = cmf.EventKLUpdate(events_of(cmf, g["ev"]), g["W0"], g["H0"])
    rule.compute_loss()
    p0 = rule.counter("ratio_passes")
    rule.iterate(2)
    p1 = rule.counter("ratio_passes")
    rule.set_option("keep_ratio", 0)
    rule.iterate(2)
    assert p1 - p0 == 2 * 2 and rule.counter("ratio_passes") - p1 == 2 * 3  # (the pass update_motifs! saves)
    rule.close()


@pytest.mark.parametrize("name", ["mu_kl_k5", "mu_kl_k33"])
def test_two_runs_are_bitwise_equal(cmf, name):
    g = load(name)
    a = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], 5, g["reg"])
    b = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], 5, g["reg"])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    ev, W0, H0, _ = sparse_case(*SPARSE[0])
    a, b = gpu_fit(cmf, ev, W0, H0, 3), gpu_fit(cmf, ev, W0, H0, 3, how="calls")
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", UNREGULARISED)
def test_loss_hist_is_non_increasing(cmf, name):
    g = load(name)
    _, _, lh = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], g["max_itr"])
    steps = np.diff(lh)
    print(name, "largest relative step", float(np.max(steps / lh[:-1])))
    assert np.all(steps <= 1e-6 * lh[:-1])  # (fp32: a relative 1e-6)


@pytest.mark.parametrize("name", ["mu_kl_k5", "mu_kl_k32"])
def test_eval_mode_leaves_W_bitwise_unchanged(cmf, name):
    g = load(name)
    ref = er.fit_events(g["ev"], g["W0"], g["H0"], max_itr=3, eval_mode=True)
    W32 = np.asarray(g["W0"], dtype=np.float32).astype(np.float64)  # (what the device holds of W0)
    for how in ("iterate", "calls"):
        got = gpu_fit(cmf, g["ev"], g["W0"], g["H0"], 3, how=how, eval_mode=True)
        np.testing.assert_array_equal(got[0], W32)
        check_against(got, ref, f"{name} eval_mode {how}")


def test_memory_stays_far_below_one_dense_copy(cmf):
    name, gen, kw, iters, reg = MEMORY
    ev, W0, H0, ref = sparse_case(name, gen, kw, iters, reg)
    N, T = ev[3]
    assert (N, T) == (3000, 200000) and 9000 < ev[0].size <= 10000
    rule = cmf.EventKLUpdate(events_of(cmf, ev), W0, H0)
    try:
        lh = [rule.compute_loss()] + list(rule.iterate(iters))
        got = rule.download() + (np.asarray(lh),)
        used = rule.counter("device_bytes")
    finally:
        rule.close()
    print("device_bytes", used, "one dense fp32 copy", 4 * N * T)
    assert 0 < used < 0.1 * 4 * N * T
    check_against(got, ref, name)


def test_error_codes(cmf):
    """Every refusal returns its code with a message and leaves the handle (or the process) usable; none launches anything."""
    g = load("mu_kl_small")
    unit, time, count, (N, T) = g["ev"]
    K, _, L = g["W0"].shape
    lib = cmf.load_library()
    i32, pd = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    u32, t32, c64 = unit.astype(np.int32), time.astype(np.int32), count.astype(np.float64)

    def create(N_, T_, K_, L_, u, t, c, nnz=None):
        h = ctypes.c_void_p()
        rc = lib.cmf_events_create(ctypes.byref(h), 0, N_, T_, K_, L_, len(u) if nnz is None else nnz, u.ctypes.data_as(i32), t.ctypes.data_as(i32),
                                   c.ctypes.data_as(pd))
        return rc, h, lib.cmf_last_error().decode()

    def bad(field, j, value):
        u, t, c = u32.copy(), t32.copy(), c64.copy()
        {"unit": u, "time": t, "count": c}[field][j] = value
        return u, t, c

    cases = [(bad("unit", 5, N), 1, "outside"), (bad("unit", 0, -1), 1, "outside"), (bad("time", 9, T), 1, "outside"), (bad("time", 9, -2), 1, "outside"),
             (bad("count", 3, 0.0), 1, "finite and > 0"), (bad("count", 3, -2.0), 1, "finite and > 0"), (bad("count", 3, np.nan), 1, "finite and > 0"),
             (bad("count", 3, np.inf), 1, "finite and > 0"), ((u32[::-1].copy(), t32[::-1].copy(), c64), 1, "sorted"),
             ((np.repeat(u32[:1], 2), np.repeat(t32[:1], 2), c64[:2]), 1, "sorted")]
    for (u, t, c), code, word in cases:
        rc, h, msg = create(N, T, K, L, u, t, c)
        assert rc == code and word in msg and not h.value, (rc, msg)
    for dims in ((0, T, K, L), (N, 0, K, L), (N, T, 0, L), (N, T, K, 0)):
        rc, h, msg = create(*dims, u32, t32, c64)
        assert rc == 1 and "at least 1" in msg
    assert create(N, T, K, L, u32, t32, c64, nnz=0)[0] == 1
    h = ctypes.c_void_p()
    assert lib.cmf_events_create(ctypes.byref(h), 0, N, T, K, L, 5, None, t32.ctypes.data_as(i32), c64.ctypes.data_as(pd)) == 1
    assert lib.cmf_events_create(None, 0, N, T, K, L, len(u32), u32.ctypes.data_as(i32), t32.ctypes.data_as(i32), c64.ctypes.data_as(pd)) == 1
    rc, h, msg = create(N, T, 257, 1, u32, t32, c64)
    assert rc == 4 and "K <= 256" in msg
    rc, h, msg = create(N, T, 33, 65, u32, t32, c64)
    assert rc == 4 and "4096" in msg
    rc, h, msg = create(N, T, K, L, u32, t32, c64)
    assert rc == 0 and h.value
    launches = ctypes.c_int64()
    loss = ctypes.c_double()
    # before the factors are set every rule entry is a call-sequence error
    for call in (lambda: lib.cmf_events_update_motifs(h, 0.0, 0.0), lambda: lib.cmf_events_update_feature_maps(h, 0.0, 0.0, ctypes.byref(loss)),
                 lambda: lib.cmf_events_compute_loss(h, ctypes.byref(loss)), lambda: lib.cmf_events_iterate(h, 1, 0, 0.0, 0.0, 0.0, 0.0, None),
                 lambda: lib.cmf_events_get_factors(h, None, None), lambda: lib.cmf_events_terms(h, None, None, None, None, None)):
        assert call() == 3 and "cmf_events_set_factors" in lib.cmf_last_error().decode()
    assert lib.cmf_events_set_factors(h, None, None) == 1
    assert lib.cmf_events_get_counter(h, b"launches", ctypes.byref(launches)) == 0 and launches.value == 0  # nothing was launched by any refusal
    W0, H0 = np.asfortranarray(g["W0"]), np.asfortranarray(g["H0"])
    assert lib.cmf_events_set_factors(h, W0.ctypes.data_as(pd), H0.ctypes.data_as(pd)) == 0
    assert lib.cmf_events_get_counter(h, b"launches", ctypes.byref(launches)) == 0
    before = launches.value
    assert lib.cmf_events_set_option(h, b"no_such_option", 1) == 1 and "unknown option" in lib.cmf_last_error().decode()
    for name in (b"unit_chunk", b"time_chunk"):
        assert lib.cmf_events_set_option(h, name, 0) == 1 and "at least 1" in lib.cmf_last_error().decode()
    assert lib.cmf_events_set_option(h, b"keep_ratio", 2) == 1
    assert lib.cmf_events_get_counter(h, b"no_such_counter", ctypes.byref(launches)) == 1
    assert lib.cmf_events_iterate(h, -1, 0, 0.0, 0.0, 0.0, 0.0, None) == 1
    assert lib.cmf_events_compute_loss(h, None) == 1
    assert lib.cmf_events_get_counter(h, b"launches", ctypes.byref(launches)) == 0 and launches.value == before
    # ... and the handle works afterwards
    assert lib.cmf_events_compute_loss(h, ctypes.byref(loss)) == 0
    want = kr.kl_loss(g["data"], g["W0"], g["H0"])
    assert abs(loss.value - want) <= REL_LOSS * want
    assert lib.cmf_events_destroy(h) == 0
