"""seqNMF's re-centring of motifs on the GPU (cmf_recentre, cmf_mu_set_recentre, cmf_mu_recentre_info, fit_cnmf(shift=True)) against
tests/recentre_restatement.py.

Shapes (N, T, K, L), the smallest at which each thing can go wrong:
    (5, 7, 1, 1)        no-op
    (6, 9, 2, 12)       T < L: a shift can empty a row of H
    (130, 700, 3, 8)    few-component kernels, N across the 128 pad, T across 512
    (40, 600, 32, 5)    general kernels, one k block
    (33, 520, 33, 40)   second k block, second 32-lag block of Lp

ONE STEP, BIT FOR BIT.  W and H hold integers and the clamp floor only (recentre_restatement.exact_step_problem, hashed like
tests/exact_problems.py's), components carry shifts of both signs and both extremes, a zero shift, a dead component and an exactly integer
ratio: cmf_recentre followed by cmf_get_factors equals the restatement bitwise, the shifts equal cmf_recentre_shifts.
LAYOUTS AND PADDING.  After cmf_recentre a fit continued for 3 iterations is bitwise the fit of a fresh handle given the restated
shifted factors through cmf_set_factors, under each option setting that changes which kernels read W and H: that finds a padding row
written, a stale sk_Wj or G, or one of the two layouts of a factor missed.
WHOLE FITS four ways (call by call, cmf_iterate, cmf_fit, fit_cnmf(shift=True)) give the same bits, the shifts of the call-by-call loop
equal the restatement's step by step, and W, H, loss_hist match the fixtures tests/golden/mu_recentre_*.npz at the 1e-4 norm-wise bar.
"""
import ctypes
import os

import numpy as np
import pytest

import exact_problems as ep
import recentre_restatement as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 4
SHAPES = [(5, 7, 1, 1), (6, 9, 2, 12), (130, 700, 3, 8), (40, 600, 32, 5), (33, 520, 33, 40)]
BAR = 1e-4
_steps = {}


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def ids(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else None


def step_reference(shape):
    """(W, H, X, W', H', shifts) of the exact one-step problem, once per shape."""
    if shape not in _steps:
        N, T, K, L = shape
        W, H = rr.exact_step_problem(shape)
        X = ep.make_problem(N, T, K, L, "W")[2]
        W2, H2, s = rr.recentre(W, H)
        _steps[shape] = (W, H, X, np.asfortranarray(W2), np.asfortranarray(H2), s)
    return _steps[shape]


def make_rule(cmf, X, W, H, n_cu=None, **kw):
    if n_cu is None:
        return cmf.MultUpdate(X, W, H, **kw)
    old = {k: os.environ.get(k) for k in ("CMF_TEST_HOOKS", "CMF_TEST_N_CU")}
    os.environ["CMF_TEST_HOOKS"] = "1"
    os.environ["CMF_TEST_N_CU"] = str(n_cu)
    try:
        rule = cmf.MultUpdate(X, W, H, **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        assert rule.counter("plan:n_cu") == n_cu
    except BaseException:
        rule.close()
        raise
    return rule


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} of {a.size} entries differ, first {tuple(bad[0])}: {a[tuple(bad[0])]!r} against {b[tuple(bad[0])]!r}"


# ---- one step, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_step_equals_the_restatement_bitwise(cmf, shape):
    W, H, X, W2, H2, s = step_reference(shape)
    N, T, K, L = shape
    if L > 2 and K >= 2:
        assert s.max() == L // 2 - 1 and s.min() == L // 2 - L, "both extremes are there"
    if K >= 6:
        assert s[2] == 0 and s[3] == 0 and s[4] == L // 2 - 2 and W[3].max() == rr.EPS
    if L == 1:
        assert not s.any()
    rule = make_rule(cmf, X, W, H)
    try:
        before = rule.counter("recentre_launches")
        got = rule.recentre()
        assert rule.counter("recentre_launches") == before + 4
        assert got.dtype == np.int32 and np.array_equal(got, s)
        assert np.array_equal(got, cmf.recentre(W, H)[2]), "cmf_recentre_shifts"
        Wg, Hg = rule.download()
        same_bits(Wg, W2, "W")
        same_bits(Hg, H2, "H")
        last, moved = rule.recentre_info()
        assert np.array_equal(last, s) and np.array_equal(moved, np.abs(s))
        # a second step: the restatement's second step, and the totals add up
        W3, H3, s3 = rr.recentre(W2, H2)
        assert np.array_equal(rule.recentre(), s3)
        Wg, Hg = rule.download()
        same_bits(Wg, W3, "W after two steps")
        same_bits(Hg, H3, "H after two steps")
        assert np.array_equal(rule.recentre_info()[1], np.abs(s) + np.abs(s3))
    finally:
        rule.close()


# ---- layouts and padding -------------------------------------------------------------------------------------------------------------
def continuation_configs(shape):
    N, T, K, L = shape
    cfgs = [("default", {}), ("reuse_est0", dict(options={"reuse_est": 0})), ("speculate0", dict(options={"speculate": 0})),
            ("xortho", dict(xortho=0.01)), ("kl", dict(div=":kl")), ("mask", dict(mask=True)), ("cu1", dict(n_cu=1)), ("cu38", dict(n_cu=38))]
    if K <= 16:
        cfgs += [("small_k0", dict(options={"small_k": 0})), ("small_k_fuse0", dict(options={"small_k_fuse": 0})),
                 ("small_k2_fuse2", dict(options={"small_k": 2, "small_k_fuse": 2}))]
    if K % 32 == 0:
        cfgs += [("conv_kernel2", dict(options={"conv_kernel": 2})), ("conv_kernel3", dict(options={"conv_kernel": 3}))]
    return cfgs


def configure(rule, cfg, shape):
    for name, value in cfg.get("options", {}).items():
        rule.set_option(name, value)
    if cfg.get("mask"):
        rule.set_mask(ep.mu_mask(shape[0], shape[1]))
    if cfg.get("div"):
        rule.set_divergence(cfg["div"])
    if cfg.get("xortho"):
        rule.set_xortho(cfg["xortho"])


CONTINUATIONS = [(shape, name, cfg) for shape in SHAPES[1:] for name, cfg in continuation_configs(shape)
                 if shape in ((130, 700, 3, 8), (40, 600, 32, 5)) or name in ("default", "kl", "xortho")]


@pytest.mark.parametrize("shape,name,cfg", CONTINUATIONS, ids=[f"{ids(s)}-{n}" for s, n, _ in CONTINUATIONS])
def test_a_fit_continued_after_a_step_equals_the_fit_from_the_restated_factors(cmf, shape, name, cfg):
    W, H, X, _, _, _ = step_reference(shape)
    X = X + 1.0  # (strictly positive: every form takes it)
    # the handle that makes the step: one iteration first, so that every cache of the factors is warm (sk_Wj packed, G built, est
    # current, a contraction speculated); the factors it then holds are downloaded and restated on the host
    rule = make_rule(cmf, X, W, H, n_cu=cfg.get("n_cu"))
    try:
        configure(rule, cfg, shape)
        rule.iterate(1)
        W1, H1 = rule.download()
        W2, H2, s = rr.recentre(W1, H1)
        assert s.any()
        assert np.array_equal(rule.recentre(), s)
        moved = (rule.iterate(3),) + rule.download()
    finally:
        rule.close()
    rule = make_rule(cmf, X, np.asfortranarray(W2), np.asfortranarray(H2), n_cu=cfg.get("n_cu"))
    try:
        configure(rule, cfg, shape)
        fresh = (rule.iterate(3),) + rule.download()
    finally:
        rule.close()
    same_bits(moved[1], fresh[1], f"{name}: W")
    same_bits(moved[2], fresh[2], f"{name}: H")
    same_bits(moved[0], fresh[0], f"{name}: losses")


# ---- whole fits ----------------------------------------------------------------------------------------------------------------------
def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"mu_recentre_{name}.npz"))


def frob_rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("name", sorted(rr.FIXTURES))
def test_whole_fits_four_ways_and_against_the_restatement(cmf, name):
    g = golden(name)
    data, W0, H0, n_iter = rr.fixture_problem(name)
    assert n_iter == int(g["n_iter"]) and tuple(g["shape"]) == rr.FIXTURES[name][:4]
    K = W0.shape[0]
    runs = {}
    # call by call, cmf_mu_recentre_info read after every iteration
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        rule.set_recentre(True)
        losses, total = [rule.compute_loss()], np.zeros(K, dtype=np.int64)
        for it in range(n_iter):
            rule.update_motifs()
            losses.append(rule.update_feature_maps())
            last, moved = rule.recentre_info()
            total += np.abs(g["shifts"][it])
            assert np.array_equal(last, g["shifts"][it]), f"iteration {it}: shifts {last} against {g['shifts'][it]}"
            assert np.array_equal(moved, total)
        runs["calls"] = (np.asarray(losses),) + rule.download()
    finally:
        rule.close()
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        rule.set_recentre(True)
        first = rule.compute_loss()
        losses = rule.iterate(n_iter)
        last, moved = rule.recentre_info()
        assert np.array_equal(last, g["shifts"][-1]) and np.array_equal(moved, g["moved"])
        runs["iterate"] = (np.concatenate([[first], losses]),) + rule.download()
    finally:
        rule.close()
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        rule.set_recentre(True)
        lh, _, early = rule.fit_native(n_iter, np.inf, False, 3, 1e-4, False)
        last, moved = rule.recentre_info()
        assert not early and np.array_equal(last, g["shifts"][-1]) and np.array_equal(moved, g["moved"])
        runs["fit"] = (lh,) + rule.download()
    finally:
        rule.close()
    r = cmf.fit_cnmf(data, L=W0.shape[2], K=K, alg=":mult", max_itr=n_iter, W_init=W0, H_init=H0, check_convergence=False, shift=True)
    runs["fit_cnmf"] = (np.asarray(r.loss_hist), r.W, r.H)
    for way in ("iterate", "fit", "fit_cnmf"):
        for i, what in enumerate(("loss_hist", "W", "H")):
            same_bits(runs[way][i], runs["calls"][i], f"{way} against call by call: {what}")
    lh, Wg, Hg = runs["calls"]
    figures = (frob_rel(Wg, g["W"]), frob_rel(Hg, g["H"]), float(np.max(np.abs(lh - g["loss_hist"]) / np.abs(g["loss_hist"]))))
    print(name, "relW %.3e relH %.3e rel loss %.3e" % figures, "moved", g["moved"].tolist())
    assert max(figures) <= BAR, figures


# ---- no added contraction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 700, 3, 8), (40, 600, 32, 5)], ids=ids)
def test_the_step_adds_no_contraction_and_eval_mode_shifts_nothing(cmf, shape):
    W, H, X, _, _, _ = step_reference(shape)
    counts = {}
    for on in (0, 1):
        rule = cmf.MultUpdate(X + 1.0, W, H)
        try:
            rule.set_recentre(on)
            rule.iterate(5)
            counts[on] = {p: rule.counter("launches:" + p) for p in ep.LAUNCH_PATHS}
            counts[on]["recentre_launches"] = rule.counter("recentre_launches")
            if on:
                Wb = rule.download()[0]
                rule.iterate(3, eval_mode=True)
                assert rule.counter("recentre_launches") == counts[on]["recentre_launches"], "eval mode: no step"
                same_bits(rule.download()[0], Wb, "W under eval mode")
        finally:
            rule.close()
    assert counts[0].pop("recentre_launches") == 0 and counts[1].pop("recentre_launches") == 4 * 5
    assert counts[0] == counts[1], {p: (counts[0][p], counts[1][p]) for p in counts[0] if counts[0][p] != counts[1][p]}
    assert sum(counts[0].values()) > 0


# ---- behaviour -----------------------------------------------------------------------------------------------------------------------
def test_a_displaced_motif_comes_back_to_the_centre(cmf):
    data, W0, H0, n_iter = rr.behaviour_problem()
    L = W0.shape[2]
    final = {}
    for shift in (True, False):
        r = cmf.fit_cnmf(data, L=L, K=W0.shape[0], alg=":mult", max_itr=n_iter, W_init=W0, H_init=H0, check_convergence=False, shift=shift)
        final[shift] = (float(r.loss_hist[-1]), rr.centre_of_mass(r.W))
    print("loss with / without the step:", final[True][0], final[False][0], "centres of mass:", final[True][1], final[False][1])
    assert np.all(np.abs(final[True][1] - L // 2) <= 1.0), "the motif's centre of mass ends within one lag of the centre"
    assert final[True][0] < final[False][0], "and the fit that could use the whole window is the better one"


# ---- write-back ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 700, 3, 8), (40, 600, 32, 5)], ids=ids)
def test_an_armed_write_back_delivers_the_shifted_factors(cmf, shape):
    W, H, X, _, _, _ = step_reference(shape)
    X = X + 1.0
    plain = cmf.MultUpdate(X, W, H)
    try:
        plain.set_recentre(True)
        plain.update_motifs()
        plain.update_feature_maps()
        shifts = plain.recentre_info()[0]
        Wp, Hp = plain.download()
    finally:
        plain.close()
    assert shifts.any(), "the first iteration moves something"
    Wc, Hc = W.copy(order="F"), H.copy(order="F")
    rule = cmf.MultUpdate(X, Wc, Hc, sync_every_call=True)
    try:
        rule.set_recentre(True)
        rule.update_motifs(X, Wc, Hc)
        rule.update_feature_maps(X, Wc, Hc)
        assert rule.counter("writeback_overlapped") >= 1
        same_bits(Wc, Wp, "the caller's W")
        same_bits(Hc, Hp, "the caller's H")
        same_bits(rule.download()[0], Wp, "the resident W")
    finally:
        rule.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(cmf):
    lib = cmf.load_library()
    Wg, Hg, Xg, _, _, _ = step_reference((130, 700, 3, 8))
    group = cmf.MultUpdate(Xg, Wg, Hg, devices=[0, 0])  # a loopback cmf_create_multi group: two shards on one device
    try:
        for call in (lambda: group.set_recentre(True), lambda: group.recentre(), lambda: group.recentre_info()):
            with pytest.raises(cmf.CMFError, match="single-GPU handles only") as e:
                call()
            assert e.value.code == ERR_UNSUPPORTED
        group.iterate(1)  # (and the group goes on as before)
    finally:
        group.close()
    W, H, X, _, _, _ = step_reference((6, 9, 2, 12))
    rule = cmf.MultUpdate(X, W, H)
    try:
        for on in (2, -1):
            assert lib.cmf_mu_set_recentre(rule._h, on) == ERR_ARG and b"0 or 1" in lib.cmf_last_error()
        assert lib.cmf_mu_set_recentre(None, 1) == ERR_ARG and lib.cmf_recentre(None, None) == ERR_ARG
        assert lib.cmf_mu_recentre_info(None, None, None) == ERR_ARG
        assert lib.cmf_mu_recentre_info(rule._h, None, None) == 0 and lib.cmf_recentre(rule._h, None) == 0
        # the Gram forms, in both orders of installing
        rule.set_recentre(True)
        with pytest.raises(cmf.CMFError, match="Gram") as e:
            rule.set_option("gram", 1)
        assert e.value.code == ERR_UNSUPPORTED
        rule.set_recentre(False)
        rule.set_option("gram", 1)
        with pytest.raises(cmf.CMFError, match="Gram") as e:
            rule.set_recentre(True)
        assert e.value.code == ERR_UNSUPPORTED
        rule.set_option("gram", 0)
        rule.set_recentre(True)
        # state of the handle: it survives cmf_set_factors
        rule.upload(W, H)
        before = rule.counter("recentre_launches")
        rule.iterate(1)
        assert rule.counter("recentre_launches") == before + 4
    finally:
        rule.close()
    h = ctypes.c_void_p()
    Xf = np.asfortranarray(X)
    assert lib.cmf_create(ctypes.byref(h), 0, 6, 9, 2, 12, Xf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    try:
        assert lib.cmf_recentre(h, None) == ERR_STATE and b"factors not set" in lib.cmf_last_error()
    finally:
        lib.cmf_destroy(h)
