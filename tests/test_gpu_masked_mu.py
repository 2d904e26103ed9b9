"""GPU tests of the MU rule under a mask (cmf_mu_set_mask, cmf_masked_loss, fit_cnmf(mask=), cross_validate) against the fp64
restatement tests/masked_mu_restatement.py, at the project's bars (tests/test_gpu_parity.py):

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist
    REL_PRIM    = 2e-6   one masked conv (here: its norm over the observed / the held-out entries, through cmf_masked_loss)

FIT_ITERS: how long a masked fit is compared under the 1e-4 bar.  tools/mu_masked_precision.py reran the restatement with float32
contractions on the shapes and masks below; profiles/mu_masked_precision.txt holds the distances from the fp64 run, and FIT_ITERS is
the largest count at which the worst of them stays below a quarter of the bar: 20.  What limits it is one case, (6, 3, 2, 5) under
50 % speckle without regularisers -- T < L, 9 observed entries, 42 unknowns: the loss itself falls towards 0 (1e-3 by iteration 30)
and its RELATIVE error is what grows (5.7e-6 at 20, 7.5e-5 at 30).  Every other case stays below 2.7e-6 through 100 iterations, so
the two shapes people sweep are also fitted for LONG_FIT_ITERS = 100 (their rows of the table: 2.7e-6 and 1.5e-6 at 100).
"""
import os

import numpy as np
import pytest

import masked_mu_restatement as mr

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
REL_PRIM = 2e-6
FIT_ITERS = 20
LONG_FIT_ITERS = 100
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)
SHAPES = [(48, 300, 4, 8), (130, 700, 32, 20), (37, 150, 33, 7), (20, 200, 6, 40), (6, 3, 2, 5), (250, 2000, 5, 20)]


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def rand_problem(seed, N, T, K, L):
    rng = np.random.default_rng(seed)
    return rng.random((K, N, L)), rng.random((K, T)), rng.random((N, T))


def make_mask(kind, N, T, L):
    if kind == "blocks":
        m = mr.block_mask(N, T, 0.2, min(L, T), 11)
    elif kind == "speckle":
        m = mr.block_mask(N, T, 0.5, 1, 12)
    else:  # one unit and one sample never observed
        m = mr.block_mask(N, T, 0.2, min(L, T), 13)
        m[N // 2, :] = 0.0
        m[:, T // 3] = 0.0
    if not m.any():
        m[0, 0] = 1.0
    return np.asfortranarray(m)


def gpu_fit(cmf, data, mask, W0, H0, iters, reg=None, options=None, how="iterate"):
    reg = reg or {}
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        if mask is not None:
            rule.set_mask(mask)
        if how == "iterate":
            lh = [rule.compute_loss()] + list(rule.iterate(iters, **reg))
        elif how == "fit":
            lh, _, _ = rule.fit_native(iters, np.inf, False, 3, 1e-4, False, **reg)
        else:  # call by call
            lh = [rule.compute_loss()]
            for _ in range(iters):
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


@pytest.mark.parametrize("N,T,K,L", SHAPES)
@pytest.mark.parametrize("reg", [dict(), REG])
@pytest.mark.parametrize("kind", ["blocks", "speckle"])
def test_single_iteration(cmf, N, T, K, L, reg, kind):
    """One update_motifs! + update_feature_maps! under a mask against the restatement."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask(kind, N, T, L)
    rule = cmf.MultUpdate(data, W0, H0)
    rule.set_mask(mask)
    l0 = rule.compute_loss()
    rule.update_motifs(l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
    Wg, _ = rule.download()
    loss = rule.update_feature_maps(l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0))
    Wg2, Hg = rule.download()
    rule.close()
    Wr, Hr = W0.copy(), H0.copy()
    r = mr.MaskedMult(data, mask)
    lr0 = mr.masked_loss(r, Wr, Hr)
    mr.update_motifs(r, Wr, Hr, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
    assert frob_rel(Wg, Wr) < REL_FACTORS
    lr = mr.update_feature_maps(r, Wr, Hr, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0))
    np.testing.assert_array_equal(Wg, Wg2)
    print("relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "rel loss", abs(loss - lr) / lr)
    assert frob_rel(Hg, Hr) < REL_FACTORS
    assert abs(loss - lr) <= REL_LOSS * lr and abs(l0 - lr0) <= REL_LOSS * lr0


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (130, 700, 32, 20), (250, 2000, 5, 20)])
def test_unobserved_row_and_column(cmf, N, T, K, L):
    """A unit and a sample without any observed entry are legal: numerators and denominators are 0 there and the factor entries
    fall to eps, as the formulas say."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("holes", N, T, L)
    got = gpu_fit(cmf, data, mask, W0, H0, 3)
    check_against(got, mr.fit_masked(data, mask, W0, H0, max_itr=3), "holes")
    assert np.all(got[0][:, N // 2, :] == np.finfo(np.float64).eps) and np.isfinite(got[1]).all()


@pytest.mark.parametrize("N,T,K,L", SHAPES)
@pytest.mark.parametrize("kind", ["blocks", "speckle"])
def test_masked_conv_norms(cmf, N, T, K, L, kind):
    """One masked conv: with data = 0, cmf_masked_loss returns the squared norm of conv(W, H) over the observed (held-out)
    entries.  |norm a - norm b| <= norm(a - b), so the norm is held to the bar of the conv itself."""
    W0, H0, _ = rand_problem(1, N, T, K, L)
    mask = make_mask(kind, N, T, L)
    est = mr.tensor_conv(W0, H0)
    rule = cmf.MultUpdate(np.zeros((N, T)), W0, H0)
    rule.set_mask(mask)
    for comp in (False, True):
        r, d = rule.masked_loss(complement=comp)
        ref = np.linalg.norm(np.where((mask == 0) if comp else (mask != 0), est, 0.0))
        assert d == 0.0
        assert abs(np.sqrt(r) - ref) <= REL_PRIM * max(ref, 1e-300), (comp, np.sqrt(r), ref)
    rule.close()


@pytest.mark.parametrize("name", ["mu_masked_small", "mu_masked_small_reg", "mu_masked_k5", "mu_masked_k33", "mu_masked_short"])
def test_golden_fit(cmf, name):
    """Full fits through fit_cnmf(mask=) against the committed fixtures (tests/golden/make_golden_masked_mu.py)."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K, N, L = g["W0"].shape
    res = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", max_itr=int(g["max_itr"]), check_convergence=False, W_init=g["W0"], H_init=g["H0"],
                       mask=g["mask"], l1_W=float(g["l1W"]), l2_W=float(g["l2W"]), l1_H=float(g["l1H"]), l2_H=float(g["l2H"]))
    assert len(res.loss_hist) == int(g["max_itr"]) + 1
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), name)


@pytest.mark.parametrize("N,T,K,L", SHAPES)
@pytest.mark.parametrize("reg", [dict(), REG])
@pytest.mark.parametrize("kind", ["blocks", "speckle"])
def test_fit_against_restatement(cmf, N, T, K, L, reg, kind):
    """FIT_ITERS iterations (see the module docstring) on the cases profiles/mu_masked_precision.txt lists."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask(kind, N, T, L)
    got = gpu_fit(cmf, data, mask, W0, H0, FIT_ITERS, reg)
    check_against(got, mr.fit_masked(data, mask, W0, H0, max_itr=FIT_ITERS, **reg), f"{(N, T, K, L)} {kind}")


@pytest.mark.parametrize("N,T,K,L", [(130, 700, 32, 20), (250, 2000, 5, 20)])
@pytest.mark.parametrize("kind", ["blocks", "speckle"])
def test_long_fit_against_restatement(cmf, N, T, K, L, kind):
    """LONG_FIT_ITERS iterations where profiles/mu_masked_precision.txt holds that long (see the module docstring)."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask(kind, N, T, L)
    got = gpu_fit(cmf, data, mask, W0, H0, LONG_FIT_ITERS)
    check_against(got, mr.fit_masked(data, mask, W0, H0, max_itr=LONG_FIT_ITERS), f"{(N, T, K, L)} {kind} x{LONG_FIT_ITERS}")


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (130, 700, 32, 20), (37, 150, 33, 7), (250, 2000, 5, 20)])
@pytest.mark.parametrize("how", ["iterate", "calls"])
def test_heldout_garbage_is_inert(cmf, N, T, K, L, how):
    """The fit with NaN at the held-out entries equals the fit with the true values there, bitwise: Xm is a select."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    bad = np.where(mask != 0, data, np.nan)
    bad[(mask == 0) & (np.arange(T)[None, :] % 2 == 0)] = np.inf
    a = gpu_fit(cmf, data, mask, W0, H0, 5, how=how)
    b = gpu_fit(cmf, bad, mask, W0, H0, 5, how=how)
    for x, y in zip(a, b):
        assert np.isfinite(y).all()
        np.testing.assert_array_equal(x, y)
    for opts in (dict(reuse_est=0), dict(small_k=0)):
        a = gpu_fit(cmf, data, mask, W0, H0, 3, options=opts, how=how)
        b = gpu_fit(cmf, bad, mask, W0, H0, 3, options=opts, how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (130, 700, 32, 20), (37, 150, 33, 7), (250, 2000, 5, 20)])
def test_all_ones_mask_is_the_unmasked_rule(cmf, N, T, K, L):
    W0, H0, data = rand_problem(3, N, T, K, L)
    a = gpu_fit(cmf, data, None, W0, H0, 10)
    b = gpu_fit(cmf, data, np.ones((N, T)), W0, H0, 10)
    np.testing.assert_allclose(b[2], a[2], rtol=1e-6)
    assert frob_rel(b[0], a[0]) < 1e-6 and frob_rel(b[1], a[1]) < 1e-6


NEUTRAL_SHAPES = [(48, 300, 4, 8), (130, 700, 32, 20), (37, 150, 33, 7), (250, 2000, 5, 20)]


@pytest.mark.parametrize("N,T,K,L", NEUTRAL_SHAPES)
@pytest.mark.parametrize("option", ["reuse_est", "speculate"])
def test_option_is_bitwise_neutral_under_a_mask(cmf, N, T, K, L, option):
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    for how in ("calls", "iterate"):
        a = gpu_fit(cmf, data, mask, W0, H0, 4, REG, options={option: 1}, how=how)
        b = gpu_fit(cmf, data, mask, W0, H0, 4, REG, options={option: 0}, how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("N,T,K,L", NEUTRAL_SHAPES)
def test_call_by_call_iterate_and_fit_agree_bitwise(cmf, N, T, K, L):
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("speckle", N, T, L)
    a = gpu_fit(cmf, data, mask, W0, H0, 4, REG, how="calls")
    for how in ("iterate", "fit"):
        b = gpu_fit(cmf, data, mask, W0, H0, 4, REG, how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (130, 700, 32, 20)])
def test_sync_every_call_writeback_is_neutral(cmf, N, T, K, L):
    """The factors written into the caller's arrays behind every call are those of the plain run, and so are the losses."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    a = gpu_fit(cmf, data, mask, W0, H0, 3, how="calls")
    W, H = np.asfortranarray(W0.copy()), np.asfortranarray(H0.copy())
    rule = cmf.MultUpdate(data, W, H, sync_every_call=True)
    lh = []
    for _ in range(3):
        rule.update_motifs(data, W, H, mask=mask)
        lh.append(rule.update_feature_maps(data, W, H, mask=mask))
    rule.close()
    np.testing.assert_array_equal(W, a[0])
    np.testing.assert_array_equal(H, a[1])
    np.testing.assert_array_equal(lh, a[2][1:])


@pytest.mark.parametrize("N,T,K,L", NEUTRAL_SHAPES)
def test_clearing_the_mask_restores_the_unmasked_trajectory(cmf, N, T, K, L):
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    a = gpu_fit(cmf, data, None, W0, H0, 3)
    for clear_with in ("mu", "pgd"):
        rule = cmf.MultUpdate(data, W0, H0)
        rule.set_mask(mask)
        masked = rule.iterate(2)
        if clear_with == "mu":
            rule.set_mask(None)
        else:  # cmf_set_mask keeps its meaning: the mask now belongs to the PGD entries, the MU entries are unmasked again
            cmf.host.check(rule._lib.cmf_set_mask(rule._h, cmf.host.ptr(mask)))
        rule.upload(W0, H0)
        lh = [rule.compute_loss()] + list(rule.iterate(3))
        W, H = rule.download()
        rule.close()
        assert abs(masked[-1] - a[2][2]) > 1e-6 * a[2][2]  # (the masked iterations were another trajectory)
        np.testing.assert_array_equal(W, a[0])
        np.testing.assert_array_equal(H, a[1])
        np.testing.assert_array_equal(lh, a[2])


@pytest.mark.parametrize("N,T,K,L", SHAPES)
@pytest.mark.parametrize("entry", ["mu", "pgd"])
def test_masked_loss(cmf, N, T, K, L, entry):
    """Both sums, for the mask and for its complement, against numpy; the two residual sums add up to the unmasked loss numerator;
    est, the factors and the rule's state are untouched; either mask entry serves."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    twin = cmf.MultUpdate(data, W0, H0)
    rule = cmf.MultUpdate(data, W0, H0)
    if entry == "mu":
        rule.set_mask(mask)
        twin.set_mask(mask)
    else:
        cmf.host.check(rule._lib.cmf_set_mask(rule._h, cmf.host.ptr(mask)))
    rule.iterate(2)
    twin.iterate(2)
    W, H = rule.download()
    sums = {}
    for comp in (False, True):
        r, d = rule.masked_loss(complement=comp)
        rr, dr = mr.heldout_sums(data, mask, W, H, complement=comp)
        print(entry, comp, "resid", r, rr, "data", d, dr)
        assert abs(r - rr) <= 1e-6 * rr and abs(d - dr) <= 1e-6 * max(dr, 1e-300)
        sums[comp] = r
    W2, H2 = rule.download()
    np.testing.assert_array_equal(W2, W)
    np.testing.assert_array_equal(H2, H)
    np.testing.assert_array_equal(rule.iterate(2), twin.iterate(2))  # est and the rule's state were left alone
    plain = cmf.MultUpdate(data, W, H)
    num = (plain.compute_loss() * plain.data_norm) ** 2
    plain.close()
    assert abs(sums[False] + sums[True] - num) <= 1e-6 * num
    rule.close()
    twin.close()


def test_masked_loss_ignores_heldout_nan(cmf):
    N, T, K, L = 48, 300, 4, 8
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    bad = np.where(mask != 0, data, np.nan)
    a, b = cmf.MultUpdate(data, W0, H0), cmf.MultUpdate(bad, W0, H0)
    a.set_mask(mask)
    b.set_mask(mask)
    assert a.masked_loss() == b.masked_loss() and np.isfinite(b.masked_loss()).all()
    a.close()
    b.close()


def test_config2_full_size_against_restatement(cmf):
    """BASELINE.json configs[1] (N=2000, T=50000, K=32, L=20) with 20 % held out in blocks of 20: two iterations against the fp64
    restatement computed here, at the 1e-4 bar (as tests/test_gpu_parity.py::test_config2_full_size_against_oracle does unmasked)."""
    N, T, K, L = 2000, 50000, 32, 20
    data = cmf.gen_synthetic(N=N, T=T, seed=1234)
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
    mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=5)
    assert abs((1.0 - mask.mean()) - 0.2) < 0.01
    try:
        from threadpoolctl import threadpool_limits

        ctx = threadpool_limits(limits=16, user_api="blas")
    except Exception:  # pragma: no cover
        import contextlib

        ctx = contextlib.nullcontext()
    with ctx:
        ref = mr.fit_masked(data, mask, W0, H0, max_itr=2)
    check_against(gpu_fit(cmf, data, mask, W0, H0, 2), ref, "config 2, 20 % held out")


def test_fit_cnmf_with_a_mask_is_the_masked_fit(cmf):
    """Fails without the feature: fit_cnmf(mask=) used to warn about an unknown keyword and fit every entry."""
    g = np.load(os.path.join(GOLDEN, "mu_masked_small.npz"))
    K, N, L = g["W0"].shape
    kw = dict(L=L, K=K, alg=":mult", max_itr=int(g["max_itr"]), check_convergence=False, W_init=g["W0"], H_init=g["H0"])
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(g["data"], mask=g["mask"], **kw)
    plain = cmf.fit_cnmf(g["data"], **kw)
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), "fit_cnmf(mask=)")
    assert frob_rel(res.W, plain.W) > 1e-3 and frob_rel(res.H, plain.H) > 1e-3
    assert abs(res.loss_hist[-1] - plain.loss_hist[-1]) > 1e-3 * plain.loss_hist[-1]
    # init_rand is drawn from Xm: held-out NaNs do not reach the initial factors
    bad = np.where(g["mask"] != 0, g["data"], np.nan)
    r2 = cmf.fit_cnmf(bad, L=L, K=K, alg=":mult", max_itr=3, check_convergence=False, mask=g["mask"], seed=4)
    r3 = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", max_itr=3, check_convergence=False, mask=g["mask"], seed=4)
    assert np.isfinite(r2.loss_hist).all()
    np.testing.assert_array_equal(r2.W, r3.W)
    np.testing.assert_array_equal(r2.loss_hist, r3.loss_hist)


def test_cross_validate(cmf):
    data = cmf.gen_synthetic(N=40, T=600, K=3, L=8, seed=3)
    out = cmf.cross_validate(data, L_vals=(6, 10), K_vals=(2, 3), frac=0.15, repeats=2, seed=17, max_itr=30, check_convergence=False)
    assert sorted(out) == [(6, 2), (6, 3), (10, 2), (10, 3)]
    for (L, K), sc in out.items():
        assert sc["train"].shape == (2,) and sc["test"].shape == (2,)
        assert np.isfinite(sc["train"]).all() and np.isfinite(sc["test"]).all() and np.all(sc["test"] < 1.0), (L, K, sc)
    # by hand, with the same seeds: pair index = combination index * repeats + repeat
    idx = 0
    for L in (6, 10):
        for K in (2, 3):
            for rep in range(2):
                mask = cmf.holdout_mask(40, 600, frac=0.15, block=L, seed=17 + idx)
                r = cmf.fit_cnmf(data, L=L, K=K, alg=":mult", mask=mask, seed=17 + idx, max_itr=30, check_convergence=False)
                train, test = cmf.evaluate_heldout(r, mask)
                assert (train, test) == (out[(L, K)]["train"][rep], out[(L, K)]["test"][rep])
                rule = cmf.MultUpdate(data, r.W, r.H)
                rule.set_mask(mask)
                assert abs(rule.compute_loss() - train) <= 1e-5 * train  # the train score is the masked loss of the fit
                rule.close()
                idx += 1


def test_refusals(cmf):
    N, T, K, L = 48, 300, 4, 8
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    rule = cmf.MultUpdate(data, W0, H0)
    with pytest.raises(cmf.CMFError, match="0 and 1 only") as ei:
        rule.set_mask(0.5 * mask)
    assert ei.value.code == 1
    with pytest.raises(cmf.CMFError, match="observes nothing") as ei:
        rule.set_mask(np.zeros((N, T)))
    assert ei.value.code == 1
    with pytest.raises(cmf.CMFError, match="no mask installed") as ei:
        rule.masked_loss()
    assert ei.value.code == 3
    rule.set_mask(mask)
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_option("gram", 1)
    assert ei.value.code == 4
    for call in (lambda: rule._lib.cmf_hals_update_motifs(rule._h, 0.0, 0.0),):
        with pytest.raises(cmf.CMFError, match="HALS rule has no masked form") as ei:
            cmf.host.check(call())
        assert ei.value.code == 3
    rule.set_mask(None)
    rule.set_option("gram", 1)
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_mask(mask)
    assert ei.value.code == 4
    rule.close()
    hals = cmf.HALSUpdate(data, W0, H0)
    cmf.host.check(hals._lib.cmf_mu_set_mask(hals._h, cmf.host.ptr(mask)))
    with pytest.raises(cmf.CMFError, match="HALS rule has no masked form"):
        hals.update_feature_maps()
    hals.close()
    group = cmf.MultUpdate(data, W0, H0, devices=[0, 0])
    with pytest.raises(cmf.CMFError, match="T-sharded groups") as ei:
        group.set_mask(mask)
    assert ei.value.code == 4
    with pytest.raises(cmf.CMFError, match="T-sharded groups") as ei:
        group.masked_loss()
    assert ei.value.code == 4
    group.close()


@pytest.mark.parametrize("N,T,K,L,options", [
    (250, 2000, 5, 20, dict(small_k=0)), (250, 2000, 5, 20, dict(small_k_fuse=0)), (250, 2000, 5, 20, dict(small_k_fuse=2)),
    (250, 2000, 5, 20, dict(conv_split=0)), (130, 700, 32, 20, dict(conv_kernel=2)), (130, 700, 32, 20, dict(conv_kernel=3)),
    (130, 700, 32, 20, dict(conv_split=0)), (130, 700, 32, 20, dict(conv_split=4)), (130, 700, 32, 20, dict(profile=1)),
    (260, 9000, 64, 20, dict(conv_kernel=2)), (260, 9000, 64, 20, dict()),
])
def test_every_option_is_honoured_under_a_mask(cmf, N, T, K, L, options):
    """Each kernel family and routing choice the MU rule has, masked, against the restatement (with and without reuse_est)."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    mask = make_mask("blocks", N, T, L)
    ref = mr.fit_masked(data, mask, W0, H0, max_itr=3, **REG)
    for reuse in (1, 0):
        got = gpu_fit(cmf, data, mask, W0, H0, 3, REG, options=dict(options, reuse_est=reuse))
        check_against(got, ref, f"{options} reuse_est={reuse}")
