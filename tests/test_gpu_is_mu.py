"""GPU tests of the Itakura-Saito form of the MU rule (option "is_div" + cmf_mu_set_divergence(CMF_DIV_IS),
MultUpdate.set_divergence(":itakura_saito"), fit_cnmf(divergence=":itakura_saito"), evaluate_divergence) against the fp64 restatement
tests/is_mu_restatement.py and the fixtures tests/golden/mu_is_*.npz, at the project's bars (tests/test_gpu_parity.py):

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_is_precision.txt (tools/mu_is_precision.py: the restatement with
float32 contractions and a float32 epilogue against its fp64 run; a count is admitted while that modelled drift stays within a third
of the bar).  Every fixture was written at a count its line admits -- the test checks that -- and no fixture is skipped or held to
another bar.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import is_mu_restatement as ir

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
IS = ":itakura_saito"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_is_small", "mu_is_small_reg", "mu_is_k5", "mu_is_k33", "mu_is_k32", "mu_is_short", "mu_is_l40"]
UNREGULARISED = [n for n in FIXTURES if n != "mu_is_small_reg"]
EPS = float(np.finfo(np.float64).eps)
# the conv option sets of tests/test_gpu_kl_mu.py, per fixture they apply to (small_k*: K <= 16; conv_kernel: K % 32 == 0)
OPTION_SETS = [("mu_is_k5", dict(small_k=0)), ("mu_is_k5", dict(small_k_fuse=0)), ("mu_is_k5", dict(small_k_fuse=2)),
               ("mu_is_k5", dict(conv_split=0)), ("mu_is_small", dict(small_k=0)), ("mu_is_small", dict(small_k=2)),
               ("mu_is_l40", dict(small_k=0)), ("mu_is_short", dict(small_k=0)),
               ("mu_is_k32", dict(conv_kernel=2)), ("mu_is_k32", dict(conv_kernel=3)), ("mu_is_k32", dict(conv_split=0)),
               ("mu_is_k32", dict(conv_split=4)), ("mu_is_k32", dict(profile=1)), ("mu_is_k33", dict(conv_split=0)),
               ("mu_is_k32", dict(speculate=0))]
_CACHE = {}


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def admitted():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_is_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


def load(name):
    if name not in _CACHE:  # (read, and where the fixture holds norms only recomputed, once)
        g = ir.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        assert g["max_itr"] <= admitted()[name], f"{name} was written at a count profiles/mu_is_precision.txt does not admit"
        _CACHE[name] = g
    return _CACHE[name]


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def gpu_fit(cmf, data, W0, H0, iters, reg=None, options=None, how="iterate", eval_mode=False):
    reg = reg or {}
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        rule.set_divergence(IS)
        if how == "iterate":
            lh = [rule.compute_loss()] + list(rule.iterate(iters, eval_mode=eval_mode, **reg))
        elif how == "fit":
            lh, _, _ = rule.fit_native(iters, np.inf, False, 3, 1e-4, eval_mode, **reg)
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


def single_calls(cmf, g, options, what):
    """compute_loss, one update_motifs!, one update_feature_maps! from the fixture's initial factors against the restatement."""
    reg = g["reg"]
    rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    try:
        for k, v in options.items():
            rule.set_option(k, v)
        rule.set_divergence(IS)
        l0 = rule.compute_loss()
        rule.update_motifs(l1W=reg["l1W"], l2W=reg["l2W"])
        Wg, _ = rule.download()
        loss = rule.update_feature_maps(l1H=reg["l1H"], l2H=reg["l2H"])
        Wg2, Hg = rule.download()
        l1 = rule.compute_loss()
    finally:
        rule.close()
    key = ("single", id(g))
    if key not in _CACHE:
        Wr, Hr = g["W0"].copy(), g["H0"].copy()
        lr0 = ir.is_loss(g["data"], Wr, Hr)
        ir.update_motifs(g["data"], Wr, Hr, l1W=reg["l1W"], l2W=reg["l2W"])
        Wr1 = Wr.copy()
        lr = ir.update_feature_maps(g["data"], Wr, Hr, l1H=reg["l1H"], l2H=reg["l2H"])
        _CACHE[key] = (Wr1, Hr, lr0, lr)
    Wr, Hr, lr0, lr = _CACHE[key]
    print(what, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "rel loss", abs(l0 - lr0) / lr0, abs(loss - lr) / lr)
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS
    np.testing.assert_array_equal(Wg, Wg2)
    assert abs(l0 - lr0) <= REL_LOSS * lr0 and abs(loss - lr) <= REL_LOSS * lr and abs(l1 - lr) <= REL_LOSS * lr
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all()


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("small_k", [1, 0])
@pytest.mark.parametrize("reuse_est", [1, 0])
def test_single_calls(cmf, name, small_k, reuse_est):
    single_calls(cmf, load(name), dict(small_k=small_k, reuse_est=reuse_est), f"{name} small_k={small_k} reuse_est={reuse_est}")


@pytest.mark.parametrize("name,options", OPTION_SETS)
def test_single_calls_under_every_conv_option(cmf, name, options):
    for reuse in (1, 0):
        single_calls(cmf, load(name), dict(options, reuse_est=reuse), f"{name} {options} reuse_est={reuse}")


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_fit_through_fit_cnmf(cmf, name):
    """fit_cnmf(divergence=":itakura_saito") against the committed fixture: W, H and every entry of loss_hist."""
    g = load(name)
    K, N, L = g["W0"].shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", divergence=IS, max_itr=g["max_itr"], check_convergence=False,
                           W_init=g["W0"], H_init=g["H0"], l1_W=g["reg"]["l1W"], l2_W=g["reg"]["l2W"], l1_H=g["reg"]["l1H"],
                           l2_H=g["reg"]["l2H"])
    assert len(res.loss_hist) == g["max_itr"] + 1
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), name)
    # evaluate_divergence is the last loss_hist entry (cmf_compute_loss on the downloaded factors)
    ev = cmf.evaluate_divergence(res, kind=IS)
    assert abs(ev - res.loss_hist[-1]) <= 1e-6 * res.loss_hist[-1], (ev, res.loss_hist[-1])


@pytest.mark.parametrize("name", FIXTURES)
def test_call_by_call_iterate_and_fit(cmf, name):
    """The three ways to run a fit each meet the fixture, and agree with each other bit for bit."""
    g = load(name)
    ref = (g["W"], g["H"], g["loss_hist"])
    a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["max_itr"], g["reg"], how="calls")
    check_against(a, ref, f"{name} calls")
    for how in ("iterate", "fit"):
        b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["max_itr"], g["reg"], how=how)
        check_against(b, ref, f"{name} {how}")
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", UNREGULARISED)
def test_loss_hist_is_non_increasing(cmf, name):
    g = load(name)
    _, _, lh = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["max_itr"])
    steps = np.diff(lh)
    print(name, "largest relative step", float(np.max(steps / lh[:-1])))
    assert np.all(steps <= 1e-6 * lh[:-1])  # (fp32: a relative 1e-6)


@pytest.mark.parametrize("name", ["mu_is_k5", "mu_is_k32", "mu_is_k33", "mu_is_small"])
@pytest.mark.parametrize("option", ["reuse_est", "speculate", "small_k_fuse"])
def test_results_do_not_depend_on_the_fusion_options(cmf, name, option):
    g = load(name)
    for how in ("calls", "iterate"):
        a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], 4, g["reg"], options={option: 1}, how=how)
        b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], 4, g["reg"], options={option: 0}, how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["mu_is_k5", "mu_is_k32"])
def test_eval_mode_updates_H_only(cmf, name):
    g = load(name)
    W, H = g["W0"].copy(), g["H0"].copy()
    lr = [ir.is_loss(g["data"], W, H)]
    for _ in range(3):
        lr.append(ir.update_feature_maps(g["data"], W, H))
    for how in ("iterate", "fit", "calls"):
        got = gpu_fit(cmf, g["data"], g["W0"], g["H0"], 3, how=how, eval_mode=True)
        np.testing.assert_array_equal(got[0], g["W0"])  # (W0 is exact in float32: eval_mode leaves W bitwise unchanged)
        check_against(got, (g["W0"], H, np.asarray(lr)), f"{name} eval_mode {how}")


@pytest.mark.parametrize("shape", ["mu_is_k33", (37, 150, 33, 7)])
def test_padding_columns_store_exact_zeros(cmf, shape):
    """N = 70 and N = 37 leave a partly live 32-column block and wholly padded ones beside the data.  Q = 1 / (0 + eps) stored there
    would pour 1 / eps into the denominators of padded W rows -- and, through the transconv, of every H column: H would fall to eps
    and W with it.  After 3 iterations every entry is finite and >= eps, and the factors are the restatement's."""
    if isinstance(shape, str):
        g = load(shape)
        data, W0, H0 = g["data"], g["W0"], g["H0"]
    else:
        data, W0, H0 = (np.asarray(a, dtype=np.float64) for a in ir.positive_problem(*shape, seed=7))
    ref = ir.fit_is(data, W0, H0, max_itr=3)
    for how in ("calls", "iterate"):
        for options in ({}, dict(reuse_est=0), dict(conv_split=0)):
            got = gpu_fit(cmf, data, W0, H0, 3, options=options, how=how)
            assert all(np.isfinite(x).all() for x in got)
            assert got[0].min() >= EPS and got[1].min() >= EPS
            assert got[1].max() > 1e-3 and got[0].max() > 1e-3  # (not collapsed to the floor)
            check_against(got, ref, f"padding {shape} {how} {options}")


@pytest.mark.parametrize("name", ["mu_is_small", "mu_is_k5", "mu_is_k32", "mu_is_k33"])
def test_square_and_kl_after_is_are_the_plain_rules_bit_for_bit(cmf, name):
    g = load(name)

    def plain(rule):
        rule.upload(g["W0"], g["H0"])
        lh = [rule.compute_loss()] + list(rule.iterate(3, **g["reg"]))
        lh.append(rule.update_feature_maps())
        return rule.download() + (np.asarray(lh),)

    for kind in (":square", ":kl"):
        fresh = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
        fresh.set_divergence(kind)
        a = plain(fresh)
        fresh.close()
        rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
        rule.set_divergence(IS)
        first = rule.iterate(2)
        rule.set_divergence(kind)
        b = plain(rule)
        # ... and IS again on the same handle is IS on a fresh one (IS -> KL / square -> IS)
        rule.set_divergence(IS)
        rule.upload(g["W0"], g["H0"])
        again = rule.iterate(2)
        rule.close()
        assert abs(first[-1] - a[2][2]) > 1e-6 * a[2][2]  # (the Itakura-Saito iterations reported another quantity)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(first, again)


def test_error_codes(cmf):
    g = load("mu_is_small")
    data, W0, H0 = g["data"], g["W0"], g["H0"]
    N, T = data.shape
    check, ptr = cmf.host.check, cmf.host.ptr
    rule = cmf.MultUpdate(data, W0, H0)
    lib, h = rule._lib, rule._h
    # the option off (default): kind 2 answers as it always did
    with pytest.raises(cmf.CMFError, match="CMF_DIV_SQUARE") as ei:
        check(lib.cmf_mu_set_divergence(h, 2))
    assert ei.value.code == 1 and "CMF_DIV_IS" not in str(ei.value)
    with pytest.raises(cmf.CMFError, match="is_div must be 0 or 1") as ei:
        rule.set_option("is_div", 2)
    assert ei.value.code == 1
    rule.set_option("is_div", 1)
    check(lib.cmf_mu_set_divergence(h, 2))
    with pytest.raises(cmf.CMFError, match="Itakura-Saito divergence is installed") as ei:
        rule.set_option("is_div", 0)
    assert ei.value.code == 3
    with pytest.raises(cmf.CMFError, match="kind must be") as ei:
        check(lib.cmf_mu_set_divergence(h, 3))
    assert ei.value.code == 1
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_option("gram", 1)
    assert ei.value.code == 4
    with pytest.raises(cmf.CMFError, match="no masked form") as ei:
        rule.set_mask(np.ones((N, T)))
    assert ei.value.code == 4
    loss = ctypes.c_double()
    for call in (lambda: lib.cmf_hals_update_motifs(h, 0.0, 0.0),
                 lambda: lib.cmf_hals_update_feature_maps(h, 0.0, 0.0, ctypes.byref(loss)),
                 lambda: lib.cmf_pgd_update_motifs(h, 0.0, 0.0, 1),
                 lambda: lib.cmf_pgd_update_feature_maps(h, 0.0, 0.0, 1, ctypes.byref(loss))):
        with pytest.raises(cmf.CMFError, match="Itakura-Saito") as ei:
            check(call())
        assert ei.value.code == 3
    check(lib.cmf_mu_set_divergence(h, 0))
    rule.set_option("is_div", 0)  # off again: kind 2 is refused as before
    with pytest.raises(cmf.CMFError, match="CMF_DIV_SQUARE") as ei:
        check(lib.cmf_mu_set_divergence(h, 2))
    assert ei.value.code == 1
    rule.set_option("gram", 1)
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_divergence(IS)
    assert ei.value.code == 4
    rule.set_option("gram", 0)
    rule.set_mask(np.ones((N, T)))
    with pytest.raises(cmf.CMFError, match="no masked form") as ei:
        rule.set_divergence(IS)
    assert ei.value.code == 4
    rule.close()
    group = cmf.MultUpdate(data, W0, H0, devices=[0, 0])
    with pytest.raises(cmf.CMFError) as ei:
        group.set_divergence(IS)
    assert ei.value.code == 4
    group.close()


@pytest.mark.parametrize("bad", ["zero", "negative", "nan", "inf"])
def test_bad_data_is_refused(cmf, bad):
    g = load("mu_is_small")
    data = g["data"].copy()
    data[7, 13] = {"zero": 0.0, "negative": -1e-3, "nan": np.nan, "inf": np.inf}[bad]
    rule = cmf.MultUpdate(data, g["W0"], g["H0"])
    with pytest.raises(cmf.CMFError, match="Itakura-Saito divergence needs") as ei:
        rule.set_divergence(IS)
    assert ei.value.code == 1 and "floor" in str(ei.value)
    if bad in ("zero", "negative"):  # the handle stays usable as the squared-error rule (finite data)
        fresh = cmf.MultUpdate(data, g["W0"], g["H0"])
        a = list(fresh.iterate(2)) + list(fresh.download())
        fresh.close()
        b = list(rule.iterate(2)) + list(rule.download())
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    rule.close()
    if bad == "zero":
        with pytest.raises(cmf.CMFError, match="Itakura-Saito divergence needs"):
            cmf.fit_cnmf(data, L=8, K=4, alg=":mult", divergence=IS, max_itr=2)


@pytest.mark.parametrize("N,T,K,L", [(130, 700, 32, 20), (250, 2000, 5, 20)])
def test_mid_size_fit_against_restatement(cmf, N, T, K, L):
    """100 iterations (the count profiles/mu_is_precision.txt admits for these shapes) against the restatement computed here."""
    assert admitted()[f"synthetic({N},{T},{K},{L})"] >= 100
    data, W0, H0 = (np.asarray(a, dtype=np.float64) for a in ir.positive_problem(N, T, K, L, seed=3))
    ref = ir.fit_is(data, W0, H0, max_itr=100)
    check_against(gpu_fit(cmf, data, W0, H0, 100), ref, f"mid-size {(N, T, K, L)}")


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (96, 1000, 32, 12), (37, 150, 33, 7)])
def test_a_walk_through_every_form_on_one_handle(cmf, N, T, K, L):
    """square -> mask -> KL under the mask -> mask cleared -> Itakura-Saito -> KL -> square on ONE handle.  After every switch
    update_motifs! is called at once (an est of the previous form that the switch had not voided would be consumed), then
    update_feature_maps! and two more iterations: W, H and the losses of every segment are bitwise those of a fresh handle that was
    given the segment's starting factors and put directly into that form."""
    data, W0, H0 = (np.asarray(a, dtype=np.float64) for a in ir.positive_problem(N, T, K, L, seed=11))
    mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=1)

    def segment(rule):
        rule.update_motifs()
        lh = [rule.update_feature_maps()] + list(rule.iterate(2))
        return rule.download() + (np.asarray(lh),)

    #        form            what the walk does on its handle                      a fresh handle, put directly into the form
    walk = [("square", lambda r: None, lambda r: None),
            ("square + mask", lambda r: r.set_mask(mask), lambda r: r.set_mask(mask)),
            ("KL + mask", lambda r: r.set_divergence(":kl"), lambda r: (r.set_divergence(":kl"), r.set_mask(mask))),
            ("KL", lambda r: r.set_mask(None), lambda r: r.set_divergence(":kl")),
            ("Itakura-Saito", lambda r: r.set_divergence(IS), lambda r: r.set_divergence(IS)),
            ("KL again", lambda r: r.set_divergence(":kl"), lambda r: r.set_divergence(":kl")),
            ("square again", lambda r: r.set_divergence(":square"), lambda r: None)]
    rule = cmf.MultUpdate(data, W0, H0)
    rule.set_option("kl_mask", 1)
    try:
        W, H = W0, H0
        seen = []
        for form, switch, install in walk:
            switch(rule)
            got = segment(rule)
            fresh = cmf.MultUpdate(data, W, H)
            try:
                fresh.set_option("kl_mask", 1)
                install(fresh)
                want = segment(fresh)
            finally:
                fresh.close()
            for x, y, what in zip(got, want, ("W", "H", "losses")):
                assert np.isfinite(x).all()
                np.testing.assert_array_equal(x, y, err_msg=f"{form}: {what} of the walked handle and of a fresh one differ")
            seen.append(got[2][-1])
            W, H = got[0].copy(), got[1].copy()
        assert len({float(v) for v in seen}) == len(seen)  # (every segment reported a loss of its own)
    finally:
        rule.close()
