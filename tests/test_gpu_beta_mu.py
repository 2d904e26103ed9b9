"""GPU tests of the beta-divergence form of the MU rule (cmf_mu_set_beta_divergence, MultUpdate.set_divergence(":beta", beta=),
fit_cnmf(divergence=":beta", beta=), evaluate_divergence) against the fp64 restatement tests/beta_mu_restatement.py and the fixtures
tests/golden/mu_beta_*.npz, at the project's bars (tests/test_gpu_parity.py):

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_beta_precision.txt (tools/mu_beta_precision.py: the restatement with
float32 contractions and a float32 epilogue against its fp64 run; a count is admitted while that modelled drift stays within a third
of the bar).  Every fixture was written at a count its line admits -- the test checks that -- and no fixture is skipped or held to
another bar.  The file mirrors tests/test_gpu_is_mu.py.

The padding test is indirect, like the Itakura-Saito one: the library has no entry that reads est back, so what is checked is that
the factors after a few iterations are finite, off the floor and the restatement's on shapes with partly and wholly padded blocks.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import beta_mu_restatement as br

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
BETA = ":beta"
IS = ":itakura_saito"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = ["small", "small_reg", "k5", "k33", "k32", "short", "l40"]
FIXTURES = ([f"mu_beta_{s}_{b}" for s in SHAPES for b in ("b050", "b150")]
            + [f"mu_beta_{s}_{b}" for s in ("small", "short") for b in ("b025", "b200", "b300")])
UNREGULARISED = [n for n in FIXTURES if "_reg_" not in n]
EPS = float(np.finfo(np.float64).eps)
# the conv option sets of tests/test_gpu_is_mu.py, per shape they apply to (small_k*: K <= 16; conv_kernel: K % 32 == 0), at both betas
OPTION_SETS = [(f"mu_beta_{s}_{b}", o) for b in ("b050", "b150") for s, o in
               [("k5", dict(small_k=0)), ("k5", dict(small_k_fuse=0)), ("k5", dict(small_k_fuse=2)),
                ("k5", dict(conv_split=0)), ("small", dict(small_k=0)), ("small", dict(small_k=2)),
                ("l40", dict(small_k=0)), ("short", dict(small_k=0)),
                ("k32", dict(conv_kernel=2)), ("k32", dict(conv_kernel=3)), ("k32", dict(conv_split=0)),
                ("k32", dict(conv_split=4)), ("k32", dict(profile=1)), ("k33", dict(conv_split=0)),
                ("k32", dict(speculate=0))]]
_CACHE = {}


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def admitted():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_beta_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


def load(name):
    if name not in _CACHE:  # (read, and where the fixture holds norms only recomputed, once)
        g = br.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        assert g["max_itr"] <= admitted()[name], f"{name} was written at a count profiles/mu_beta_precision.txt does not admit"
        _CACHE[name] = g
    return _CACHE[name]


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def gpu_fit(cmf, data, W0, H0, beta, iters, reg=None, options=None, how="iterate", eval_mode=False, counters=None):
    reg = reg or {}
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        rule.set_divergence(BETA, beta=beta)
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
        if counters is not None:
            counters["pow"] = rule.counter("pow_update_launches")
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
    reg, beta = g["reg"], g["beta"]
    rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    try:
        for k, v in options.items():
            rule.set_option(k, v)
        rule.set_divergence(BETA, beta=beta)
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
        lr0 = br.beta_loss(g["data"], Wr, Hr, beta)
        br.update_motifs(g["data"], Wr, Hr, beta, l1W=reg["l1W"], l2W=reg["l2W"])
        Wr1 = Wr.copy()
        lr = br.update_feature_maps(g["data"], Wr, Hr, beta, l1H=reg["l1H"], l2H=reg["l2H"])
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
    """fit_cnmf(divergence=":beta", beta=) against the committed fixture: W, H and every entry of loss_hist."""
    g = load(name)
    K, N, L = g["W0"].shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", divergence=BETA, beta=g["beta"], max_itr=g["max_itr"], check_convergence=False,
                           W_init=g["W0"], H_init=g["H0"], l1_W=g["reg"]["l1W"], l2_W=g["reg"]["l2W"], l1_H=g["reg"]["l1H"],
                           l2_H=g["reg"]["l2H"])
    assert len(res.loss_hist) == g["max_itr"] + 1
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), name)
    # evaluate_divergence is the last loss_hist entry (cmf_compute_loss on the downloaded factors)
    ev = cmf.evaluate_divergence(res, kind=BETA, beta=g["beta"])
    assert abs(ev - res.loss_hist[-1]) <= 1e-6 * res.loss_hist[-1], (ev, res.loss_hist[-1])


@pytest.mark.parametrize("name", FIXTURES)
def test_call_by_call_iterate_and_fit(cmf, name):
    """The three ways to run a fit each meet the fixture, and agree with each other bit for bit.  The power kernels run exactly
    where the step exponent is not 1 (1 < beta <= 2 launches the element-wise kernels of the plain rule)."""
    g = load(name)
    ref = (g["W"], g["H"], g["loss_hist"])
    c = {}
    a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["beta"], g["max_itr"], g["reg"], how="calls", counters=c)
    check_against(a, ref, f"{name} calls")
    assert c["pow"] == (0 if 1.0 < g["beta"] <= 2.0 else 2 * g["max_itr"])
    for how in ("iterate", "fit"):
        b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["beta"], g["max_itr"], g["reg"], how=how, counters=c)
        check_against(b, ref, f"{name} {how}")
        assert c["pow"] == (0 if 1.0 < g["beta"] <= 2.0 else 2 * g["max_itr"])
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", UNREGULARISED)
def test_loss_hist_is_non_increasing(cmf, name):
    g = load(name)
    _, _, lh = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["beta"], g["max_itr"])
    steps = np.diff(lh)
    print(name, "largest relative step", float(np.max(steps / lh[:-1])))
    assert np.all(steps <= 1e-6 * lh[:-1])  # (fp32: a relative 1e-6)


@pytest.mark.parametrize("name", [f"mu_beta_{s}_{b}" for s in ("k5", "k32", "k33", "small") for b in ("b050", "b150")])
@pytest.mark.parametrize("option", ["reuse_est", "speculate", "small_k_fuse"])
def test_results_do_not_depend_on_the_fusion_options(cmf, name, option):
    g = load(name)
    for how in ("calls", "iterate"):
        a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["beta"], 4, g["reg"], options={option: 1}, how=how)
        b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["beta"], 4, g["reg"], options={option: 0}, how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["mu_beta_k5_b050", "mu_beta_k5_b150", "mu_beta_k32_b050", "mu_beta_k32_b150"])
def test_eval_mode_updates_H_only(cmf, name):
    g = load(name)
    W, H = g["W0"].copy(), g["H0"].copy()
    lr = [br.beta_loss(g["data"], W, H, g["beta"])]
    for _ in range(3):
        lr.append(br.update_feature_maps(g["data"], W, H, g["beta"]))
    for how in ("iterate", "fit", "calls"):
        got = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["beta"], 3, how=how, eval_mode=True)
        np.testing.assert_array_equal(got[0], g["W0"])  # (W0 is exact in float32: eval_mode leaves W bitwise unchanged)
        check_against(got, (g["W0"], H, np.asarray(lr)), f"{name} eval_mode {how}")


@pytest.mark.parametrize("beta", [0.5, 1.5])
@pytest.mark.parametrize("shape", ["k33", (37, 150, 33, 7)])
def test_padding_columns_store_exact_zeros(cmf, shape, beta):
    """N = 70 and N = 37 leave a partly live 32-column block and wholly padded ones beside the data.  Q = eps^(beta - 1) there is 6.7e7
    at beta = 0.5 and 1.5e-8 -- tiny, not 0 -- at beta = 1.5: both arrays must hold exact zeros instead.  After 3 iterations every
    entry is finite and >= eps, and the factors are the restatement's."""
    if isinstance(shape, str):
        g = load(f"mu_beta_{shape}_b{int(beta * 100):03d}")
        data, W0, H0 = g["data"], g["W0"], g["H0"]
    else:
        data, W0, H0 = (np.asarray(a, dtype=np.float64) for a in br.count_problem(*shape, seed=7))
    ref = br.fit_beta(data, W0, H0, beta, max_itr=3)
    for how in ("calls", "iterate"):
        for options in ({}, dict(reuse_est=0), dict(conv_split=0)):
            got = gpu_fit(cmf, data, W0, H0, beta, 3, options=options, how=how)
            assert all(np.isfinite(x).all() for x in got)
            assert got[0].min() >= EPS and got[1].min() >= EPS
            assert got[1].max() > 1e-3 and got[0].max() > 1e-3  # (not collapsed to the floor)
            check_against(got, ref, f"padding {shape} beta={beta} {how} {options}")


@pytest.mark.parametrize("name", ["mu_beta_small_b050", "mu_beta_k5_b150", "mu_beta_k32_b050", "mu_beta_k33_b150"])
def test_a_walk_beta_kl_is_square_beta_on_one_handle(cmf, name):
    """beta -> KL -> Itakura-Saito -> square -> beta (another beta, then the first again) on ONE handle.  After every switch
    update_motifs! is called at once (an est of the previous form that the switch had not voided would be consumed), then
    update_feature_maps! and two more iterations: W, H and the losses of every segment are bitwise those of a fresh handle that was
    given the segment's starting factors and put directly into that form -- for the square segment, the plain rule's."""
    g = load(name)
    data, beta = g["data"] + 1.0, g["beta"]  # (strictly positive: the walk passes through Itakura-Saito)
    other = 3.0 if beta < 1 else 0.25

    def segment(rule):
        rule.update_motifs()
        lh = [rule.update_feature_maps()] + list(rule.iterate(2))
        return rule.download() + (np.asarray(lh),)

    walk = [("beta", lambda r: r.set_divergence(BETA, beta=beta)),
            ("KL", lambda r: r.set_divergence(":kl")),
            ("Itakura-Saito", lambda r: r.set_divergence(IS)),
            ("square", lambda r: r.set_divergence(":square")),
            ("beta again", lambda r: r.set_divergence(BETA, beta=beta)),
            ("another beta", lambda r: r.set_divergence(BETA, beta=other)),  # (changing beta on an installed handle voids est)
            ("the first beta", lambda r: r.set_divergence(BETA, beta=beta))]
    rule = cmf.MultUpdate(data, g["W0"], g["H0"])
    try:
        W, H = g["W0"], g["H0"]
        seen = []
        for form, switch in walk:
            switch(rule)
            got = segment(rule)
            fresh = cmf.MultUpdate(data, W, H)
            try:
                if form != "square":
                    switch(fresh)
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


def test_error_codes(cmf):
    g = load("mu_beta_small_b050")
    data, W0, H0 = g["data"], g["W0"], g["H0"]
    N, T = data.shape
    check = cmf.host.check
    rule = cmf.MultUpdate(data, W0, H0)
    lib, h = rule._lib, rule._h
    w = cmf.host.BETA_WINDOW
    for bad in (-0.5, 0.0, 1.0, w / 2, 1.0 - w / 2, 1.0 + w / 2, 4.5, float("nan"), float("inf")):
        with pytest.raises(cmf.CMFError) as ei:
            check(lib.cmf_mu_set_beta_divergence(h, bad))
        assert ei.value.code == 1, bad
        if bad in (0.0, 1.0):
            assert "CMF_DIV_IS" in str(ei.value) and "CMF_DIV_KL" in str(ei.value)
    # ... and the handle is still the squared-error rule
    fresh = cmf.MultUpdate(data, W0, H0)
    np.testing.assert_array_equal(fresh.iterate(2), rule.iterate(2))
    fresh.close()
    for edge in (w, 1.0 - w, 1.0 + w, 4.0):  # the window's edges and the upper bound are accepted
        check(lib.cmf_mu_set_beta_divergence(h, edge))
    check(lib.cmf_mu_set_beta_divergence(h, 0.5))
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
        with pytest.raises(cmf.CMFError, match="beta-divergence is installed") as ei:
            check(call())
        assert ei.value.code == 3
    check(lib.cmf_mu_set_divergence(h, 0))
    rule.set_option("gram", 1)
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_divergence(BETA, beta=0.5)
    assert ei.value.code == 4
    rule.set_option("gram", 0)
    rule.set_mask(np.ones((N, T)))
    with pytest.raises(cmf.CMFError, match="no masked form") as ei:
        rule.set_divergence(BETA, beta=0.5)
    assert ei.value.code == 4
    rule.close()
    with pytest.raises(ValueError, match="CMF_DIV_KL"):
        cmf.fit_cnmf(data, L=8, K=4, alg=":mult", divergence=BETA, beta=1.0, max_itr=2)
    group = cmf.MultUpdate(data, W0, H0, devices=[0, 0])
    with pytest.raises(cmf.CMFError) as ei:
        group.set_divergence(BETA, beta=0.5)
    assert ei.value.code == 4
    group.close()


@pytest.mark.parametrize("bad", ["negative", "nan", "inf"])
def test_bad_data_is_refused(cmf, bad):
    g = load("mu_beta_small_b050")
    data = g["data"].copy()
    data[7, 13] = {"negative": -1e-3, "nan": np.nan, "inf": np.inf}[bad]
    rule = cmf.MultUpdate(data, g["W0"], g["H0"])
    with pytest.raises(cmf.CMFError, match="the beta-divergence needs") as ei:
        rule.set_divergence(BETA, beta=0.5)
    assert ei.value.code == 1
    if bad == "negative":  # the handle stays usable as the squared-error rule (finite data)
        fresh = cmf.MultUpdate(data, g["W0"], g["H0"])
        a = list(fresh.iterate(2)) + list(fresh.download())
        fresh.close()
        b = list(rule.iterate(2)) + list(rule.download())
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    rule.close()
