"""GPU tests of the KL form of the MU rule (cmf_mu_set_divergence, MultUpdate.set_divergence, fit_cnmf(divergence=":kl"),
evaluate_divergence) against the fp64 restatement tests/kl_mu_restatement.py and the fixtures tests/golden/mu_kl_*.npz, at the
project's bars (tests/test_gpu_parity.py):

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_kl_precision.txt (tools/mu_kl_precision.py: the restatement with
float32 contractions against its fp64 run; a count is admitted while that modelled drift stays within a third of the bar).  Every
fixture was written at a count its line admits -- the test checks that -- and no fixture is skipped or held to another bar.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import kl_mu_restatement as kr

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_k33", "mu_kl_k32", "mu_kl_short", "mu_kl_l40"]
UNREGULARISED = [n for n in FIXTURES if n != "mu_kl_small_reg"]
EPS = float(np.finfo(np.float64).eps)
# the options the masked tests sweep, per fixture they apply to (small_k*: K <= 16; conv_kernel: K % 32 == 0)
OPTION_SETS = [("mu_kl_k5", dict(small_k=0)), ("mu_kl_k5", dict(small_k_fuse=0)), ("mu_kl_k5", dict(small_k_fuse=2)),
               ("mu_kl_k5", dict(conv_split=0)), ("mu_kl_small", dict(small_k=0)), ("mu_kl_small", dict(small_k=2)),
               ("mu_kl_l40", dict(small_k=0)), ("mu_kl_short", dict(small_k=0)),
               ("mu_kl_k32", dict(conv_kernel=2)), ("mu_kl_k32", dict(conv_kernel=3)), ("mu_kl_k32", dict(conv_split=0)),
               ("mu_kl_k32", dict(conv_split=4)), ("mu_kl_k32", dict(profile=1)), ("mu_kl_k33", dict(conv_split=0)),
               ("mu_kl_k32", dict(speculate=0))]


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def admitted():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_kl_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


def load(name):
    g = kr.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    assert g["max_itr"] <= admitted()[name], f"{name} was written at a count profiles/mu_kl_precision.txt does not admit"
    return g


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def gpu_fit(cmf, data, W0, H0, iters, reg=None, options=None, how="iterate", eval_mode=False):
    reg = reg or {}
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        rule.set_divergence(":kl")
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
        rule.set_divergence(":kl")
        l0 = rule.compute_loss()
        rule.update_motifs(l1W=reg["l1W"], l2W=reg["l2W"])
        Wg, _ = rule.download()
        loss = rule.update_feature_maps(l1H=reg["l1H"], l2H=reg["l2H"])
        Wg2, Hg = rule.download()
        l1 = rule.compute_loss()
    finally:
        rule.close()
    Wr, Hr = g["W0"].copy(), g["H0"].copy()
    lr0 = kr.kl_loss(g["data"], Wr, Hr)
    kr.update_motifs(g["data"], Wr, Hr, l1W=reg["l1W"], l2W=reg["l2W"])
    relW = frob_rel(Wg, Wr)
    lr = kr.update_feature_maps(g["data"], Wr, Hr, l1H=reg["l1H"], l2H=reg["l2H"])
    print(what, "relW", relW, "relH", frob_rel(Hg, Hr), "rel loss", abs(l0 - lr0) / lr0, abs(loss - lr) / lr)
    assert relW < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS
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
    """fit_cnmf(divergence=":kl") against the committed fixture: W, H and every entry of loss_hist."""
    g = load(name)
    K, N, L = g["W0"].shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", divergence=":kl", max_itr=g["max_itr"], check_convergence=False,
                           W_init=g["W0"], H_init=g["H0"], l1_W=g["reg"]["l1W"], l2_W=g["reg"]["l2W"], l1_H=g["reg"]["l1H"],
                           l2_H=g["reg"]["l2H"])
    assert len(res.loss_hist) == g["max_itr"] + 1
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), name)
    # evaluate_divergence is the last loss_hist entry (cmf_compute_loss on the downloaded factors)
    ev = cmf.evaluate_divergence(res)
    assert abs(ev - res.loss_hist[-1]) <= 1e-6 * res.loss_hist[-1], (ev, res.loss_hist[-1])
    mse = cmf.evaluate_mse(res)
    assert abs(cmf.evaluate_divergence(res, kind=":square") - mse) <= 1e-6 * mse


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


@pytest.mark.parametrize("name", ["mu_kl_k5", "mu_kl_k32", "mu_kl_k33", "mu_kl_small"])
@pytest.mark.parametrize("option", ["reuse_est", "speculate", "small_k_fuse"])
def test_results_do_not_depend_on_the_fusion_options(cmf, name, option):
    g = load(name)
    for how in ("calls", "iterate"):
        a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], 4, g["reg"], options={option: 1}, how=how)
        b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], 4, g["reg"], options={option: 0}, how=how)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["mu_kl_k5", "mu_kl_k32"])
def test_eval_mode_updates_H_only(cmf, name):
    g = load(name)
    W, H = g["W0"].copy(), g["H0"].copy()
    lr = [kr.kl_loss(g["data"], W, H)]
    for _ in range(3):
        lr.append(kr.update_feature_maps(g["data"], W, H))
    for how in ("iterate", "fit", "calls"):
        got = gpu_fit(cmf, g["data"], g["W0"], g["H0"], 3, how=how, eval_mode=True)
        check_against(got, (g["W0"], H, np.asarray(lr)), f"{name} eval_mode {how}")


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (130, 700, 32, 20), (37, 150, 33, 7)])
def test_zeros_and_an_all_zero_unit_give_finite_factors(cmf, N, T, K, L):
    data, W0, H0 = kr.synthetic(N, T, K, L, seed=4)
    assert (data == 0).mean() > 0.25 and not data[N // 2].any()
    got = gpu_fit(cmf, data, W0, H0, 5)
    assert all(np.isfinite(x).all() for x in got)
    assert np.all(got[0][:, N // 2, :] == EPS)  # the all-zero unit's motif entries fall to eps
    check_against(got, kr.fit_kl(data, W0, H0, max_itr=5), f"zeros {(N, T, K, L)}")


@pytest.mark.parametrize("name", ["mu_kl_small", "mu_kl_k5", "mu_kl_k32", "mu_kl_k33"])
def test_square_after_kl_is_the_plain_rule_bit_for_bit(cmf, name):
    g = load(name)

    def plain(rule):
        rule.upload(g["W0"], g["H0"])
        lh = [rule.compute_loss()] + list(rule.iterate(3, **g["reg"]))
        lh.append(rule.update_feature_maps())
        return rule.download() + (np.asarray(lh),)

    fresh = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    a = plain(fresh)
    fresh.close()
    rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    rule.set_divergence(":kl")
    kl = rule.iterate(2)
    rule.set_divergence(":square")
    b = plain(rule)
    rule.close()
    assert abs(kl[-1] - a[2][2]) > 1e-6 * a[2][2]  # (the KL iterations reported another quantity)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_error_codes(cmf):
    g = load("mu_kl_small")
    data, W0, H0 = g["data"], g["W0"], g["H0"]
    N, T = data.shape
    check, ptr = cmf.host.check, cmf.host.ptr
    rule = cmf.MultUpdate(data, W0, H0)
    with pytest.raises(cmf.CMFError, match="CMF_DIV_SQUARE") as ei:
        check(rule._lib.cmf_mu_set_divergence(rule._h, 2))
    assert ei.value.code == 1
    rule.set_divergence(":kl")
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_option("gram", 1)
    assert ei.value.code == 4
    with pytest.raises(cmf.CMFError, match="no masked form") as ei:
        rule.set_mask(np.ones((N, T)))
    assert ei.value.code == 4
    loss = ctypes.c_double()
    for call in (lambda: rule._lib.cmf_hals_update_motifs(rule._h, 0.0, 0.0),
                 lambda: rule._lib.cmf_hals_update_feature_maps(rule._h, 0.0, 0.0, ctypes.byref(loss)),
                 lambda: rule._lib.cmf_pgd_update_motifs(rule._h, 0.0, 0.0, 1),
                 lambda: rule._lib.cmf_pgd_update_feature_maps(rule._h, 0.0, 0.0, 1, ctypes.byref(loss))):
        with pytest.raises(cmf.CMFError, match="KL divergence is installed") as ei:
            check(call())
        assert ei.value.code == 3
    rule.set_divergence(":square")
    rule.set_option("gram", 1)
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_divergence(":kl")
    assert ei.value.code == 4
    rule.set_option("gram", 0)
    rule.set_mask(np.ones((N, T)))
    with pytest.raises(cmf.CMFError, match="no masked form") as ei:
        rule.set_divergence(":kl")
    assert ei.value.code == 4
    rule.close()
    group = cmf.MultUpdate(data, W0, H0, devices=[0, 0])
    with pytest.raises(cmf.CMFError, match="T-sharded groups") as ei:
        group.set_divergence(":kl")
    assert ei.value.code == 4
    group.close()


@pytest.mark.parametrize("bad", ["negative", "nan", "inf", "zero"])
def test_bad_data_is_refused(cmf, bad):
    g = load("mu_kl_small")
    data = g["data"].copy()
    if bad == "zero":
        data[:] = 0.0
    else:
        data[7, 13] = {"negative": -1e-3, "nan": np.nan, "inf": np.inf}[bad]
    rule = cmf.MultUpdate(data, g["W0"], g["H0"])
    with pytest.raises(cmf.CMFError, match="KL divergence needs") as ei:
        rule.set_divergence(":kl")
    assert ei.value.code == 1
    rule.close()
    if bad == "negative":
        with pytest.raises(cmf.CMFError, match="KL divergence needs"):
            cmf.fit_cnmf(data, L=8, K=4, alg=":mult", divergence=":kl", max_itr=2)


def test_config2_full_size_against_restatement(cmf):
    """BASELINE.json configs[1] (N=2000, T=50000, K=32, L=20), the synthetic data clipped at 0: two iterations against the fp64
    restatement computed here, at the 1e-4 bar."""
    N, T, K, L = 2000, 50000, 32, 20
    data = np.maximum(cmf.gen_synthetic(N=N, T=T, seed=1234), 0.0)
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
    try:
        from threadpoolctl import threadpool_limits

        ctx = threadpool_limits(limits=16, user_api="blas")
    except Exception:  # pragma: no cover
        import contextlib

        ctx = contextlib.nullcontext()
    with ctx:
        ref = kr.fit_kl(data, W0, H0, max_itr=2)
    check_against(gpu_fit(cmf, data, W0, H0, 2), ref, "config 2")
