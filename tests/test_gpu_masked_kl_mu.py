"""GPU tests of the KL form of the MU rule under a 0/1 mask (cmf_set_option "kl_mask" + cmf_mu_set_mask + cmf_mu_set_divergence,
fit_cnmf(divergence=":kl", mask=, options={"kl_mask": 1}), evaluate_heldout / cross_validate with divergence=":kl") against the fp64
restatement tests/masked_kl_mu_restatement.py and the fixtures tests/golden/mu_masked_kl_*.npz, at the project's bars:

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_masked_kl_precision.txt (tools/mu_masked_kl_precision.py).  Every
fixture was written at a count its line admits -- load() checks that -- and none is skipped or held to another bar.  Data under
mask == 0 is NaN throughout unless a test says otherwise.  Everything here sets the option "kl_mask", which the library does not
know without the feature.
"""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import kl_mu_restatement as kr
import masked_kl_mu_restatement as mk
import masked_mu_restatement as mr

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_masked_kl_small", "mu_masked_kl_small_reg", "mu_masked_kl_k5", "mu_masked_kl_k33", "mu_masked_kl_k32",
            "mu_masked_kl_short", "mu_masked_kl_l40"]
MONOTONE = [n for n in FIXTURES if n not in ("mu_masked_kl_small_reg", "mu_masked_kl_short")]  # unregularised, T >= L
KL_FIXTURES = ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_k33", "mu_kl_k32", "mu_kl_short", "mu_kl_l40"]
# tests/test_gpu_kl_mu.py::OPTION_SETS on the masked fixtures of the same inputs (small_k*: K <= 16; conv_kernel: K % 32 == 0)
OPTION_SETS = [("mu_masked_kl_k5", dict(small_k=0)), ("mu_masked_kl_k5", dict(small_k_fuse=0)), ("mu_masked_kl_k5", dict(small_k_fuse=2)),
               ("mu_masked_kl_k5", dict(conv_split=0)), ("mu_masked_kl_small", dict(small_k=0)), ("mu_masked_kl_small", dict(small_k=2)),
               ("mu_masked_kl_l40", dict(small_k=0)), ("mu_masked_kl_short", dict(small_k=0)),
               ("mu_masked_kl_k32", dict(conv_kernel=2)), ("mu_masked_kl_k32", dict(conv_kernel=3)), ("mu_masked_kl_k32", dict(conv_split=0)),
               ("mu_masked_kl_k32", dict(conv_split=4)), ("mu_masked_kl_k32", dict(profile=1)), ("mu_masked_kl_k33", dict(conv_split=0)),
               ("mu_masked_kl_k32", dict(speculate=0))]


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


@functools.lru_cache(maxsize=None)
def admitted():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_masked_kl_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


@functools.lru_cache(maxsize=None)
def load(name):
    g = mk.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    assert g["max_itr"] <= admitted()[name], f"{name} was written at a count profiles/mu_masked_kl_precision.txt does not admit"
    return g


@functools.lru_cache(maxsize=None)
def synthetic(shape, kind):
    return mk.synthetic_case(shape, kind)


@functools.lru_cache(maxsize=None)
def single_call_reference(shape, kind, with_reg):
    """(loss of the initial factors, W after one update_motifs!, H after one update_feature_maps!, its loss) of the restatement."""
    assert admitted()[mk.case_name(shape, kind, with_reg)] >= 1
    data, _, mask, W0, H0 = synthetic(shape, kind)
    reg = mk.REG if with_reg else dict(l1W=0, l2W=0, l1H=0, l2H=0)
    rule = mk.MaskedKL(data, mask)
    W, H = W0.copy(), H0.copy()
    l0 = mk.masked_kl_loss(rule, W, H)
    mk.update_motifs(rule, W, H, l1W=reg["l1W"], l2W=reg["l2W"])
    loss = mk.update_feature_maps(rule, W, H, l1H=reg["l1H"], l2H=reg["l2H"])
    return l0, W, H, loss


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def new_rule(cmf, data, mask, W0, H0, options=None, order="mask_first"):
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        rule.set_option("kl_mask", 1)
        if order == "mask_first":
            rule.set_mask(mask)
            rule.set_divergence(":kl")
        else:
            rule.set_divergence(":kl")  # (needs clean raw data: the unmasked check runs first)
            rule.set_mask(mask)
    except Exception:
        rule.close()
        raise
    return rule


def run(rule, iters, reg=None, how="iterate", eval_mode=False):
    reg = reg or {}
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


def gpu_fit(cmf, data, mask, W0, H0, iters, reg=None, options=None, how="iterate", order="mask_first", eval_mode=False):
    rule = new_rule(cmf, data, mask, W0, H0, options, order)
    try:
        return run(rule, iters, reg, how, eval_mode)
    finally:
        rule.close()


def check_against(got, ref, what=""):
    (Wg, Hg, lg), (Wr, Hr, lr) = got, ref
    print(what, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "max rel loss", float(np.max(np.abs(lg - lr) / lr)))
    np.testing.assert_allclose(lg, lr, rtol=REL_LOSS)
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS


def assert_same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def single_calls(cmf, data, mask, W0, H0, reg, options, ref, what):
    """compute_loss, one update_motifs!, one update_feature_maps! from the initial factors against the restatement."""
    lr0, Wr, Hr, lr = ref
    rule = new_rule(cmf, data, mask, W0, H0, options)
    try:
        l0 = rule.compute_loss()
        rule.update_motifs(l1W=reg["l1W"], l2W=reg["l2W"])
        Wg, _ = rule.download()
        loss = rule.update_feature_maps(l1H=reg["l1H"], l2H=reg["l2H"])
        Wg2, Hg = rule.download()
        l1 = rule.compute_loss()
    finally:
        rule.close()
    print(what, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "rel loss", abs(l0 - lr0) / lr0, abs(loss - lr) / lr)
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all()
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS
    np.testing.assert_array_equal(Wg, Wg2)
    assert abs(l0 - lr0) <= REL_LOSS * lr0 and abs(loss - lr) <= REL_LOSS * lr and abs(l1 - lr) <= REL_LOSS * lr


# ---- 1. single calls: every shape, mask, regulariser set, small_k and reuse_est ---------------------------------------------
@pytest.mark.parametrize("shape", mk.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", mk.MASKS)
@pytest.mark.parametrize("with_reg", [False, True], ids=["noreg", "reg"])
def test_single_calls(cmf, shape, kind, with_reg):
    data, _, mask, W0, H0 = synthetic(shape, kind)
    reg = mk.REG if with_reg else dict(l1W=0, l2W=0, l1H=0, l2H=0)
    ref = single_call_reference(shape, kind, with_reg)
    for small_k in (1, 0):
        for reuse_est in (1, 0):
            single_calls(cmf, data, mask, W0, H0, reg, dict(small_k=small_k, reuse_est=reuse_est), ref,
                         f"{shape} {kind} reg={with_reg} small_k={small_k} reuse_est={reuse_est}")


@pytest.mark.parametrize("shape,options,expect,never", [
    ((48, 300, 4, 8), {}, ["conv_small_kernel<2>"], []),
    ((250, 2000, 5, 20), dict(conv_split=0), ["conv_small_kernel<3>", "conv_small_kernel:pre"], ["conv_small_kernel:quarter"]),
    ((250, 2000, 5, 20), {}, ["conv_small_kernel<3>", "conv_small_kernel:quarter"], []),
    # (routed to the one-wave tiles whatever conv_kernel says; 32 tiles on 256 CUs are a thin last round: all cut, in sixteenths)
    ((96, 1000, 32, 12), dict(conv_kernel=2), ["conv3_kernel:pieces16"], ["conv2_kernel", "conv_kernel", "conv3_kernel:whole"]),
    ((96, 1000, 32, 12), dict(conv_split=0), ["conv3_kernel:whole"], ["conv2_kernel", "conv_kernel"]),
    ((37, 150, 33, 7), {}, ["conv_kernel"], ["conv2_kernel"]),
    ((20, 200, 6, 40), dict(small_k=0), ["conv_kernel"], [])])
def test_each_shape_reaches_its_conv_path(cmf, shape, options, expect, never):
    """The launch counters say which conv kernel ran, and the single calls on that path meet the restatement."""
    data, _, mask, W0, H0 = synthetic(shape, "blocks")
    rule = new_rule(cmf, data, mask, W0, H0, options)
    try:
        run(rule, 2, how="calls")
        counts = {n: rule.counter("launches:" + n) for n in expect + never}
    finally:
        rule.close()
    print(shape, options, counts)
    assert all(counts[n] > 0 for n in expect) and all(counts[n] == 0 for n in never), counts
    reg = dict(l1W=0, l2W=0, l1H=0, l2H=0)
    for reuse in (1, 0):
        single_calls(cmf, data, mask, W0, H0, reg, dict(options, reuse_est=reuse), single_call_reference(shape, "blocks", False),
                     f"{shape} {options} reuse_est={reuse}")


def test_a_unit_with_nothing_observed_falls_to_eps(cmf):
    shape = (48, 300, 4, 8)
    data, _, mask, W0, H0 = synthetic(shape, "dead")
    W, H, lh = gpu_fit(cmf, data, mask, W0, H0, 3)
    assert np.isfinite(lh).all() and np.isfinite(W).all() and np.isfinite(H).all()
    assert np.all(W[:, shape[0] // 2, :] == mk.EPS)  # numerator and denominator are both 0 there


# ---- 2. whole fits against every fixture ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_call_by_call_iterate_and_fit(cmf, name):
    """The three ways to run a fit each meet the fixture, and agree with each other bit for bit."""
    g = load(name)
    ref = (g["W"], g["H"], g["loss_hist"])
    a = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], g["max_itr"], g["reg"], how="calls")
    check_against(a, ref, f"{name} calls")
    for how in ("iterate", "fit"):
        b = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], g["max_itr"], g["reg"], how=how)
        check_against(b, ref, f"{name} {how}")
        assert_same(a, b)


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_fit_through_fit_cnmf(cmf, name):
    g = load(name)
    K, N, L = g["W0"].shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", divergence=":kl", mask=g["mask"], options={"kl_mask": 1},
                           max_itr=g["max_itr"], check_convergence=False, W_init=g["W0"], H_init=g["H0"], l1_W=g["reg"]["l1W"],
                           l2_W=g["reg"]["l2W"], l1_H=g["reg"]["l1H"], l2_H=g["reg"]["l2H"])
    assert len(res.loss_hist) == g["max_itr"] + 1
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), name)
    with pytest.raises(NotImplementedError, match="mask="):
        cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", divergence=":kl", mask=g["mask"], max_itr=1)


@pytest.mark.parametrize("name", ["mu_masked_kl_k5", "mu_masked_kl_k32"])
def test_eval_mode_updates_H_only(cmf, name):
    g = load(name)
    rule = mk.MaskedKL(g["data"], g["mask"])
    W, H = g["W0"].copy(), g["H0"].copy()
    lr = [mk.masked_kl_loss(rule, W, H)]
    for _ in range(3):
        lr.append(mk.update_feature_maps(rule, W, H))
    for how in ("iterate", "fit", "calls"):
        got = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], 3, how=how, eval_mode=True)
        check_against(got, (g["W0"], H, np.asarray(lr)), f"{name} eval_mode {how}")


# ---- 3. the option sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,options", OPTION_SETS)
def test_single_calls_under_every_conv_option(cmf, name, options):
    g = load(name)
    rule = mk.MaskedKL(g["data"], g["mask"])
    W, H = g["W0"].copy(), g["H0"].copy()
    l0 = mk.masked_kl_loss(rule, W, H)
    mk.update_motifs(rule, W, H, l1W=g["reg"]["l1W"], l2W=g["reg"]["l2W"])
    loss = mk.update_feature_maps(rule, W, H, l1H=g["reg"]["l1H"], l2H=g["reg"]["l2H"])
    for reuse in (1, 0):
        single_calls(cmf, g["data"], g["mask"], g["W0"], g["H0"], g["reg"], dict(options, reuse_est=reuse), (l0, W, H, loss),
                     f"{name} {options} reuse_est={reuse}")


@pytest.mark.parametrize("name", ["mu_masked_kl_k5", "mu_masked_kl_k32", "mu_masked_kl_k33", "mu_masked_kl_small"])
@pytest.mark.parametrize("option", ["reuse_est", "speculate", "small_k_fuse"])
def test_results_do_not_depend_on_the_fusion_options(cmf, name, option):
    g = load(name)
    for how in ("calls", "iterate"):
        a = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], 4, g["reg"], options={option: 1}, how=how)
        b = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], 4, g["reg"], options={option: 0}, how=how)
        assert_same(a, b)


def test_conv_kernel_2_against_3(cmf):
    g = load("mu_masked_kl_k32")
    a = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], 4, options=dict(conv_kernel=2))
    b = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], 4, options=dict(conv_kernel=3))
    check_against(a, b, "conv_kernel 2 against 3")


# ---- 4. an all-ones mask is the unmasked KL rule ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", KL_FIXTURES)
def test_all_ones_mask_meets_the_unmasked_kl_fixtures(cmf, name):
    """(The denominators come from contractions with ones, where the unmasked rule sums H and W: equal at the bar, not bitwise.)"""
    g = kr.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    itr = min(g["max_itr"], 20)
    got = gpu_fit(cmf, g["data"], np.ones(g["data"].shape), g["W0"], g["H0"], itr, g["reg"], order="kl_first")
    if itr == g["max_itr"]:
        ref = (g["W"], g["H"], g["loss_hist"])
    else:
        ref = kr.fit_kl(g["data"], g["W0"], g["H0"], max_itr=itr, **g["reg"])
        np.testing.assert_allclose(ref[2], g["loss_hist"][: itr + 1], rtol=1e-10)
    check_against(got, ref, f"{name} under an all-ones mask")


# ---- 5. held-out garbage is inert ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", [((48, 300, 4, 8), "blocks"), ((250, 2000, 5, 20), "speckle"), ((96, 1000, 32, 12), "dead"),
                                        ((37, 150, 33, 7), "blocks"), ((20, 200, 6, 40), "speckle"), ((6, 3, 2, 5), "dead"),
                                        ((20, 7, 2, 10), "blocks")])
def test_held_out_garbage_is_inert(cmf, shape, kind):
    _, clean, mask, W0, H0 = synthetic(shape, kind)
    ref = gpu_fit(cmf, np.where(mask != 0, clean, 0.0), mask, W0, H0, 4, mk.REG)
    assert all(np.isfinite(x).all() for x in ref)
    for junk in (np.nan, np.inf, -1.0):
        for reuse in (1, 0):
            got = gpu_fit(cmf, np.where(mask != 0, clean, junk), mask, W0, H0, 4, mk.REG, options=dict(reuse_est=reuse))
            assert_same(got, ref)


# ---- 6. masked_loss, evaluate_heldout, cross_validate -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", [((48, 300, 4, 8), "blocks"), ((96, 1000, 32, 12), "speckle"), ((37, 150, 33, 7), "dead"),
                                        ((250, 2000, 5, 20), "blocks")])
def test_masked_loss_and_evaluate_heldout(cmf, shape, kind):
    _, clean, mask, W0, H0 = synthetic(shape, kind)
    want = [mk.heldout_sums(clean, mask, W0, H0, complement=c) for c in (False, True)]
    rule = new_rule(cmf, clean, mask, W0, H0)
    try:
        before = rule.compute_loss()
        got = [rule.masked_loss(complement=c) for c in (False, True)]
        assert rule.compute_loss() == before  # (nothing stored, the rule's state as it was)
    finally:
        rule.close()
    print(shape, kind, "sums", got, want)
    for (d, s), (dr, sr) in zip(got, want):
        assert abs(d - dr) <= REL_LOSS * dr and abs(s - sr) <= REL_LOSS * sr
    assert abs(before - want[0][0] / want[0][1]) <= REL_LOSS * before
    res = cmf.CNMF_results(np.asfortranarray(clean), W0, H0, np.zeros(1), np.zeros(1))
    train, test = cmf.evaluate_heldout(res, mask, divergence=":kl")
    assert abs(train - want[0][0] / want[0][1]) <= REL_LOSS * train and abs(test - want[1][0] / want[1][1]) <= REL_LOSS * test
    sq_train, sq_test = cmf.evaluate_heldout(res, mask)  # the default stays the squared error
    (r1, d1), (r0, d0) = mr.heldout_sums(clean, mask, W0, H0), mr.heldout_sums(clean, mask, W0, H0, complement=True)
    assert abs(sq_train - np.sqrt(r1 / d1)) <= REL_LOSS * sq_train and abs(sq_test - np.sqrt(r0 / d0)) <= REL_LOSS * sq_test


def test_cross_validate_kl_is_fit_plus_evaluate_by_hand(cmf):
    N, T = 24, 200
    rng = np.random.default_rng(21)
    data = np.asfortranarray(rng.poisson(2.0 * rng.random((N, 1)) * (1.0 + np.sin(np.arange(T) / 7.0) ** 2)).astype(np.float64))
    L_vals, K_vals, seed = [4, 6], [2, 3], 7
    out = cmf.cross_validate(data, L_vals, K_vals, frac=0.2, seed=seed, divergence=":kl", max_itr=5, check_convergence=False)
    idx = 0
    for L in L_vals:
        for K in K_vals:
            s = seed + idx
            mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=s)
            r = cmf.fit_cnmf(data, L=L, K=K, alg=":mult", mask=mask, seed=s, divergence=":kl", options={"kl_mask": 1}, max_itr=5,
                             check_convergence=False)
            train, test = cmf.evaluate_heldout(r, mask, divergence=":kl")
            got = out[(L, K)]
            print((L, K), got, train, test)
            assert np.isfinite(got["train"]).all() and np.isfinite(got["test"]).all()
            assert got["train"][0] == train and got["test"][0] == test
            assert abs(train - r.loss_hist[-1]) <= 1e-5 * train  # the train score is the loss the fit recorded last
            idx += 1


# ---- 7. state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mu_masked_kl_small", "mu_masked_kl_k32", "mu_masked_kl_k33"])
def test_install_orders_and_replacing_the_mask(cmf, name):
    g = load(name)
    clean, mask, W0, H0 = g["clean"], g["mask"], g["W0"], g["H0"]
    a = gpu_fit(cmf, clean, mask, W0, H0, 3, g["reg"], order="mask_first")
    b = gpu_fit(cmf, clean, mask, W0, H0, 3, g["reg"], order="kl_first")
    assert_same(a, b)
    assert_same(a, gpu_fit(cmf, g["data"], mask, W0, H0, 3, g["reg"]))  # (NaN under the mask: the same)
    other = np.asfortranarray(1.0 - mask if (1.0 - mask).any() and (clean * (1.0 - mask)).sum() > 0 else mask[::-1].copy())
    rule = new_rule(cmf, clean, other, W0, H0)
    try:
        run(rule, 2, g["reg"])
        rule.set_mask(mask)  # replaced while KL is installed
        rule.upload(W0, H0)
        assert_same(run(rule, 3, g["reg"]), a)
    finally:
        rule.close()


@pytest.mark.parametrize("name", ["mu_masked_kl_small", "mu_masked_kl_k32"])
def test_clearing_the_mask(cmf, name):
    g = load(name)
    check, ptr = cmf.host.check, cmf.host.ptr
    # clean raw data: the unmasked KL rule bit for bit against a fresh handle
    fresh = cmf.MultUpdate(g["clean"], g["W0"], g["H0"])
    fresh.set_divergence(":kl")
    want = run(fresh, 3, g["reg"])
    fresh.close()
    rule = new_rule(cmf, g["clean"], g["mask"], g["W0"], g["H0"])
    try:
        run(rule, 2, g["reg"])
        rule.set_mask(None)
        rule.upload(g["W0"], g["H0"])
        assert_same(run(rule, 3, g["reg"]), want)
    finally:
        rule.close()
    # NaN under the mask: clearing it is refused (the raw data fail the KL check) and the handle stays as it was
    want = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], 5, g["reg"])
    rule = new_rule(cmf, g["data"], g["mask"], g["W0"], g["H0"])
    try:
        lh = list(run(rule, 2, g["reg"])[2])
        with pytest.raises(cmf.CMFError, match="KL divergence needs") as ei:
            rule.set_mask(None)
        assert ei.value.code == 1
        with pytest.raises(cmf.CMFError, match="KL divergence needs") as ei:  # cmf_set_mask takes the MU mask away too
            check(rule._lib.cmf_set_mask(rule._h, ptr(np.asfortranarray(g["mask"]))))
        assert ei.value.code == 1
        lh += list(rule.iterate(3, **g["reg"]))
        W, H = rule.download()
        assert_same((W, H, np.asarray(lh)), want)
    finally:
        rule.close()


@pytest.mark.parametrize("name", ["mu_masked_kl_small", "mu_masked_kl_k5", "mu_masked_kl_k32", "mu_masked_kl_k33"])
def test_square_after_masked_kl_is_the_masked_rule_bit_for_bit(cmf, name):
    g = load(name)

    def plain(rule):
        rule.upload(g["W0"], g["H0"])
        lh = [rule.compute_loss()] + list(rule.iterate(3, **g["reg"]))
        lh.append(rule.update_feature_maps())
        return rule.download() + (np.asarray(lh),)

    fresh = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    fresh.set_mask(g["mask"])
    a = plain(fresh)
    fresh.close()
    rule = new_rule(cmf, g["data"], g["mask"], g["W0"], g["H0"])
    kl = rule.iterate(2)
    rule.set_divergence(":square")
    b = plain(rule)
    rule.close()
    assert abs(kl[-1] - a[2][2]) > 1e-6 * a[2][2]  # (the KL iterations reported another quantity)
    assert_same(a, b)


def test_error_codes(cmf):
    g = load("mu_masked_kl_small")
    data, clean, mask, W0, H0 = g["data"], g["clean"], g["mask"], g["W0"], g["H0"]
    check, ptr = cmf.host.check, cmf.host.ptr
    rule = cmf.MultUpdate(clean, W0, H0)
    # option off (the default, or set back): the two refusals of before
    for off in (False, True):
        if off:
            rule.set_option("kl_mask", 1)
            rule.set_option("kl_mask", 0)
        rule.set_divergence(":kl")
        with pytest.raises(cmf.CMFError, match="no masked form") as ei:
            rule.set_mask(mask)
        assert ei.value.code == 4
        rule.set_divergence(":square")
        rule.set_mask(mask)
        with pytest.raises(cmf.CMFError, match="no masked form") as ei:
            rule.set_divergence(":kl")
        assert ei.value.code == 4
        rule.set_mask(None)
    with pytest.raises(cmf.CMFError, match="kl_mask must be 0 or 1") as ei:
        rule.set_option("kl_mask", 2)
    assert ei.value.code == 1
    rule.set_option("kl_mask", 1)
    rule.set_mask(mask)
    rule.set_divergence(":kl")
    with pytest.raises(cmf.CMFError, match="both installed") as ei:
        rule.set_option("kl_mask", 0)
    assert ei.value.code == 3
    with pytest.raises(cmf.CMFError, match="Gram") as ei:
        rule.set_option("gram", 1)
    assert ei.value.code == 4
    weights = mask.copy()
    weights[0, 0] = 0.5
    with pytest.raises(cmf.CMFError, match="0 and 1 only") as ei:
        rule.set_mask(weights)
    assert ei.value.code == 1
    loss = ctypes.c_double()
    for call in (lambda: rule._lib.cmf_hals_update_motifs(rule._h, 0.0, 0.0),
                 lambda: rule._lib.cmf_hals_update_feature_maps(rule._h, 0.0, 0.0, ctypes.byref(loss)),
                 lambda: rule._lib.cmf_pgd_update_motifs(rule._h, 0.0, 0.0, 1),
                 lambda: rule._lib.cmf_pgd_update_feature_maps(rule._h, 0.0, 0.0, 1, ctypes.byref(loss))):
        with pytest.raises(cmf.CMFError) as ei:
            check(call())
        assert ei.value.code == 3
    assert np.isfinite(rule.iterate(2)).all()  # (none of the refusals disturbed the rule)
    rule.close()
    # observed data that the KL form cannot take: refused whichever of the two comes second, code 1
    i, j = np.argwhere(mask != 0)[3]
    for bad in (-1e-3, np.nan, np.inf):
        d = data.copy()
        d[i, j] = bad
        rule = cmf.MultUpdate(d, W0, H0)
        rule.set_option("kl_mask", 1)
        rule.set_mask(mask)
        with pytest.raises(cmf.CMFError, match="KL divergence needs") as ei:
            rule.set_divergence(":kl")
        assert ei.value.code == 1
        rule.close()
    d = clean.copy()
    d[i, j] = -1.0
    other = mask.copy()
    other[i, j] = 0.0
    rule = new_rule(cmf, d, other, W0, H0)  # (valid under `other`, which holds the bad entry out)
    want = run(rule, 2)
    with pytest.raises(cmf.CMFError, match="KL divergence needs") as ei:
        rule.set_mask(mask)  # a mask that observes the bad entry: refused, the old one stays
    assert ei.value.code == 1
    rule.upload(W0, H0)
    assert_same(run(rule, 2), want)
    rule.close()
    group = cmf.MultUpdate(clean, W0, H0, devices=[0, 0])
    for call in (lambda: group.set_option("kl_mask", 1), lambda: group.set_mask(mask), lambda: group.set_divergence(":kl")):
        with pytest.raises(cmf.CMFError) as ei:
            call()
        assert ei.value.code == 4
    group.close()


# ---- 8. the loss does not increase -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MONOTONE)
def test_loss_hist_is_non_increasing(cmf, name):
    g = load(name)
    _, _, lh = gpu_fit(cmf, g["data"], g["mask"], g["W0"], g["H0"], g["max_itr"])
    steps = np.diff(lh)
    print(name, "largest relative step", float(np.max(steps / lh[:-1])))
    assert np.all(steps <= 1e-6 * lh[:-1])  # (fp32 sums: a relative 1e-6, as in tests/test_gpu_kl_mu.py)
