"""GPU tests of seqNMF's cross-orthogonality penalties on the MU rule (cmf_mu_set_xortho, cmf_mu_xortho_cost, cmf_mu_xortho_terms;
MultUpdate.set_xortho / xortho_cost / xortho_terms, fit_cnmf(lambda_xortho=, lambda_ortho_H=, lambda_ortho_W=), evaluate_xortho,
xortho_sweep) against the fp64 restatement tests/xortho_mu_restatement.py and the fixtures tests/golden/mu_xortho_*.npz, at the
project's bars (tests/test_gpu_parity.py):

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_xortho_precision.txt (tools/mu_xortho_precision.py).  Every fixture was
written at a count its line admits -- `load` checks that -- and no fixture is skipped or held to another bar.  The four denominator
terms and the three costs are compared EXACTLY on integer-valued problems whose every sum stays below 2^24.

The terms entry reaches xH by another route than the update takes (a one-source C3 contraction and an unweighted off), and the norm-wise
bars above pass a fault confined to one chunk tail, one window seam or one k block.  tests/test_gpu_exact_xortho.py holds the penalised
UPDATES themselves to fp64 at 2 ulp per element on every kernel path of the shape table, the fold kernel's second pass, and the state
around G bitwise; tests/test_gpu_exact_cu_plans.py repeats it under plans for fewer compute units.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import exact_problems as ep
import xortho_mu_restatement as xr

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = [name for name, _, _ in xr.CASES]
EXACT_SHAPES = ["k5", "k32", "k33", "short", "l1", "edge", "l40", (37, 150, 33, 7)]
# the conv option sets of tests/test_gpu_beta_mu.py, per shape they apply to (small_k*: K <= 16; conv_kernel: K % 32 == 0), at both weight sets
OPTION_SETS = [(f"mu_xortho_{s}_{w}", o) for w in xr.WEIGHT_SETS for s, o in
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


def load(name):
    if name not in _CACHE:  # (read, and where the fixture holds norms only recomputed, once)
        g = xr.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        assert g["max_itr"] <= xr.admitted()[name], f"{name} was written at a count profiles/mu_xortho_precision.txt does not admit"
        _CACHE[name] = g
    return _CACHE[name]


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def gpu_fit(cmf, data, W0, H0, weights, iters, reg=None, options=None, how="iterate", eval_mode=False, counters=None):
    reg = reg or {}
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        if weights is not None:
            rule.set_xortho(*weights)
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
            for name in ("xortho_launches", "small_k_fused_h_updates", "speculated_contractions"):
                counters[name] = rule.counter(name)
            counters["costs"] = rule.xortho_cost()
        return W, H, np.asarray(lh)
    finally:
        rule.close()


def check_against(got, ref, what=""):
    (Wg, Hg, lg), (Wr, Hr, lr) = got, ref
    print(what, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "max rel loss", float(np.max(np.abs(lg - lr) / lr)))
    np.testing.assert_allclose(lg, lr, rtol=REL_LOSS)
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS


# ---- exact terms -----------------------------------------------------------------------------------------------------------------
def shape_of(shape):
    return xr.shape_row(shape)[1] if isinstance(shape, str) else shape


def integer_problems(N, T, K, L):
    """Integer-valued (W, H, X): a dense H of ones and twos, and H as a single impulse at the first, the last and a mid column and on
    either side of the column-block boundaries of the smoothing (64) and the off (256) kernels."""
    W, H, X = ep.make_problem(N, T, K, L, "H", seed=3)
    X = np.asfortranarray(X % 4.0)  # (xW sums G <= 2 (K - 1) (2 L - 1) times data over T columns: 1.3e7 at the largest shape)
    out = [("dense", W, H, X)]
    for t0 in sorted({0, T - 1, T // 2, 63, 64, 255, 256}):
        if 0 <= t0 < T:
            Hi = np.zeros((K, T), order="F")
            Hi[(t0 * 7) % K, t0] = 3.0
            out.append((f"impulse at {t0}", W, Hi, X))
    return out


def check_exact(cmf, W, H, X, options, what):
    want = xr.terms(X, W, H)
    wcost = xr.costs(X, W, H)
    A = xr.tensor_transconv(W, X)
    for a in want + (A, xr.smooth(A, W.shape[2]), W.sum(axis=2)):
        assert np.all(a == np.rint(a)) and a.max() < ep.EXACT, what  # (every sum the device forms in fp32 is an integer below 2^24)
    assert max(wcost) < 2.0 ** 53
    rule = cmf.MultUpdate(X, W, H)
    try:
        for k, v in options.items():
            rule.set_option(k, v)
        for name, g, w in zip(("xW", "xH", "oH", "oW"), rule.xortho_terms(), want):
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
        np.testing.assert_array_equal(rule.xortho_cost(), wcost, err_msg=f"{what}: costs")
        # the contraction reads lag-shifted rows out of G's padding, which must be exact zeros and stay so: after one penalised
        # update_motifs! (W changes, H and data do not) xW is still exact
        rule.set_xortho(0.5, 0.25, 0.125)
        rule.update_motifs()
        np.testing.assert_array_equal(rule.xortho_terms()[0], want[0], err_msg=f"{what}: xW after update_motifs!")
        assert rule.counter("xortho_launches") > 0
    finally:
        rule.close()


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
def test_terms_and_costs_are_exact_on_integer_problems(cmf, shape):
    N, T, K, L = shape_of(shape)
    for small_k in ((1, 0) if K <= 16 else (None,)):
        options = {} if small_k is None else dict(small_k=small_k)
        for name, W, H, X in integer_problems(N, T, K, L):
            check_exact(cmf, W, H, X, options, f"{shape} {name} {options}")


def test_null_outputs_are_skipped(cmf):
    W, H, X = ep.make_problem(*shape_of("k5"), "H", seed=3)
    X = np.asfortranarray(X % 4.0)
    rule = cmf.MultUpdate(X, W, H)
    try:
        lib, h, check = rule._lib, rule._h, cmf.host.check
        want, wcost = xr.terms(X, W, H), xr.costs(X, W, H)
        check(lib.cmf_mu_xortho_terms(h, None, None, None, None))
        check(lib.cmf_mu_xortho_cost(h, None, None, None))
        for i in range(3):
            c = ctypes.c_double(-1.0)
            args = [None, None, None]
            args[i] = ctypes.byref(c)
            check(lib.cmf_mu_xortho_cost(h, *args))
            assert c.value == wcost[i]
        xH = np.zeros(H.shape, order="F")
        check(lib.cmf_mu_xortho_terms(h, None, xH.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None))
        np.testing.assert_array_equal(xH, want[1])
    finally:
        rule.close()


# ---- K = 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mu_xortho_k1_x", "mu_xortho_k1_all"])
def test_one_component_has_no_penalty(cmf, name):
    g = load(name)
    rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    try:
        rule.set_xortho(3.0, 2.0, 1.0)
        for t in rule.xortho_terms():
            assert np.all(t == 0.0)
        assert rule.xortho_cost() == (0.0, 0.0, 0.0)
    finally:
        rule.close()
    plain = xr.fit(g["data"], g["W0"], g["H0"], max_itr=g["max_itr"])
    for how in ("calls", "iterate"):
        check_against(gpu_fit(cmf, g["data"], g["W0"], g["H0"], (3.0, 2.0, 1.0), g["max_itr"], how=how), plain, f"{name} {how}")
    np.testing.assert_allclose(g["loss_hist"], plain[2], rtol=1e-12)  # (the fixture itself is the plain rule's)


# ---- single calls ----------------------------------------------------------------------------------------------------------------
def single_calls(cmf, g, options, what):
    """compute_loss, one update_motifs!, one update_feature_maps! from the fixture's initial factors against the restatement."""
    reg, w = g["reg"], g["weights"]
    rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    try:
        for k, v in options.items():
            rule.set_option(k, v)
        rule.set_xortho(*w)
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
        lr0 = xr.compute_loss(g["data"], Wr, Hr)
        xr.update_motifs(g["data"], Wr, Hr, *w, l1W=reg["l1W"], l2W=reg["l2W"])
        Wr1 = Wr.copy()
        lr = xr.update_feature_maps(g["data"], Wr, Hr, *w, l1H=reg["l1H"], l2H=reg["l2H"])
        _CACHE[key] = (Wr1, Hr, lr0, lr)
    Wr, Hr, lr0, lr = _CACHE[key]
    print(what, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "rel loss", abs(l0 - lr0) / lr0, abs(loss - lr) / lr)
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS
    np.testing.assert_array_equal(Wg, Wg2)
    assert abs(l0 - lr0) <= REL_LOSS * lr0 and abs(loss - lr) <= REL_LOSS * lr and abs(l1 - lr) <= REL_LOSS * lr
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all()


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("small_k", [1, 0])
def test_single_calls(cmf, name, small_k):
    single_calls(cmf, load(name), dict(small_k=small_k), f"{name} small_k={small_k}")


@pytest.mark.parametrize("name,options", OPTION_SETS)
def test_single_calls_under_every_conv_option(cmf, name, options):
    for reuse in (1, 0):
        single_calls(cmf, load(name), dict(options, reuse_est=reuse), f"{name} {options} reuse_est={reuse}")


# ---- whole fits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_whole_fit_through_fit_cnmf(cmf, name):
    g = load(name)
    K, N, L = g["W0"].shape
    lam, lamH, lamW = g["weights"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (an "unknown keyword" warning is a failure)
        res = cmf.fit_cnmf(g["data"], L=L, K=K, alg=":mult", lambda_xortho=lam, lambda_ortho_H=lamH, lambda_ortho_W=lamW, max_itr=g["max_itr"],
                           check_convergence=False, W_init=g["W0"], H_init=g["H0"], l1_W=g["reg"]["l1W"], l2_W=g["reg"]["l2W"],
                           l1_H=g["reg"]["l1H"], l2_H=g["reg"]["l2H"])
    assert len(res.loss_hist) == g["max_itr"] + 1
    check_against((res.W, res.H, res.loss_hist), (g["W"], g["H"], g["loss_hist"]), name)
    ev = cmf.evaluate_xortho(res)
    print(name, "costs", ev, "fixture", g["costs"])
    if K > 1:
        np.testing.assert_allclose(ev, g["costs"], rtol=1e-3)  # (bilinear in factors held to 1e-4)
    else:
        assert ev == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_call_by_call_iterate_and_fit(cmf, name):
    """The three ways to run a fit each meet the fixture, and agree with each other bit for bit; the penalties' kernels run."""
    g = load(name)
    ref = (g["W"], g["H"], g["loss_hist"])
    c = {}
    a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["weights"], g["max_itr"], g["reg"], how="calls", counters=c)
    check_against(a, ref, f"{name} calls")
    assert c["xortho_launches"] > 0 and c["small_k_fused_h_updates"] == 0 and c["speculated_contractions"] == 0
    for how in ("iterate", "fit"):
        b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["weights"], g["max_itr"], g["reg"], how=how)
        check_against(b, ref, f"{name} {how}")
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", [f"mu_xortho_{s}_{w}" for s in ("k5", "k32") for w in xr.WEIGHT_SETS])
def test_eval_mode_updates_H_only(cmf, name):
    g = load(name)
    Wr, Hr, lr = xr.fit(g["data"], g["W0"], g["H0"], *g["weights"], max_itr=3, eval_mode=True)
    np.testing.assert_array_equal(Wr, g["W0"])
    for how in ("iterate", "fit", "calls"):
        got = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["weights"], 3, how=how, eval_mode=True)
        np.testing.assert_array_equal(got[0], g["W0"])  # (W0 is exact in float32: eval_mode leaves W bitwise unchanged)
        check_against(got, (g["W0"], Hr, lr), f"{name} eval_mode {how}")


@pytest.mark.parametrize("weights", [(0.02, 0.0, 0.0), (0.0, 0.01, 0.0), (0.0, 0.0, 0.1)], ids=["lambda", "lambda_H", "lambda_W"])
@pytest.mark.parametrize("shape", ["small", "k33"])
def test_each_weight_alone(cmf, shape, weights):
    """One weight at a time (the other sides launch nothing of their own), call by call, pipelined and with H alone."""
    g = load(f"mu_xortho_{shape}_x")
    ref = xr.fit(g["data"], g["W0"], g["H0"], *weights, max_itr=4)
    for how in ("calls", "iterate"):
        check_against(gpu_fit(cmf, g["data"], g["W0"], g["H0"], weights, 4, how=how), ref, f"{shape} {weights} {how}")
    ref = xr.fit(g["data"], g["W0"], g["H0"], *weights, max_itr=4, eval_mode=True)
    check_against(gpu_fit(cmf, g["data"], g["W0"], g["H0"], weights, 4, eval_mode=True), ref, f"{shape} {weights} eval_mode")


# ---- weights zero ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["k5", "small", "k32", "k33"])
@pytest.mark.parametrize("how", ["calls", "iterate"])
def test_zero_weights_are_the_plain_rule_bit_for_bit(cmf, shape, how):
    g = load(f"mu_xortho_{shape}_x")
    ca, cb = {}, {}
    a = gpu_fit(cmf, g["data"], g["W0"], g["H0"], None, 5, how=how, counters=ca)  # never called cmf_mu_set_xortho
    b = gpu_fit(cmf, g["data"], g["W0"], g["H0"], (0.0, 0.0, 0.0), 5, how=how, counters=cb)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # (the counters are read before xortho_cost, which launches the penalties' kernels by itself)
    assert ca["xortho_launches"] == 0 and cb["xortho_launches"] == 0
    assert ca["small_k_fused_h_updates"] == cb["small_k_fused_h_updates"] and ca["speculated_contractions"] == cb["speculated_contractions"]
    if how == "calls":
        assert ca["speculated_contractions"] > 0  # (the fusions are on: the plain path speculates)
    # weights, one penalised iteration, the initial factors again, zeros: the same bits as the handle that never had weights
    rule = cmf.MultUpdate(g["data"], g["W0"], g["H0"])
    try:
        rule.set_xortho(*xr.WEIGHT_SETS["all"])
        rule.iterate(1)
        assert rule.counter("xortho_launches") > 0
        rule.upload(g["W0"], g["H0"])
        rule.set_xortho(0.0)
        before = rule.counter("xortho_launches")
        if how == "iterate":
            lh = [rule.compute_loss()] + list(rule.iterate(5))
        else:
            lh = [rule.compute_loss()]
            for _ in range(5):
                rule.update_motifs()
                lh.append(rule.update_feature_maps())
        assert rule.counter("xortho_launches") == before
        for x, y in zip(a, rule.download() + (np.asarray(lh),)):
            np.testing.assert_array_equal(x, y)
    finally:
        rule.close()


# ---- behaviour -------------------------------------------------------------------------------------------------------------------
def test_the_penalty_kills_surplus_components(cmf):
    g = load(xr.PLANTED)
    cp, c0 = {}, {}
    Wp, Hp, _ = gpu_fit(cmf, g["data"], g["W0"], g["H0"], g["weights"], g["max_itr"], counters=cp)
    gpu_fit(cmf, g["data"], g["W0"], g["H0"], (0.0, 0.0, 0.0), g["max_itr"], counters=c0)
    print("x-ortho cost", cp["costs"][0], "of", c0["costs"][0], "=", cp["costs"][0] / c0["costs"][0])
    assert cp["costs"][0] <= 0.5 * c0["costs"][0]
    dead = xr.dead_components(g["W"], g["H"])
    assert dead >= 1 and xr.dead_components(Wp, Hp) == dead


def test_xortho_sweep(cmf):
    g = load("mu_xortho_small_x")
    K, N, L = g["W0"].shape
    out = cmf.xortho_sweep(g["data"], xr.SWEEP_LAMBDAS, L, K, max_itr=100, check_convergence=False, W_init=g["W0"], H_init=g["H0"])
    assert list(out) == list(xr.SWEEP_LAMBDAS)
    loss = [out[lam]["loss"] for lam in xr.SWEEP_LAMBDAS]
    cost = [out[lam]["xortho"] for lam in xr.SWEEP_LAMBDAS]
    print("loss", loss, "xortho", cost)
    assert np.all(np.diff(loss) >= 0) and np.all(np.diff(cost) <= 0)
    for lam in xr.SWEEP_LAMBDAS:
        assert out[lam]["res"].loss_hist[-1] == out[lam]["loss"] and len(out[lam]["res"].loss_hist) == 101


# ---- refusals and arguments ------------------------------------------------------------------------------------------------------
def test_refusals_and_arguments(cmf):
    g = load("mu_xortho_small_x")
    data, W0, H0 = g["data"] + 1.0, g["W0"], g["H0"]  # (strictly positive: the Itakura-Saito form is installed below)
    N, T = data.shape
    check = cmf.host.check
    rule = cmf.MultUpdate(data, W0, H0)
    lib, h = rule._lib, rule._h
    for bad in ((-1e-3, 0, 0), (0, -1.0, 0), (0, 0, float("nan")), (float("inf"), 0, 0), (0, float("-inf"), 0)):
        with pytest.raises(cmf.CMFError) as ei:
            check(lib.cmf_mu_set_xortho(h, *[float(v) for v in bad]))
        assert ei.value.code == 1, bad
    assert lib.cmf_mu_set_xortho(None, 0.1, 0.0, 0.0) == 1
    assert lib.cmf_mu_xortho_cost(None, None, None, None) == 1 and lib.cmf_mu_xortho_terms(None, None, None, None, None) == 1
    # ... and the handle is still the plain rule
    fresh = cmf.MultUpdate(data, W0, H0)
    np.testing.assert_array_equal(fresh.iterate(2), rule.iterate(2))
    fresh.close()
    rule.upload(W0, H0)

    installs = [("mask", lambda r: r.set_mask(np.ones((N, T))), lambda r: r.set_mask(None), "mask"),
                ("kl", lambda r: r.set_divergence(":kl"), lambda r: r.set_divergence(":square"), "divergence"),
                ("is", lambda r: r.set_divergence(":itakura_saito"), lambda r: r.set_divergence(":square"), "divergence"),
                ("beta", lambda r: r.set_divergence(":beta", beta=0.5), lambda r: r.set_divergence(":square"), "divergence"),
                ("gram", lambda r: r.set_option("gram", 1), lambda r: r.set_option("gram", 0), "Gram")]
    for what, install, remove, word in installs:
        for weights in ((0.1, 0, 0), (0, 0.1, 0), (0, 0, 0.1)):
            install(rule)  # the form first, the weights second
            with pytest.raises(cmf.CMFError, match=word) as ei:
                rule.set_xortho(*weights)
            assert ei.value.code == 4, (what, weights)
            rule.set_xortho(0.0)  # (zeros are always accepted)
            remove(rule)
            rule.set_xortho(*weights)  # the weights first, the form second
            with pytest.raises(cmf.CMFError, match="cmf_mu_set_xortho") as ei:
                install(rule)
            assert ei.value.code == 4, (what, weights)
            rule.set_xortho(0.0)
    # the weights survive cmf_set_factors: the next update is the penalised one of a fresh handle
    w = xr.WEIGHT_SETS["all"]
    rule.set_xortho(*w)
    rule.upload(W0, H0)
    got = list(rule.iterate(2)) + list(rule.download())
    assert rule.counter("xortho_launches") > 0
    fresh = cmf.MultUpdate(data, W0, H0)
    fresh.set_xortho(*w)
    want = list(fresh.iterate(2)) + list(fresh.download())
    fresh.close()
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    rule.close()
    group = cmf.MultUpdate(data, W0, H0, devices=[0, 0])
    with pytest.raises(cmf.CMFError) as ei:
        group.set_xortho(0.1)
    assert ei.value.code == 4
    group.set_xortho(0.0)
    group.close()
    for alg in (":hals", ":pgd"):
        with pytest.raises(NotImplementedError, match="alg=:mult"):
            cmf.fit_cnmf(data, L=8, K=4, alg=alg, lambda_xortho=0.1, max_itr=2)
    with pytest.raises(ValueError, match="finite and >= 0"):
        cmf.fit_cnmf(data, L=8, K=4, alg=":mult", lambda_xortho=-0.1, max_itr=2)
