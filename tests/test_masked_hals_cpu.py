"""CPU checks of the HALS rule under a mask by imputation (library option "hals_mask"): the fp64 restatement
(tests/masked_hals_restatement.py) against the oracle's HALS and against its own invariants, the host-side refusals, and mu_refusal
(cmf.jl_amd/csrc/cmf_mu_install.h) compiled stand-alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hals_gram_form as gf
import masked_hals_restatement as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


def rand_problem(seed, N, T, K, L):
    rng = np.random.default_rng(seed)
    return rng.random((K, N, L)), rng.random((K, T)), rng.random((N, T))


@pytest.mark.parametrize("N,T,K,L", [(24, 90, 3, 5), (13, 40, 5, 7), (6, 3, 2, 5)])
@pytest.mark.parametrize("reg", [dict(), REG])
def test_all_ones_mask_is_the_oracles_hals_bit_for_bit(oracle, N, T, K, L, reg):
    W0, H0, data = rand_problem(3, N, T, K, L)
    Wr, Hr, lr, _ = oracle.fit_hals(data, W0, H0, max_itr=3, check_convergence=False, **reg)
    W, H, lh = hr.masked_hals_fit(oracle, data, np.ones((N, T)), W0, H0, max_itr=3, **reg)
    np.testing.assert_array_equal(W, Wr)
    np.testing.assert_array_equal(H, Hr)
    np.testing.assert_array_equal(lh, lr)


@pytest.mark.parametrize("reg", [dict(), REG])
def test_the_half_steps_are_the_oracles_on_the_imputed_data(oracle, reg):
    """masked_hals_half_W / _H against the oracle's half-steps called on X~ = where(M, X, conv(W, H)) formed here."""
    N, T, K, L = 20, 70, 3, 6
    W0, H0, data = rand_problem(5, N, T, K, L)
    mask = hr.block_mask(N, T, 0.3, 1, 2)
    Xt = np.where(mask != 0, data, oracle.tensor_conv(W0, H0))
    Wr, Hr = W0.copy(), H0.copy()
    oracle.hals_update_motifs(oracle.HALSUpdate(Xt, Wr, Hr), Xt, Wr, Hr, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
    W = hr.masked_hals_half_W(oracle, data, mask, W0.copy(), H0, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
    np.testing.assert_array_equal(W, Wr)
    Xt = np.where(mask != 0, data, oracle.tensor_conv(Wr, H0))
    oracle.hals_update_feature_maps(oracle.HALSUpdate(Xt, Wr, Hr), Xt, Wr, Hr, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0))
    H = H0.copy()
    loss = hr.masked_hals_half_H(oracle, data, mask, Wr, H, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0))
    np.testing.assert_array_equal(H, Hr)
    assert loss == pytest.approx(hr.masked_loss(oracle, data, mask, Wr, Hr), rel=1e-12)


@pytest.mark.parametrize("reg", [dict(), REG])
def test_the_three_ways_to_run_it_agree(oracle, reg):
    """The carried residual, the residual formed afresh in front of each half-update, the C oracle's half-updates and the
    Gram-projected sweeps in fp64 (the model of tools/hals_masked_precision.py): one rule, to rounding."""
    N, T, K, L = 24, 90, 3, 5
    W0, H0, data = rand_problem(6, N, T, K, L)
    mask = hr.block_mask(N, T, 0.2, L, 4)
    a = hr.masked_hals_fit(oracle, data, mask, W0, H0, max_itr=4, **reg)
    b = hr.masked_hals_fit(oracle, data, mask, W0, H0, max_itr=4, carried=False, **reg)
    c = hr.masked_hals_fit(oracle, data, mask, W0, H0, max_itr=4, use_c=True, **reg)
    for other in (b, c):
        for x, y in zip(a, other):
            np.testing.assert_allclose(y, x, rtol=1e-9, atol=1e-12)
    W, H, ls = W0.copy(), H0.copy(), []
    for _ in range(4):
        W, H, loss = hr.f32_iteration(oracle, gf, data, mask, W, H, reg.get("l1W", 0), reg.get("l2W", 0), reg.get("l1H", 0), reg.get("l2H", 0), np.float64)
        ls.append(loss)
    np.testing.assert_allclose(W, a[0], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(H, a[1], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(ls, a[2][1:], rtol=1e-9)


@pytest.mark.parametrize("mname,frac,block", [("30% speckle", 0.3, 1), ("20% in blocks of L", 0.2, 6)])
def test_loss_is_non_increasing_without_regularisers(oracle, mname, frac, block):
    """Every HALS step minimises a block of the surrogate norm(X~ - conv)^2 exactly, and the surrogate majorises the masked loss with
    equality at the point of imputation: 30 iterations, slack 1e-12 relative (fp64; exact block minimisation allows no more)."""
    N, T, K, L = 30, 160, 3, 6
    W0, H0, data = rand_problem(9, N, T, K, L)
    mask = hr.block_mask(N, T, frac, block, 4)
    assert 0.5 * frac < 1.0 - mask.mean() < 1.5 * frac
    _, _, lh = hr.masked_hals_fit(oracle, data, mask, W0, H0, max_itr=30)
    assert len(lh) == 31 and np.all(np.diff(lh) <= 1e-12 * lh[:-1]), np.diff(lh).max()
    assert lh[-1] < 0.9 * lh[0]


@pytest.mark.parametrize("carried", [True, False])
def test_values_at_held_out_entries_do_not_matter(oracle, carried):
    N, T, K, L = 20, 70, 3, 6
    W0, H0, data = rand_problem(7, N, T, K, L)
    for mask in hr.masks(N, T, L).values():
        a = hr.masked_hals_fit(oracle, data, mask, W0, H0, max_itr=3, carried=carried, **REG)
        data_nan = hr.garbage(data, mask)
        assert np.isnan(data_nan).any() and np.isinf(data_nan).any() and np.array_equal(data_nan[mask != 0], data[mask != 0])
        b = hr.masked_hals_fit(oracle, data_nan, mask, W0, H0, max_itr=3, carried=carried, **REG)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert np.isfinite(b[2]).all()


def test_host_refusals_come_before_any_device_work(cmf):
    data = np.random.default_rng(0).random((6, 40))
    mask = np.ones((6, 40))
    with pytest.raises(NotImplementedError, match="no masked form") as ei:
        cmf.fit_cnmf(data, L=3, K=2, alg=":hals", mask=mask)
    assert "unless options={'hals_mask': 1}" in str(ei.value)
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":hals", mask=mask, options={"hals_mask": 0})
    for alg in (":admm", cmf.ANLSUpdate, ":sep"):  # the option is the HALS rule's alone
        with pytest.raises(NotImplementedError, match="no masked form"):
            cmf.fit_cnmf(data, L=3, K=2, alg=alg, mask=mask, options={"hals_mask": 1})
    with pytest.raises(TypeError, match="draws its own masks"):
        cmf.cross_validate(data, [3], [2], alg=":hals")
    with pytest.raises(TypeError, match="draws its own masks"):
        cmf.cross_validate(data, [3], [2], alg=":pgd", options={"hals_mask": 1})
    with pytest.raises(TypeError, match="draws its own masks"):
        cmf.cross_validate(data, [3], [2], alg=":hals", options={"hals_mask": 1}, mask=mask)
    with pytest.raises(ValueError, match="0 and 1 only"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":hals", mask=0.5 * mask, options={"hals_mask": 1})


@pytest.fixture(scope="module")
def refusals(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx, "a host C++ compiler (g++ or clang++) is needed: a missing tool is a failure, not a skip"
    exe = str(tmp_path_factory.mktemp("hals_mask") / "hals_mask_refusal")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "cmf.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "hals_mask_refusal.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    assert p.stderr.startswith("ok "), p.stderr
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    cells = {}
    for line in p.stdout.splitlines():
        key, code, msg = line.split("\t")
        rule, form, gates, hm = key.split("|")
        cells[(rule, form, gates, int(hm))] = (int(code), msg)
    return cells


def test_mu_refusal_lets_hals_run_under_a_mask_iff_the_option_is_on(refusals):
    CMF_OK, CMF_ERR_STATE = 0, 3
    assert len(refusals) == 8 * 8 * 2 * 2
    for (rule, form, gates, hm), (code, msg) in refusals.items():
        div, masked = form.split("+")[0], form.endswith("+mask")
        if div != "square":  # a divergence installed: refused whatever the option says
            assert code == CMF_ERR_STATE, (rule, form, gates, hm)
            if not (rule == "HALS" and masked and not hm):
                assert "this rule minimises the squared error only" in msg
        elif rule == "HALS" and masked:
            assert (code == CMF_OK) == bool(hm), (form, gates, hm)
            if not hm:
                assert "HALS rule has no masked form" in msg and "clear it first" in msg
        else:
            assert code == CMF_OK, (rule, form, gates, hm)
        if rule == "PGD":  # the option is nothing to the PGD rule
            assert (code, msg) == refusals[(rule, form, gates, 1 - hm)]
