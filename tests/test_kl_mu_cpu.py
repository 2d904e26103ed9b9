"""CPU checks of the KL form of the MU rule: the fp64 restatement (tests/kl_mu_restatement.py) against its own invariants -- the
divergence never increases, a perfect fit is a fixed point, the denominators are the contractions of all ones --, the committed
fixtures, the host-side refusals, and the new C entry in every binding table."""
import ctypes
import os
import re

import numpy as np
import pytest

import kl_mu_restatement as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the six shapes the rule's condition (a non-increasing loss) was stated on: (N, T, K, L)
SHAPES = [(60, 400, 3, 8), (100, 700, 5, 10), (70, 300, 33, 6), (96, 1000, 32, 12), (20, 7, 2, 10), (45, 130, 16, 40)]
FIXTURES = ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_k33", "mu_kl_k32", "mu_kl_short", "mu_kl_l40"]


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_loss_never_increases_over_100_iterations(N, T, K, L):
    """l1 = l2 = 0: the multiplicative update of the KL divergence is monotone.  Data with up to 30 % exact zeros and one all-zero
    unit; everything stays finite, and the all-zero unit's motif entries fall to eps."""
    data, W0, H0 = kr.synthetic(N, T, K, L, seed=11)
    assert (data == 0).mean() > 0.25 and not data[N // 2].any()
    W, H, lh = kr.fit_kl(data, W0, H0, max_itr=100)
    assert len(lh) == 101 and np.isfinite(lh).all() and np.isfinite(W).all() and np.isfinite(H).all()
    steps = np.diff(lh)
    print(f"({N},{T},{K},{L}): loss {lh[0]:.6g} -> {lh[-1]:.6g}, largest step {steps.max():.3e}")
    assert np.all(steps <= 0.0), steps.max()
    assert np.all(W[:, N // 2, :] == kr.EPS)
    assert W.min() >= kr.EPS and H.min() >= kr.EPS


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_a_perfect_fit_is_a_fixed_point(N, T, K, L):
    """data = tensor_conv(W, H): R is all ones (up to eps), the numerators are the denominators, one iteration leaves W and H
    where they were -- to a few ulps of the sums involved -- and the loss is 0."""
    rng = np.random.default_rng(5)
    W0, H0 = rng.random((K, N, L)) + 0.1, rng.random((K, T)) + 0.1
    data = kr.tensor_conv(W0, H0)
    W, H, lh = kr.fit_kl(data, W0, H0, max_itr=1)
    live = min(L, T)  # (lags l >= T never enter est: their numerators and denominators are 0 and W falls to eps there)
    if L > T:
        assert np.all(W[:, :, T:] == kr.EPS)
    dW = np.abs(W[:, :, :live] - W0[:, :, :live]).max() / np.abs(W0).max()
    dH = np.abs(H - H0).max() / np.abs(H0).max()
    print(f"({N},{T},{K},{L}): dW {dW:.2e} dH {dH:.2e} loss {lh}")
    # a sum of up to T (numW) or N L (numH) terms in fp64 against the same sum in another order: a few eps sqrt(terms)
    assert dW < 1e-14 and dH < 1e-14
    assert abs(lh[0]) < 1e-14 and abs(lh[1]) < 1e-13


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_denominators_are_the_contractions_of_all_ones(N, T, K, L):
    """denomW and denomH are what mult.jl:33 and :48 give with est replaced by all ones -- through the restatement's own hxt and
    tensor_transconv."""
    rng = np.random.default_rng(6)
    W, H = rng.random((K, N, L)), rng.random((K, T))
    dW1, dH1 = kr.ones_denominators(W, H, N)
    np.testing.assert_allclose(kr.denom_W(H, N, L), dW1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(kr.denom_H(W, T), dH1, rtol=1e-12, atol=0)
    if L > T:
        assert not kr.denom_W(H, N, L)[:, :, T:].any()


def test_divergence_select_and_data_checks():
    x = np.array([[0.0, 2.0], [3.0, 0.0]])
    e = np.array([[0.5, 2.0], [1.0, 4.0]])
    want = (0 - 0 + 0.5) + (0 - 2 + 2) + (3 * np.log(3.0) - 3 + 1) + (0 - 0 + 4)
    assert abs(kr.divergence(x, e) - want) < 1e-15
    for bad in (np.array([[1.0, -1.0]]), np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]]), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            kr.check_data(bad)


def test_float32_contractions_stay_close():
    """The cdtype switch models the device: one iteration differs from fp64 at float32 level, not more."""
    data, W0, H0 = kr.synthetic(60, 400, 3, 8, seed=2)
    W, H, lh = kr.fit_kl(data, W0, H0, max_itr=1)
    W32, H32, lh32 = kr.fit_kl(data, W0, H0, max_itr=1, cdtype=np.float32)
    assert 0 < np.linalg.norm(W32 - W) / np.linalg.norm(W) < 1e-5
    assert 0 < np.linalg.norm(H32 - H) / np.linalg.norm(H) < 1e-5
    assert abs(lh32[-1] - lh[-1]) < 1e-5 * lh[-1]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_current(name):
    """The committed fixture is what the restatement computes today, and stays within the size agreed for golden files."""
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 250_000
    g = kr.load_fixture(path)
    W, H, lh = kr.fit_kl(g["data"], g["W0"], g["H0"], max_itr=g["max_itr"], **g["reg"])
    rtol = 1e-10 if g["exact"] else 1e-7  # (W32 / H32: stored rounded to float32, 6e-8 relative)
    np.testing.assert_allclose(W, g["W"], rtol=rtol, atol=1e-14)
    np.testing.assert_allclose(H, g["H"], rtol=rtol, atol=1e-14)
    np.testing.assert_allclose(lh, g["loss_hist"], rtol=1e-10)
    assert len(lh) == g["max_itr"] + 1 and (g["data"] == 0).any()
    if name == "mu_kl_small_reg":
        assert all(v > 0 for v in g["reg"].values())  # all four regularisers
    if name != "mu_kl_small_reg":
        assert np.all(np.diff(lh) <= 0.0)


def test_divergence_is_a_known_keyword(cmf):
    from cmf_jl_amd import host

    assert "divergence" in host._KNOWN_KW
    assert callable(cmf.evaluate_divergence) and callable(cmf.MultUpdate.set_divergence)
    assert host._divergence_kind(":kl") == 1 and host._divergence_kind(":square") == 0
    with pytest.raises(ValueError, match="':square' or ':kl'"):
        host._divergence_kind(":itakura")


def test_host_refusals_name_their_reason(cmf):
    """Raised before anything touches a device: no GPU needed."""
    data = np.random.default_rng(0).random((6, 40))
    for alg in (":hals", ":pgd", ":admm", cmf.ANLSUpdate, ":sep"):
        with pytest.raises(NotImplementedError, match="alg=:mult"):
            cmf.fit_cnmf(data, L=3, K=2, alg=alg, divergence=":kl")
    with pytest.raises(NotImplementedError, match="mask="):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":kl", mask=np.ones((6, 40)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":kl", devices=[0, 0])
    with pytest.raises(ValueError, match="':square' or ':kl'"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":is")


def test_new_entry_is_exported_and_bound(cmf):
    assert "cmf_mu_set_divergence" in cmf.SYMBOLS
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert hasattr(lib, "cmf_mu_set_divergence")
    assert lib.cmf_abi_version() == 6  # the entry is additive
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert re.search(r"int cmf_mu_set_divergence\(cmf_handle h, int kind\);", header)
    assert re.search(r"#define CMF_DIV_SQUARE 0\b", header) and re.search(r"#define CMF_DIV_KL 1\b", header)
    julia = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert "(:cmf_mu_set_divergence, LIBCMF)" in julia and "function set_divergence!(" in julia
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`cmf_mu_set_divergence`" in integ


def test_restatement_is_test_infrastructure_only():
    """Nothing under cmf.jl_amd/, include/ or bench.py imports the restatement."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("cmf.jl_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(d, f) for f in files if f.endswith((".py", ".h", ".hip", ".jl"))]
    for p in paths:
        assert "kl_mu_restatement" not in open(p, errors="replace").read(), p
