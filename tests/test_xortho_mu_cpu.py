"""CPU tests of seqNMF's cross-orthogonality penalties on the MU rule: the fp64 restatement tests/xortho_mu_restatement.py against the
objective it states, against the oracle's plain rule, the fixtures against profiles/mu_xortho_precision.txt, the behaviour the GPU test
asks for with margin, and the argument handling of the Python interface (raised before anything touches a device)."""
import ctypes
import os

import numpy as np
import pytest

import xortho_mu_restatement as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = [name for name, _, _ in xr.CASES]


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


def problem(N, T, K, L, seed):
    """Factors and data of order 1."""
    rng = np.random.default_rng(seed)
    return rng.random((N, T)) + 0.1, rng.random((K, N, L)) + 0.1, rng.random((K, T)) + 0.1


@pytest.mark.parametrize("N,T,K,L", [(6, 40, 3, 4), (5, 9, 4, 6), (4, 5, 2, 8), (7, 30, 5, 1)])
def test_terms_are_the_forward_differences_of_the_penalty(N, T, K, L):
    """The penalty part of the objective is linear in any single entry of W and of H, so its forward difference over a step of 1 is
    its partial derivative up to fp64 rounding: lam xW + lamW oW for W, lam xH + lamH oH for H (1e-9 relative)."""
    data, W, H = problem(N, T, K, L, seed=3)
    lam, lamH, lamW = 0.7, 0.3, 0.9
    xW, xH, oH, oW = xr.terms(data, W, H)
    p0 = xr.penalty(data, W, H, lam, lamH, lamW)
    rng = np.random.default_rng(4)
    for _ in range(12):
        k, n, l = rng.integers(K), rng.integers(N), rng.integers(L)
        W2 = W.copy()
        W2[k, n, l] += 1.0
        got = xr.penalty(data, W2, H, lam, lamH, lamW) - p0
        want = lam * xW[k, n, l] + lamW * oW[k, n, l]
        assert want > 0 and abs(got - want) <= 1e-9 * want, (k, n, l, got, want)
        k, t = rng.integers(K), rng.integers(T)
        H2 = H.copy()
        H2[k, t] += 1.0
        got = xr.penalty(data, W, H2, lam, lamH, lamW) - p0
        want = lam * xH[k, t] + lamH * oH[k, t]
        assert want > 0 and abs(got - want) <= 1e-9 * want, (k, t, got, want)
    # each weight alone picks out its own term
    for w, tW, tH in (((1.0, 0, 0), xW, xH), ((0, 1.0, 0), 0 * xW, oH), ((0, 0, 1.0), oW, 0 * xH)):
        p = xr.penalty(data, W, H, *w)
        W2, H2 = W.copy(), H.copy()
        W2[0, 1, 0] += 1.0
        H2[1, 2] += 1.0
        np.testing.assert_allclose(xr.penalty(data, W2, H, *w) - p, tW[0, 1, 0], rtol=1e-9, atol=1e-9 * abs(p))
        np.testing.assert_allclose(xr.penalty(data, W, H2, *w) - p, tH[1, 2], rtol=1e-9, atol=1e-9 * abs(p))


def test_costs_are_the_off_diagonal_sums_of_the_objective():
    data, W, H = problem(9, 33, 4, 5, seed=8)
    np.testing.assert_allclose(xr.costs(data, W, H), xr.costs_literal(data, W, H), rtol=1e-12)
    # S is seqNMF's conv2(., ones(1, 2L-1), 'same'); off the sum over the other components
    L = 5
    full = np.array([np.convolve(H[k], np.ones(2 * L - 1))[L - 1 : L - 1 + H.shape[1]] for k in range(H.shape[0])])
    np.testing.assert_allclose(xr.smooth(H, L), full, rtol=1e-12)
    np.testing.assert_allclose(xr.off(H), H.sum(axis=0)[None, :] - H, rtol=1e-12)
    assert np.all(xr.off(H[:1]) == 0.0)  # K = 1: off is empty


def test_sums_of_non_negative_terms_stay_non_negative_beside_a_dead_component():
    """A dead component at eps beside one of order 1: off and S of the restatement are exact sums, never rounding noise of either sign."""
    H = np.full((3, 50), xr.EPS)
    H[0] = 1.0 + np.random.default_rng(0).random(50)
    G = xr.off(xr.smooth(H, 6))
    assert np.all(G > 0) and G[0].max() < 1e-13


@pytest.mark.parametrize("N,T,K,L", [(12, 60, 3, 5), (8, 6, 2, 9)])
@pytest.mark.parametrize("reg", [{}, xr.REG])
def test_weights_zero_is_the_oracle_bit_for_bit(N, T, K, L, reg):
    from oracle import cmf_oracle as oc

    data, W0, H0 = problem(N, T, K, L, seed=21)
    W, H, lh = xr.fit(data, W0, H0, 0.0, 0.0, 0.0, max_itr=7, **reg)
    Wo, Ho, lo, _ = oc.fit_mult(data, W0, H0, max_itr=7, check_convergence=False, **reg)
    np.testing.assert_array_equal(W, Wo)
    np.testing.assert_array_equal(H, Ho)
    np.testing.assert_array_equal(lh, lo)


def test_every_fixture_was_written_at_an_admitted_count():
    adm = xr.admitted()
    assert sorted(adm) == sorted(FIXTURES)
    for name, s, wset in xr.CASES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert 1 <= int(g["max_itr"]) <= adm[name], (name, int(g["max_itr"]), adm[name])
        assert (float(g["lam"]), float(g["lamH"]), float(g["lamW"])) == xr.weights_of(s, wset)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 250_000
        _, (N, T, K, L), _, _, _, _ = xr.shape_row(s)
        assert g["data8"].shape == (N, T) and g["W0"].shape == (K, N, L) and g["H0"].shape == (K, T)
    # the shapes that make the windows and off go wrong
    shapes = {r[0]: r[1] for r in xr.SHAPES}
    assert shapes["l1"][3] == 1 and shapes["k1"][2] == 1 and shapes["edge"][1] == 2 * shapes["edge"][3] - 2 and shapes["short"][1] < shapes["short"][3]


def test_the_planted_fixture_kills_components_with_margin():
    """What tests/test_gpu_xortho_mu.py asks of the device -- an x-ortho cost of at most 0.5 x the lambda = 0 fit's from the same initial
    factors -- holds for the restatement with a factor 2 to spare, and at least one component dies."""
    g = xr.load_fixture(os.path.join(GOLDEN, xr.PLANTED + ".npz"))
    assert g["weights"] == (xr.LAM, 0.0, 0.0)
    W0f, H0f, _ = xr.fit(g["data"], g["W0"], g["H0"], max_itr=g["max_itr"])
    plain = xr.costs(g["data"], W0f, H0f)[0]
    pen = xr.costs(g["data"], g["W"], g["H"])[0]
    print("x-ortho cost", pen, "of", plain, "=", pen / plain, "dead", xr.dead_components(g["W"], g["H"]))
    np.testing.assert_allclose(pen, g["costs"][0], rtol=1e-9)
    assert pen <= 0.25 * plain
    assert xr.dead_components(g["W"], g["H"]) >= 1 and xr.dead_components(W0f, H0f) == 0


def test_the_sweep_lambdas_trade_loss_for_x_ortho_cost_strictly():
    data, W0, H0, _ = xr.inputs("small")
    loss, cost = [], []
    for lam in xr.SWEEP_LAMBDAS:
        W, H, lh = xr.fit(data, W0, H0, lam, max_itr=100)
        loss.append(lh[-1])
        cost.append(xr.costs(data, W, H)[0])
    assert np.all(np.diff(loss) > 0) and np.all(np.diff(cost) < 0), (loss, cost)


def test_host_argument_handling(cmf):
    """Raised before anything touches a device: no GPU needed."""
    data = np.random.default_rng(0).random((6, 40)) + 0.1
    for kw in (dict(lambda_xortho=-1e-3), dict(lambda_ortho_H=-1.0), dict(lambda_ortho_W=float("nan")), dict(lambda_xortho=float("inf"))):
        with pytest.raises(ValueError, match="finite and >= 0"):
            cmf.fit_cnmf(data, L=3, K=2, alg=":mult", **kw)
    for alg in (":hals", ":pgd", ":admm", cmf.ANLSUpdate, ":sep"):
        for kw in (dict(lambda_xortho=0.1), dict(lambda_ortho_H=0.1), dict(lambda_ortho_W=0.1)):
            with pytest.raises(NotImplementedError, match="alg=:mult"):
                cmf.fit_cnmf(data, L=3, K=2, alg=alg, **kw)
    for kw in (dict(mask=np.ones((6, 40))), dict(divergence=":kl"), dict(devices=[0, 0]), dict(options={"gram": 1})):
        with pytest.raises(NotImplementedError, match="squared-error MU rule on one GPU"):
            cmf.fit_cnmf(data, L=3, K=2, alg=":mult", lambda_xortho=0.1, **kw)
    with pytest.raises(TypeError, match="its own lambda_xortho"):
        cmf.xortho_sweep(data, [0.1], 3, 2, lambda_xortho=0.2)
    assert {"lambda_xortho", "lambda_ortho_H", "lambda_ortho_W"} <= set(cmf.host._META_KEYS)


def test_entries_are_exported_and_refuse_a_null_handle(cmf):
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert lib.cmf_abi_version() == 6  # additive entries
    lib.cmf_mu_set_xortho.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    assert lib.cmf_mu_set_xortho(None, 0.1, 0.0, 0.0) == 1  # CMF_ERR_ARG: handle is NULL (no device touched)
    lib.cmf_mu_xortho_cost.argtypes = [ctypes.c_void_p] * 4
    assert lib.cmf_mu_xortho_cost(None, None, None, None) == 1
    lib.cmf_mu_xortho_terms.argtypes = [ctypes.c_void_p] * 5
    assert lib.cmf_mu_xortho_terms(None, None, None, None, None) == 1
    for name in ("cmf_mu_set_xortho", "cmf_mu_xortho_cost", "cmf_mu_xortho_terms"):
        assert name in cmf.SYMBOLS


def test_save_model_carries_the_weights(cmf, tmp_path):
    res = cmf.CNMF_results(np.ones((3, 5)), np.ones((2, 3, 2)), np.ones((2, 5)), np.zeros(1), np.zeros(1))
    path = str(tmp_path / "m.npz")
    cmf.save_model(res, path, alg=":mult", lambda_xortho=0.02, lambda_ortho_H=0.005, lambda_ortho_W=0.05)
    _, meta = cmf.load_model(path)
    assert float(meta["lambda_xortho"]) == 0.02 and float(meta["lambda_ortho_H"]) == 0.005 and float(meta["lambda_ortho_W"]) == 0.05


def test_restatement_is_test_infrastructure_only():
    """Nothing under cmf.jl_amd/, include/ or bench.py imports the restatement."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("cmf.jl_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(d, f) for f in files if f.endswith((".py", ".h", ".hip", ".jl"))]
    for p in paths:
        assert "xortho_mu_restatement" not in open(p, errors="replace").read(), p
