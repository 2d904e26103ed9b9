"""CPU tests of the Itakura-Saito form of the MU rule: the fp64 restatement tests/is_mu_restatement.py (the executable definition of
what the library's CMF_DIV_IS computes), its committed fixtures, and the host-side refusals that are raised before anything touches
a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import is_mu_restatement as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(6, 40, 2, 3), (20, 7, 2, 10), (48, 300, 4, 8)]  # (N, T, K, L)
FIXTURES = ["mu_is_small", "mu_is_small_reg", "mu_is_k5", "mu_is_k33", "mu_is_k32", "mu_is_short", "mu_is_l40"]


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


def problem(N, T, K, L, seed):
    data, W0, H0 = ir.positive_problem(N, T, K, L, seed)
    return tuple(np.asarray(a, dtype=np.float64) for a in (data, W0, H0))


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_loss_never_increases_over_100_iterations(N, T, K, L):
    """l1 = l2 = 0: with the exponent 1/2 the multiplicative update of the Itakura-Saito divergence is monotone."""
    data, W0, H0 = problem(N, T, K, L, seed=11)
    W, H, lh = ir.fit_is(data, W0, H0, max_itr=100)
    assert len(lh) == 101 and np.isfinite(lh).all() and np.isfinite(W).all() and np.isfinite(H).all()
    steps = np.diff(lh)
    print(f"({N},{T},{K},{L}): loss {lh[0]:.6g} -> {lh[-1]:.6g}, largest step {steps.max():.3e}")
    assert np.all(steps <= 0), steps.max()
    assert W.min() >= ir.EPS and H.min() >= ir.EPS and lh[-1] >= 0.0


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_a_perfect_fit_is_a_fixed_point(N, T, K, L):
    """data = tensor_conv(W, H) + eps: r is all ones, P = Q, the numerators are the denominators, and an iteration leaves W and H
    where they were; the loss is 0."""
    rng = np.random.default_rng(5)
    W0, H0 = rng.random((K, N, L)) + 0.1, rng.random((K, T)) + 0.1
    data = ir.tensor_conv(W0, H0) + ir.EPS
    W, H, lh = ir.fit_is(data, W0, H0, max_itr=1)
    live = min(L, T)  # (lags l >= T never enter est: their numerators are 0 and W falls to eps there)
    if L > T:
        assert np.all(W[:, :, T:] == ir.EPS)
    dW = np.abs(W[:, :, :live] - W0[:, :, :live]).max() / np.abs(W0).max()
    dH = np.abs(H - H0).max() / np.abs(H0).max()
    print(f"({N},{T},{K},{L}): dW {dW:.2e} dH {dH:.2e} loss {lh}")
    assert dW < 1e-12 and dH < 1e-12
    assert abs(lh[0]) < 1e-24 and abs(lh[1]) < 1e-24


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_scale_invariance(N, T, K, L):
    """c data from sqrt(c) W0, sqrt(c) H0 gives the same loss_hist: the divergence depends on data ./ e alone."""
    data, W0, H0 = problem(N, T, K, L, seed=12)
    c = 7.3
    _, _, lh = ir.fit_is(data, W0, H0, max_itr=100)
    Wc, Hc, lhc = ir.fit_is(c * data, np.sqrt(c) * W0, np.sqrt(c) * H0, max_itr=100)
    np.testing.assert_allclose(lhc, lh, rtol=1e-9)


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_update_with_regularisers_is_the_formula(N, T, K, L):
    """Element for element, from loops over the definition (no shared code with the restatement's contractions)."""
    data, W0, H0 = problem(N, T, K, L, seed=13)
    l1W, l2W, l1H, l2H = 0.1, 0.5, 0.1, 0.2
    eps = ir.EPS

    def est_of(W, H):
        e = np.zeros((N, T))
        for l in range(L):
            for t in range(l, T):
                e[:, t] += W[:, :, l].T @ H[:, t - l]
        return e + eps

    e = est_of(W0, H0)
    Q = 1.0 / e
    P = (data * Q) * Q
    num, den = np.zeros((K, N, L)), np.zeros((K, N, L))
    for l in range(L):
        for t in range(l, T):
            num[:, :, l] += np.outer(H0[:, t - l], P[:, t])
            den[:, :, l] += np.outer(H0[:, t - l], Q[:, t])
    Wn = np.maximum(eps, W0 * np.sqrt(num / (den + l1W + 2 * l2W * W0 + eps)))
    W = W0.copy()
    ir.update_motifs(data, W, H0.copy(), l1W=l1W, l2W=l2W)
    np.testing.assert_allclose(W, Wn, rtol=1e-12, atol=0)
    e = est_of(W, H0)
    Q = 1.0 / e
    P = (data * Q) * Q
    numH, denH = np.zeros((K, T)), np.zeros((K, T))
    for l in range(L):
        for t in range(T - l):
            numH[:, t] += W[:, :, l] @ P[:, t + l]
            denH[:, t] += W[:, :, l] @ Q[:, t + l]
    Hn = np.maximum(eps, H0 * np.sqrt(numH / (denH + l1H + 2 * l2H * H0 + eps)))
    H = H0.copy()
    loss = ir.update_feature_maps(data, W, H, l1H=l1H, l2H=l2H)
    np.testing.assert_allclose(H, Hn, rtol=1e-12, atol=0)
    r = data / est_of(W, Hn)
    assert abs(loss - np.sum((r - 1) - np.log(r)) / (N * T)) <= 1e-12 * loss


def test_data_checks():
    ok = np.full((3, 4), 2.0)
    assert ir.check_data(ok) is not None
    for bad in (0.0, -1.0, np.nan, np.inf):
        x = ok.copy()
        x[1, 2] = bad
        with pytest.raises(ValueError, match="Itakura-Saito divergence needs"):
            ir.check_data(x)
        with pytest.raises(ValueError, match="Itakura-Saito divergence needs"):
            ir.fit_is(x, np.ones((2, 3, 2)), np.ones((2, 4)), max_itr=1)


def test_float32_model_stays_close():
    """The cdtype / edtype switches model the device: one iteration differs from fp64 at float32 level, not more."""
    data, W0, H0 = problem(48, 300, 4, 8, seed=2)
    W, H, lh = ir.fit_is(data, W0, H0, max_itr=1)
    W32, H32, lh32 = ir.fit_is(data, W0, H0, max_itr=1, cdtype=np.float32, edtype=np.float32)
    assert 0 < np.linalg.norm(W32 - W) / np.linalg.norm(W) < 1e-5
    assert 0 < np.linalg.norm(H32 - H) / np.linalg.norm(H) < 1e-5
    assert abs(lh32[-1] - lh[-1]) < 1e-5 * lh[-1]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_current(name):
    """The committed fixture is what the restatement computes today, and stays within the size agreed for golden files."""
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 250_000
    g = ir.load_fixture(path)
    W, H, lh = ir.fit_is(g["data"], g["W0"], g["H0"], max_itr=g["max_itr"], **g["reg"])
    rtol = 1e-12 if g["exact"] else 1e-7  # (W32 / H32: stored rounded to float32, 6e-8 relative)
    np.testing.assert_allclose(W, g["W"], rtol=rtol, atol=0)
    np.testing.assert_allclose(H, g["H"], rtol=rtol, atol=0)
    np.testing.assert_allclose(lh, g["loss_hist"], rtol=1e-12)
    assert len(lh) == g["max_itr"] + 1 and g["data"].min() > 0
    if name == "mu_is_small_reg":
        assert all(v > 0 for v in g["reg"].values())  # all four regularisers
    else:
        assert np.all(np.diff(lh) <= 0.0)


def test_fixture_counts_are_admitted():
    """Every fixture was written at a count profiles/mu_is_precision.txt admits."""
    adm = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_is_precision.txt")):
        if line.startswith("admit "):
            adm[line.split()[1]] = int(line.split()[2])
    for name in FIXTURES:
        assert int(np.load(os.path.join(GOLDEN, name + ".npz"))["max_itr"]) <= adm[name], name
    assert adm["synthetic(130,700,32,20)"] >= 100 and adm["synthetic(250,2000,5,20)"] >= 100  # (the two mid-size fits of the GPU test)


def test_spellings(cmf):
    from cmf_jl_amd import host

    assert host._divergence_kind(":itakura_saito") == 2 and host._divergence_kind("itakura_saito") == 2
    assert host._divergence_kind(":kl") == 1 and host._divergence_kind(":square") == 0
    for bad in (":is", ":itakura", "is"):
        with pytest.raises(ValueError, match="':square' or ':kl'"):
            host._divergence_kind(bad)


def test_host_refusals_name_their_reason(cmf):
    """Raised before anything touches a device: no GPU needed."""
    data = np.random.default_rng(0).random((6, 40)) + 0.1
    for alg in (":hals", ":pgd", ":admm", cmf.ANLSUpdate, ":sep"):
        with pytest.raises(NotImplementedError, match="alg=:mult"):
            cmf.fit_cnmf(data, L=3, K=2, alg=alg, divergence=":itakura_saito")
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":itakura_saito", mask=np.ones((6, 40)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":itakura_saito", devices=[0, 0])
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.cross_validate(data, [3], [2], divergence=":itakura_saito")
    res = cmf.CNMF_results(data, np.ones((2, 6, 3)), np.ones((2, 40)), np.zeros(1), np.zeros(1))
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.evaluate_heldout(res, np.ones((6, 40)), divergence=":itakura_saito")
    with pytest.raises(ValueError, match="':square' or ':kl'"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":is")


def test_constant_is_declared_and_bound(cmf):
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert re.search(r"#define CMF_DIV_IS 2\b", header)
    julia = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert re.search(r"const CMF_DIV_IS = 2\b", julia) and ":itakura_saito" in julia
    assert "`CMF_DIV_IS`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert lib.cmf_abi_version() == 6  # nothing is added but a constant
    buf = ctypes.create_string_buffer(4096)
    assert lib.cmf_option_names(buf, 4096) == 0 and b"is_div" not in buf.value


def test_restatement_is_test_infrastructure_only():
    """Nothing under cmf.jl_amd/, include/ or bench.py imports the restatement."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("cmf.jl_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(d, f) for f in files if f.endswith((".py", ".h", ".hip", ".jl"))]
    for p in paths:
        assert "is_mu_restatement" not in open(p, errors="replace").read(), p
