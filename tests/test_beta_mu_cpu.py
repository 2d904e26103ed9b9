"""CPU tests of the beta-divergence form of the MU rule: the fp64 restatement tests/beta_mu_restatement.py (the executable definition
of what cmf_mu_set_beta_divergence computes), its committed fixtures, the window constant, and the host-side refusals that are raised
before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import beta_mu_restatement as br
import is_mu_restatement as ir
import kl_mu_restatement as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(6, 40, 2, 3), (20, 7, 2, 10), (48, 300, 4, 8)]  # (N, T, K, L)
BETAS = [0.25, 0.5, 1.5, 2.0, 3.0]  # the fixtures'
SHAPE_NAMES = ["small", "small_reg", "k5", "k33", "k32", "short", "l40"]
FIXTURES = ([f"mu_beta_{s}_{b}" for s in SHAPE_NAMES for b in ("b050", "b150")]
            + [f"mu_beta_{s}_{b}" for s in ("small", "short") for b in ("b025", "b200", "b300")])


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


def problem(N, T, K, L, seed):
    return tuple(np.asarray(a, dtype=np.float64) for a in br.count_problem(N, T, K, L, seed))


def profile_lines(key):
    return [line.split() for line in open(os.path.join(ROOT, "profiles", "mu_beta_precision.txt")) if line.startswith(key + " ")]


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_loss_never_increases_over_100_iterations(N, T, K, L, beta):
    """l1 = l2 = 0: with the exponent gamma(beta) the multiplicative update of the beta-divergence is monotone (counts with exact
    zeros: the x = 0 terms are in)."""
    data, W0, H0 = problem(N, T, K, L, seed=11)
    assert (data == 0).any()
    W, H, lh = br.fit_beta(data, W0, H0, beta, max_itr=100)
    assert len(lh) == 101 and np.isfinite(lh).all() and np.isfinite(W).all() and np.isfinite(H).all()
    steps = np.diff(lh)
    print(f"({N},{T},{K},{L}) beta={beta}: loss {lh[0]:.6g} -> {lh[-1]:.6g}, largest step {steps.max():.3e}")
    assert np.all(steps <= 0), steps.max()
    assert W.min() >= br.EPS and H.min() >= br.EPS and lh[-1] >= 0.0


def test_gamma_is_the_mm_exponent():
    assert br.gamma(0.5) == 1 / 1.5 and br.gamma(0.25) == 1 / 1.75 and br.gamma(3.0) == 0.5 and br.gamma(4.0) == 1 / 3
    assert br.gamma(1.0 + 1e-9) == 1.0 and br.gamma(1.5) == 1.0 and br.gamma(2.0) == 1.0


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_beta_2_is_the_squared_error_rule(N, T, K, L):
    """fit_beta(beta = 2) reproduces the factors of the oracle's MU rule to 1e-10, and its loss D = sum (x - e)^2 / 2 per entry maps to
    the oracle's norm(est - data) / norm(data) by sqrt(2 D) / norm(data)."""
    from oracle import cmf_oracle as oc

    data, W0, H0 = problem(N, T, K, L, seed=12)
    W, H, lh = br.fit_beta(data, W0, H0, 2.0, max_itr=20)
    Wo, Ho, lo, _ = oc.fit_mult(data, W0, H0, max_itr=20, check_convergence=False)
    np.testing.assert_allclose(W, Wo, rtol=1e-10, atol=1e-10 * np.abs(Wo).max())
    np.testing.assert_allclose(H, Ho, rtol=1e-10, atol=1e-10 * np.abs(Ho).max())
    np.testing.assert_allclose(np.sqrt(2.0 * lh * data.size) / np.linalg.norm(data), lo, rtol=1e-9)


@pytest.mark.parametrize("N,T,K,L", SHAPES)
def test_limits_are_kl_and_itakura_saito(N, T, K, L):
    """The restatement's loss at beta = 1 +- 1e-6 approaches kl_loss * sum(data) / (N T), at beta = 1e-6 the Itakura-Saito loss (fp64,
    strictly positive data, the restatement's functions called directly)."""
    data, W0, H0 = problem(N, T, K, L, seed=13)
    data = data + 1.0
    kl = kr.kl_loss(data, W0, H0) * data.sum() / data.size
    for beta in (1.0 - 1e-6, 1.0 + 1e-6):
        np.testing.assert_allclose(br.beta_loss(data, W0, H0, beta), kl, rtol=1e-4)
    np.testing.assert_allclose(br.beta_loss(data, W0, H0, 1e-6), ir.is_loss(data, W0, H0), rtol=1e-4)


@pytest.mark.parametrize("name", ["mu_beta_small_b050", "mu_beta_small_b150", "mu_beta_small_b025", "mu_beta_small_b300",
                                  "mu_beta_short_b050", "mu_beta_short_b150", "mu_beta_short_b200", "mu_beta_k5_b050", "mu_beta_l40_b150"])
def test_series_form_of_the_term_is_the_formula(name):
    """y^beta phi(x / y) equals (x^beta + (beta - 1) y^beta - beta x y^(beta - 1)) / (beta (beta - 1)) in fp64 to 1e-7 relative, along
    the fixture's own trajectory (both sides of |delta| = 1/8 and the x = 0 terms occur)."""
    g = br.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    data, beta = g["data"], g["beta"]
    W, H = g["W0"].copy(), g["H0"].copy()
    near = far = zero = 0
    for it in range(min(g["max_itr"], 20) + 1):
        e = br.tensor_conv(W, H) + br.EPS
        d = np.abs(data / e - 1.0)
        near, far, zero = near + int(np.sum((d < 0.125) & (data > 0))), far + int(np.sum((d >= 0.125) & (data > 0))), zero + int(np.sum(data == 0))
        a, b = br.beta_loss(data, W, H, beta), br.beta_loss(data, W, H, beta, direct=True)
        assert abs(a - b) <= 1e-7 * b, (it, a, b)
        br.update_motifs(data, W, H, beta, **{k: g["reg"][k] for k in ("l1W", "l2W")})
        br.update_feature_maps(data, W, H, beta, **{k: g["reg"][k] for k in ("l1H", "l2H")})
    assert near > 0 and far > 0 and zero > 0


def test_series_coefficients():
    """c_k = 2 (beta - 2) ... (beta - k - 1) / (k + 2)!: the binomial series of ((1 + d)^beta - 1 - beta d) / (beta (beta - 1))."""
    for beta in (0.25, 0.5, 1.5, 3.0):
        c = br.series_coefficients(beta)
        np.testing.assert_allclose(c[:4], [(beta - 2) / 3, (beta - 2) * (beta - 3) / 12, (beta - 2) * (beta - 3) * (beta - 4) / 60,
                                           (beta - 2) * (beta - 3) * (beta - 4) * (beta - 5) / 360], rtol=1e-14)
        for d in (-0.12, -0.01, 1e-4, 0.12):
            x, e = np.array([[1.0 + d]]), np.array([[1.0]])
            exact = ((1 + d) ** beta - 1 - beta * d) / (beta * (beta - 1))
            assert abs(br.terms(x, e, beta)[0, 0] - exact) <= 2e-7 * exact + 1e-30  # (cut after d^6; tiny d: the formula itself cancels)


def test_data_checks():
    ok = np.full((3, 4), 2.0)
    ok[0, 0] = 0.0  # an exact zero is legal
    assert br.check_data(ok) is not None
    for bad in (-1.0, np.nan, np.inf):
        x = ok.copy()
        x[1, 2] = bad
        with pytest.raises(ValueError, match="the beta-divergence needs"):
            br.check_data(x)
        with pytest.raises(ValueError, match="the beta-divergence needs"):
            br.fit_beta(x, np.ones((2, 3, 2)), np.ones((2, 4)), 0.5, max_itr=1)


def test_float32_model_stays_close():
    """The cdtype / edtype switches model the device: one iteration differs from fp64 at float32 level, not more."""
    data, W0, H0 = problem(48, 300, 4, 8, seed=2)
    for beta in (0.5, 1.5):
        W, H, lh = br.fit_beta(data, W0, H0, beta, max_itr=1)
        W32, H32, lh32 = br.fit_beta(data, W0, H0, beta, max_itr=1, cdtype=np.float32, edtype=np.float32)
        assert 0 < np.linalg.norm(W32 - W) / np.linalg.norm(W) < 1e-5
        assert 0 < np.linalg.norm(H32 - H) / np.linalg.norm(H) < 1e-5
        assert abs(lh32[-1] - lh[-1]) < 1e-5 * lh[-1]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_current(name):
    """The committed fixture is what the restatement computes today, and stays within the size agreed for golden files."""
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 250_000
    g = br.load_fixture(path)
    W, H, lh = br.fit_beta(g["data"], g["W0"], g["H0"], g["beta"], max_itr=g["max_itr"], **g["reg"])
    rtol = 1e-12 if g["exact"] else 1e-7  # (W32 / H32: stored rounded to float32, 6e-8 relative)
    np.testing.assert_allclose(W, g["W"], rtol=rtol, atol=0)
    np.testing.assert_allclose(H, g["H"], rtol=rtol, atol=0)
    np.testing.assert_allclose(lh, g["loss_hist"], rtol=1e-12)
    assert len(lh) == g["max_itr"] + 1 and g["data"].min() == 0 and f"b{int(round(g['beta'] * 100)):03d}" in name
    if "_reg_" in name:
        assert all(v > 0 for v in g["reg"].values())  # all four regularisers
    else:
        assert np.all(np.diff(lh) <= 0.0)


def test_fixture_counts_are_admitted():
    """Every fixture was written at a count profiles/mu_beta_precision.txt admits; the T < L shape at 20 iterations or more."""
    adm = {name: int(count) for _, name, count in profile_lines("admit")}
    for name in FIXTURES:
        assert int(np.load(os.path.join(GOLDEN, name + ".npz"))["max_itr"]) <= adm[name], name
    assert all(adm[n] >= 20 for n in FIXTURES if "_short_" in n)


def test_window_constant_agrees_everywhere(cmf):
    """One number in the profile (where tools/mu_beta_precision.py derives it), the header, host.py and the restatement."""
    (_, w), = profile_lines("window")
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert float(re.search(r"#define CMF_BETA_WINDOW (\S+)", header).group(1)) == float(w)
    assert float(re.search(r"#define CMF_BETA_MAX (\S+)", header).group(1)) == cmf.host.BETA_MAX == br.BETA_MAX == 4.0
    assert cmf.host.BETA_WINDOW == float(w) == br.WINDOW
    assert float(w) in (0.01, 0.02, 0.05, 0.1)


def test_accepted_set():
    w = br.WINDOW
    for ok in (w, 0.5, 1.0 - w, 1.0 + w, 1.5, 2.0, 3.0, 4.0):
        assert br.check_beta(ok) == ok
    for bad in (-1.0, 0.0, w / 2, 1.0 - w / 2, 1.0, 1.0 + w / 2, 4.0 + 1e-9, np.nan, np.inf):
        with pytest.raises(ValueError):
            br.check_beta(bad)


def test_host_refusals_name_their_reason(cmf):
    """Raised before anything touches a device: no GPU needed."""
    data = np.random.default_rng(0).random((6, 40)) + 0.1
    w = cmf.host.BETA_WINDOW
    for bad, what in ((-0.5, r"\(0, 4\]"), (0.0, "CMF_DIV_IS"), (1.0, "CMF_DIV_KL"), (w / 2, "lies within"), (1.0 - w / 2, "lies within"),
                      (1.0 + w / 2, "lies within"), (4.5, r"\(0, 4\]"), (float("nan"), "finite"), (None, "needs beta=")):
        with pytest.raises(ValueError, match=what):
            cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":beta", beta=bad)
    with pytest.raises(ValueError, match="divergence=':beta' only"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":kl", beta=0.5)
    for alg in (":hals", ":pgd", ":admm", cmf.ANLSUpdate, ":sep"):
        with pytest.raises(NotImplementedError, match="alg=:mult"):
            cmf.fit_cnmf(data, L=3, K=2, alg=alg, divergence=":beta", beta=0.5)
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":beta", beta=0.5, mask=np.ones((6, 40)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":beta", beta=0.5, devices=[0, 0])
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.cross_validate(data, [3], [2], divergence=":beta", beta=0.5)
    res = cmf.CNMF_results(data, np.ones((2, 6, 3)), np.ones((2, 40)), np.zeros(1), np.zeros(1))
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.evaluate_heldout(res, np.ones((6, 40)), divergence=":beta")
    with pytest.raises(ValueError, match="CMF_DIV_KL"):
        cmf.evaluate_divergence(res, kind=":beta", beta=1.0)
    assert cmf.host._divergence_kind(":beta") == 3 and cmf.host._divergence_kind("beta") == 3


def test_entry_is_declared_and_bound(cmf):
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert re.search(r"int cmf_mu_set_beta_divergence\(cmf_handle h, double beta\);", header)
    julia = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert ":cmf_mu_set_beta_divergence" in julia
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert lib.cmf_abi_version() == 6  # an additive entry
    lib.cmf_mu_set_beta_divergence.argtypes = [ctypes.c_void_p, ctypes.c_double]
    assert lib.cmf_mu_set_beta_divergence(None, 0.5) == 1  # CMF_ERR_ARG: handle is NULL (no device touched)


def test_restatement_is_test_infrastructure_only():
    """Nothing under cmf.jl_amd/, include/ or bench.py imports the restatement."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("cmf.jl_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(d, f) for f in files if f.endswith((".py", ".h", ".hip", ".jl"))]
    for p in paths:
        assert "beta_mu_restatement" not in open(p, errors="replace").read(), p
