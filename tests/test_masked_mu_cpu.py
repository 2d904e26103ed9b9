"""CPU checks of the masked MU rule: the fp64 restatement (tests/masked_mu_restatement.py) against the oracle and against its own
invariants, holdout_mask, the host-side refusals, and the two new C entries in every binding table."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import masked_mu_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_masked_small", "mu_masked_small_reg", "mu_masked_k5", "mu_masked_k33", "mu_masked_short"]


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


def rand_problem(seed, N, T, K, L):
    rng = np.random.default_rng(seed)
    return rng.random((K, N, L)), rng.random((K, T)), rng.random((N, T))


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (37, 150, 33, 7), (6, 3, 2, 5)])
@pytest.mark.parametrize("reg", [dict(), dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)])
def test_all_ones_mask_is_the_oracles_mu_rule(oracle, monkeypatch, N, T, K, L, reg):
    """3 iterations: W, H and the loss within 1e-12 relative -- and, in the form that follows the oracle's operation order
    (LITERAL_SLICES), bit for bit."""
    W0, H0, data = rand_problem(3, N, T, K, L)
    Wr, Hr, lr, _ = oracle.fit_mult(data, W0, H0, max_itr=3, check_convergence=False, **reg)
    W, H, lh = mr.fit_masked(data, np.ones((N, T)), W0, H0, max_itr=3, **reg)
    np.testing.assert_allclose(W, Wr, rtol=1e-12, atol=0)
    np.testing.assert_allclose(H, Hr, rtol=1e-12, atol=0)
    np.testing.assert_allclose(lh, lr, rtol=1e-12, atol=0)
    monkeypatch.setattr(mr, "LITERAL_SLICES", True)
    W, H, lh = mr.fit_masked(data, np.ones((N, T)), W0, H0, max_itr=3, **reg)
    np.testing.assert_array_equal(W, Wr)
    np.testing.assert_array_equal(H, Hr)
    np.testing.assert_array_equal(lh, lr)


@pytest.mark.parametrize("name", FIXTURES)
def test_heldout_nan_is_inert_and_fixture_is_current(name):
    """Overwriting the held-out entries of data with NaN leaves W, H and loss_hist bitwise unchanged; and the committed fixture
    is what the restatement computes today."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    reg = {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")}
    W, H, lh = mr.fit_masked(g["data"], g["mask"], g["W0"], g["H0"], max_itr=int(g["max_itr"]), **reg)
    np.testing.assert_allclose(W, g["W"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(H, g["H"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(lh, g["loss_hist"], rtol=1e-10)
    data_nan = np.where(g["mask"] != 0, g["data"], np.nan)
    assert np.isnan(data_nan).any()
    Wn, Hn, ln = mr.fit_masked(data_nan, g["mask"], g["W0"], g["H0"], max_itr=int(g["max_itr"]), **reg)
    np.testing.assert_array_equal(Wn, W)
    np.testing.assert_array_equal(Hn, H)
    np.testing.assert_array_equal(ln, lh)
    assert np.isfinite(ln).all()


@pytest.mark.parametrize("name", [n for n in FIXTURES if n != "mu_masked_small_reg"])
def test_loss_is_non_increasing_without_regularisers(name):
    """The masked rule is the multiplicative update of norm(M .* (data - conv(W, H)))^2: monotone for l1 = l2 = 0."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    lh = g["loss_hist"]
    assert len(lh) == int(g["max_itr"]) + 1
    assert np.all(np.diff(lh) <= 1e-13 * lh[:-1]), np.diff(lh).max()


def test_loss_is_non_increasing_on_a_longer_fit():
    W0, H0, data = rand_problem(9, 60, 400, 3, 8)
    for frac, block in ((0.2, 8), (0.5, 1)):
        _, _, lh = mr.fit_masked(data, mr.block_mask(60, 400, frac, block, 4), W0, H0, max_itr=60)
        assert np.all(np.diff(lh) <= 1e-13 * lh[:-1])


def test_rows_and_columns_without_observations_fall_to_eps():
    W0, H0, data = rand_problem(4, 12, 60, 2, 4)
    mask = np.ones((12, 60))
    mask[5, :] = 0.0   # a unit never observed
    mask[:, 20] = 0.0  # a sample never observed
    W, H, lh = mr.fit_masked(data, mask, W0, H0, max_itr=3)
    assert np.all(W[:, 5, :] == mr.EPS) and np.isfinite(W).all() and np.isfinite(H).all() and np.isfinite(lh).all()


def _zero_runs(row):
    """lengths of the maximal runs of zeros of a 0/1 vector, and whether each ends at the end of the vector"""
    z = np.concatenate(([0], (row == 0).astype(int), [0]))
    d = np.diff(z)
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return ends - starts, ends == len(row)


@pytest.mark.parametrize("N,T,frac,block", [(60, 1500, 0.2, 8), (40, 700, 0.1, 20), (30, 500, 0.5, 1), (5, 7, 0.3, 10)])
def test_holdout_mask(cmf, N, T, frac, block):
    m = cmf.holdout_mask(N, T, frac=frac, block=block, seed=7)
    assert m.shape == (N, T) and m.flags.f_contiguous and set(np.unique(m)) <= {0.0, 1.0}
    np.testing.assert_array_equal(m, cmf.holdout_mask(N, T, frac=frac, block=block, seed=7))  # deterministic in the seed
    assert not np.array_equal(m, cmf.holdout_mask(N, T, frac=frac, block=block, seed=8)) or N * T < 50
    for n in range(N if block > 1 else 0):  # every run is `block` long, except where T cuts it (block = 1 is speckle: entries may touch)
        lens, at_end = _zero_runs(m[n])
        assert np.all((lens == block) | (at_end & (lens < block))), (n, lens)
    if N * T >= 10000:
        # The held-out share: an entry is held out with probability frac, and entries of one run are perfectly correlated, so
        # the share has the spread of a binomial over the N T / block independent runs: sd = sqrt(frac (1 - frac) block / (N T)).
        # 4 sd, plus the start-up bias of a row that begins observed-or-run rather than stationary (below frac * block / T).
        sd = math.sqrt(frac * (1 - frac) * block / (N * T))
        assert abs((1.0 - m.mean()) - frac) < 4 * sd + frac * block / T, (1.0 - m.mean(), frac, sd)


def test_holdout_mask_argument_checks(cmf):
    assert cmf.holdout_mask(4, 9, frac=0.0).min() == 1.0
    with pytest.raises(ValueError):
        cmf.holdout_mask(4, 9, frac=1.0)
    with pytest.raises(ValueError):
        cmf.holdout_mask(4, 9, frac=0.1, block=0)
    with pytest.raises(ValueError, match="block / \\(block \\+ 1\\)"):
        cmf.holdout_mask(4, 9, frac=0.9, block=2)


def test_mask_is_a_known_keyword(cmf):
    from cmf_jl_amd import host

    assert "mask" in host._KNOWN_KW
    for name in ("holdout_mask", "evaluate_heldout", "cross_validate"):
        assert callable(getattr(cmf, name))
    assert callable(cmf.MultUpdate.set_mask) and callable(cmf.MultUpdate.masked_loss)


def test_host_refusals_name_their_reason(cmf):
    """Raised before anything touches a device: no GPU needed."""
    data = np.random.default_rng(0).random((6, 40))
    mask = np.ones((6, 40))
    with pytest.raises(ValueError, match=r"loss_func=MaskedLoss\("):
        cmf.fit_cnmf(data, L=3, K=2, alg=":pgd", mask=mask)
    for alg in (":hals", ":admm", cmf.ANLSUpdate, ":sep"):
        with pytest.raises(NotImplementedError, match="no masked form"):
            cmf.fit_cnmf(data, L=3, K=2, alg=alg, mask=mask)
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", mask=mask, devices=[0, 0])
    with pytest.raises(ValueError, match="0 and 1 only"):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", mask=0.5 * mask)
    with pytest.raises(ValueError):
        cmf.fit_cnmf(data, L=3, K=2, alg=":mult", mask=np.ones((6, 39)))
    with pytest.raises(TypeError):
        cmf.cross_validate(data, [3], [2], mask=mask)


def test_new_entries_are_exported_and_bound(cmf):
    for name in ("cmf_mu_set_mask", "cmf_masked_loss"):
        assert name in cmf.SYMBOLS
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert hasattr(lib, "cmf_mu_set_mask") and hasattr(lib, "cmf_masked_loss")
    assert lib.cmf_abi_version() == 6  # the entries are additive
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert re.search(r"int cmf_mu_set_mask\(cmf_handle h, const double \*mask\);", header)
    assert re.search(r"int cmf_masked_loss\(cmf_handle h, int complement, double \*resid_sumsq, double \*data_sumsq\);", header)
    assert "Only the PGD entries read the mask" not in header
    julia = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert "(:cmf_mu_set_mask, LIBCMF)" in julia and "(:cmf_masked_loss, LIBCMF)" in julia
    assert "function evaluate_heldout(" in julia and "mask=nothing" in julia
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`cmf_mu_set_mask`" in integ and "`cmf_masked_loss`" in integ
