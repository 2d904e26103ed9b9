"""CPU checks of the KL form of the MU rule under a 0/1 mask: the fp64 restatement (tests/masked_kl_mu_restatement.py) against the
committed fixtures, against the unmasked KL restatement under an all-ones mask, and against its own invariants (a non-increasing
loss, held-out entries that never enter, observed data that must be valid); the iteration counts of the fixtures against
profiles/mu_masked_kl_precision.txt; the opt-in option "kl_mask" in the header and in the library's tables; the host refusal."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import kl_mu_restatement as kr
import masked_kl_mu_restatement as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_masked_kl_small", "mu_masked_kl_small_reg", "mu_masked_kl_k5", "mu_masked_kl_k33", "mu_masked_kl_k32",
            "mu_masked_kl_short", "mu_masked_kl_l40"]
# unregularised with T >= L: where the multiplicative update is monotone beyond round-off
MONOTONE = [n for n in FIXTURES if n not in ("mu_masked_kl_small_reg", "mu_masked_kl_short")]
SMALL_SHAPES = [s for s in mk.SHAPES if s[0] * s[1] <= 20000]


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


@functools.lru_cache(maxsize=None)
def load(name):
    return mk.load_fixture(os.path.join(GOLDEN, name + ".npz"))


def admitted():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "mu_masked_kl_precision.txt")):
        if line.startswith("admit "):
            _, name, count = line.split()
            out[name] = int(count)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_current(name):
    """The committed fixture is what the restatement computes today (on data with NaN under the mask), within the size agreed
    for golden files, and holds no inputs of its own."""
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 250_000
    assert not {"data", "W0", "H0"} & set(np.load(path).files)
    g = load(name)
    assert np.isnan(g["data"][g["mask"] == 0]).all() and (g["mask"] == 0).any()
    W, H, lh = mk.fit_masked_kl(g["data"], g["mask"], g["W0"], g["H0"], max_itr=g["max_itr"], **g["reg"])
    rtol = 1e-10 if g["exact"] else 1e-7  # (W32 / H32: stored rounded to float32, 6e-8 relative)
    np.testing.assert_allclose(W, g["W"], rtol=rtol, atol=1e-14)
    np.testing.assert_allclose(H, g["H"], rtol=rtol, atol=1e-14)
    np.testing.assert_allclose(lh, g["loss_hist"], rtol=1e-10)
    assert len(lh) == g["max_itr"] + 1
    if name == "mu_masked_kl_small_reg":
        assert all(v > 0 for v in g["reg"].values())  # all four regularisers
    if name == "mu_masked_kl_k33":  # one unit and one sample never observed: their factor entries fall to eps
        N, T = g["mask"].shape
        assert not g["mask"][N // 2].any() and not g["mask"][:, T // 3].any()
        assert np.all(W[:, N // 2, :] == mk.EPS)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_count_is_admitted(name):
    adm = admitted()
    assert name in adm and load(name)["max_itr"] <= adm[name], f"{name} was written at a count profiles/mu_masked_kl_precision.txt does not admit"


def test_every_synthetic_case_has_an_admit_line():
    adm = admitted()
    for shape in mk.SHAPES:
        for kind in mk.MASKS:
            for reg in ({}, mk.REG):
                assert adm.get(mk.case_name(shape, kind, reg), 0) >= 1, mk.case_name(shape, kind, reg)


@pytest.mark.parametrize("name", ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_short", "mu_kl_l40"])
def test_all_ones_mask_is_the_unmasked_kl_rule(name):
    g = kr.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    ones = np.ones(g["data"].shape)
    itr = min(g["max_itr"], 20)
    a = mk.fit_masked_kl(g["data"], ones, g["W0"], g["H0"], max_itr=itr, **g["reg"])
    b = kr.fit_kl(g["data"], g["W0"], g["H0"], max_itr=itr, **g["reg"])
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N,T,K,L", mk.SHAPES)
def test_denominators_under_an_all_ones_mask_are_the_ones_denominators(N, T, K, L):
    rng = np.random.default_rng(6)
    W, H = rng.random((K, N, L)), rng.random((K, T))
    ones = np.ones((N, T))
    dW, dH = kr.ones_denominators(W, H, N)
    np.testing.assert_array_equal(kr.hxt(H, ones, L), dW)
    np.testing.assert_array_equal(kr.tensor_transconv(W, ones), dH)
    np.testing.assert_allclose(dW, kr.denom_W(H, N, L), rtol=1e-12)
    np.testing.assert_allclose(dH, kr.denom_H(W, T), rtol=1e-12)


@pytest.mark.parametrize("name", MONOTONE)
def test_loss_is_non_increasing(name):
    lh = load(name)["loss_hist"]
    assert np.all(np.diff(lh) <= 0.0), np.diff(lh).max()


@pytest.mark.parametrize("N,T,K,L", [s for s in SMALL_SHAPES if s[1] >= s[3]])
@pytest.mark.parametrize("kind", mk.MASKS)
def test_loss_is_non_increasing_on_the_synthetic_cases(N, T, K, L, kind):
    data, _, mask, W0, H0 = mk.synthetic_case((N, T, K, L), kind)
    W, H, lh = mk.fit_masked_kl(data, mask, W0, H0, max_itr=20)
    assert np.isfinite(lh).all() and np.isfinite(W).all() and np.isfinite(H).all()
    assert np.all(np.diff(lh) <= 0.0), np.diff(lh).max()
    if kind == "dead":  # a unit with nothing observed: numerator and denominator are 0, its motif entries fall to eps
        assert np.all(W[:, N // 2, :] == mk.EPS)


@pytest.mark.parametrize("N,T,K,L", SMALL_SHAPES)
@pytest.mark.parametrize("kind", mk.MASKS)
def test_held_out_garbage_never_enters(N, T, K, L, kind):
    """NaN, Inf and -1 under mask == 0 leave W, H and the loss bit-identical to the run with zeros there."""
    _, clean, mask, W0, H0 = mk.synthetic_case((N, T, K, L), kind)
    ref = mk.fit_masked_kl(np.where(mask != 0, clean, 0.0), mask, W0, H0, max_itr=5, **mk.REG)
    for junk in (np.nan, np.inf, -1.0):
        got = mk.fit_masked_kl(np.where(mask != 0, clean, junk), mask, W0, H0, max_itr=5, **mk.REG)
        for x, y in zip(got, ref):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("bad", [-1e-3, np.nan, np.inf])
def test_observed_bad_data_is_refused(bad):
    _, clean, mask, W0, H0 = mk.synthetic_case((48, 300, 4, 8), "blocks")
    i, j = np.argwhere(mask != 0)[5]
    data = clean.copy()
    data[i, j] = bad
    with pytest.raises(ValueError, match="KL divergence needs"):
        mk.fit_masked_kl(data, mask, W0, H0, max_itr=1)
    with pytest.raises(ValueError, match="positive sum"):
        mk.fit_masked_kl(np.where(mask != 0, 0.0, 1.0), mask, W0, H0, max_itr=1)


def test_heldout_sums_split_the_divergence():
    _, clean, mask, W0, H0 = mk.synthetic_case((48, 300, 4, 8), "speckle")
    (d1, s1), (d0, s0) = mk.heldout_sums(clean, mask, W0, H0), mk.heldout_sums(clean, mask, W0, H0, complement=True)
    assert abs((d1 + d0) - kr.divergence(clean, kr.tensor_conv(W0, H0) + kr.EPS)) <= 1e-12 * abs(d1 + d0)
    assert abs((s1 + s0) - clean.sum()) <= 1e-12 * clean.sum()
    rule = mk.MaskedKL(np.where(mask != 0, clean, np.nan), mask)
    assert mk.masked_kl_loss(rule, W0, H0) == d1 / s1


def test_option_is_documented_but_not_listed(cmf):
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert '"kl_mask"' in header and header.index('"kl_mask"') < header.index('"nnls_large"')
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert lib.cmf_abi_version() == 6  # no new entry
    buf = ctypes.create_string_buffer(4096)
    assert lib.cmf_option_names(buf, 4096) == 0
    assert "kl_mask" not in buf.value.decode().split(",")
    lib.cmf_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    assert lib.cmf_set_option(None, b"kl_mask", 1) == 1  # CMF_ERR_ARG: a NULL handle, not an unknown name's crash
    src = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_options.h")).read()
    assert re.search(r'OPT_FLAG\(kl_mask, "[^\n"]*", FX_MU_GATE\)', src)  # (a gate among the 0/1 rows of cmf_set_option's table)
    julia = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert "divergence::Symbol=:square" in julia and '"kl_mask"' in julia
    assert "kl_mask" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_host_keywords_and_refusal(cmf):
    """Without the option the refusal is the one from before, and now names the option; raised before anything touches a device."""
    from cmf_jl_amd import host

    assert {"mask", "divergence", "options"} <= host._KNOWN_KW
    data = np.random.default_rng(0).random((6, 40))
    for options in (None, {}, {"kl_mask": 0}):
        with pytest.raises(NotImplementedError, match="mask=") as ei:
            cmf.fit_cnmf(data, L=3, K=2, alg=":mult", divergence=":kl", mask=np.ones((6, 40)), options=options)
        assert "kl_mask" in str(ei.value) and "no masked form yet" in str(ei.value)
    import inspect

    assert inspect.signature(cmf.evaluate_heldout).parameters["divergence"].default == ":square"
    with pytest.raises(ValueError, match="':square' or ':kl'"):
        host._divergence_kind(":is")
    with pytest.raises(TypeError, match="draws its own masks"):
        cmf.cross_validate(data, [3], [2], divergence=":kl", mask=np.ones((6, 40)))


def test_restatement_is_a_test_helper_only():
    """Nothing the package, the header or the benchmark reads imports the restatement."""
    hits = []
    for base in (os.path.join(ROOT, "cmf.jl_amd"), os.path.join(ROOT, "include")):
        for dirpath, _, files in os.walk(base):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".jl")):
                    if "masked_kl_mu_restatement" in open(os.path.join(dirpath, f), errors="replace").read():
                        hits.append(os.path.join(dirpath, f))
    if "masked_kl_mu_restatement" in open(os.path.join(ROOT, "bench.py")).read():
        hits.append("bench.py")
    assert not hits, hits
