"""CPU checks of the Itakura-Saito and beta forms of the MU rule under a 0/1 mask: the fp64 restatement
(tests/masked_pq_mu_restatement.py) against the committed fixtures, against the unmasked restatements under an all-ones mask, and
against its own invariants (a non-increasing loss, held-out entries that never enter, observed data that must be valid, held-out
sums that add up); the iteration counts of the fixtures against profiles/mu_masked_pq_precision.txt; the opt-in option "pq_mask"
in the header and in the library's tables; the host refusal."""
import ctypes
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

import beta_mu_restatement as br
import is_mu_restatement as ir
import masked_pq_mu_restatement as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden_masked_pq_mu as mg  # noqa: E402

SMALL_SHAPES = [s for s in pm.SHAPES if s[0] * s[1] <= 20000]
NOREG = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
CASE_IDS = lambda c: pm.fixture_name(*c[:4])[:-4]  # noqa: E731
QUICK_CASES = [c for c in mg.CASES if c[0][0] * c[0][1] <= 20000]  # (the two large shapes cost seconds per fp64 iteration)


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


@functools.lru_cache(maxsize=None)
def load(case):
    return pm.load_fixture(os.path.join(GOLDEN, pm.fixture_name(*case[:4])))


def test_fixture_files_are_the_cases_and_hold_no_inputs():
    want = {pm.fixture_name(*c[:4]) for c in mg.CASES}
    have = {f for f in os.listdir(GOLDEN) if re.match(r"mu_masked_(is|beta)_.*\.npz$", f)}
    assert have == want
    for f in have:
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 250_000
        assert not {"data", "W0", "H0", "mask", "mask_bits"} & set(np.load(os.path.join(GOLDEN, f)).files)
        assert re.match(r"mu_masked_is_[0-9x]+_[a-z]+(_reg)?\.npz$|mu_masked_beta_[0-9x]+_[a-z]+(_reg)?_b\d{3}\.npz$", f)


@pytest.mark.parametrize("case", QUICK_CASES, ids=CASE_IDS)
def test_fixture_is_current(case):
    """The committed fixture is what the restatement computes today, on data with NaN under the mask."""
    g = load(case)
    assert np.isnan(g["data"][g["mask"] == 0]).all() and (g["mask"] == 0).any()
    W, H, lh = pm.fit_masked_pq(g["data"], g["mask"], g["W0"], g["H0"], g["beta"], max_itr=g["max_itr"], **g["reg"])
    np.testing.assert_allclose(W, g["W"], rtol=1e-7, atol=1e-14)  # (W32 / H32: stored rounded to float32, 6e-8 relative)
    np.testing.assert_allclose(H, g["H"], rtol=1e-7, atol=1e-14)
    np.testing.assert_allclose(lh, g["loss_hist"], rtol=1e-12)


@pytest.mark.parametrize("case", [c for c in mg.CASES if c not in QUICK_CASES], ids=CASE_IDS)
def test_large_fixture_is_current_in_its_first_iterations(case):
    """(the two large shapes: one iteration of the restatement against the stored loss_hist, which determines the trajectory)"""
    g = load(case)
    _, _, lh = pm.fit_masked_pq(g["data"], g["mask"], g["W0"], g["H0"], g["beta"], max_itr=1, **g["reg"])
    np.testing.assert_allclose(lh, g["loss_hist"][:2], rtol=1e-12)


def test_fixtures_sit_at_admitted_counts():
    adm = mg.admitted()
    assert set(adm) == {pm.case_name(*c[:4]) for c in mg.CASES + mg.LIVE}
    # every shape under every mask kind, with and without the regularisers, for every beta of pm.BETAS is a fixture or a live case
    assert {c[:4] for c in mg.CASES + mg.LIVE} >= {(s, k, r, b) for s in pm.SHAPES for k in pm.MASKS for r in (False, True) for b in pm.BETAS}
    assert all(mg.count_of(c, adm) >= 1 for c in mg.LIVE)
    for case in mg.CASES:
        assert 1 <= load(case)["max_itr"] == mg.count_of(case, adm) <= adm[pm.case_name(*case[:4])], case
    # the profile's own rule: admitted while the distance stays at most a third of the bar
    for line in open(mg.PROFILE):
        if line.startswith("synthetic("):
            f = [x.strip() for x in line.split("|")]
            ok = 0
            for count, d in zip((1, 2, 5, 10, 20), f[1:6]):
                if d == "-" or float(d) > 1e-4 / 3:
                    break
                ok = count
            assert adm[f[0]] == ok, line


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_reg", [False, True], ids=["noreg", "reg"])
def test_all_ones_mask_is_the_unmasked_restatement(shape, with_reg):
    _, clean, mask, W0, H0 = pm.synthetic_case(shape, "blocks")
    reg = pm.REG if with_reg else NOREG
    for beta in pm.BETAS + pm.BETAS_FIRST:
        a = pm.fit_masked_pq(clean, np.ones_like(mask), W0, H0, beta, max_itr=5, **reg)
        b = ir.fit_is(clean, W0, H0, max_itr=5, **reg) if beta == 0 else br.fit_beta(clean, W0, H0, beta, max_itr=5, **reg)
        for x, y in zip(a, b):
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", pm.MASKS)
def test_what_lies_under_the_mask_never_enters(shape, kind):
    _, clean, mask, W0, H0 = pm.synthetic_case(shape, kind)
    for beta in pm.BETAS:
        want = pm.fit_masked_pq(np.where(mask != 0, clean, 0.0), mask, W0, H0, beta, max_itr=4, **pm.REG)
        for junk in (np.nan, np.inf, -1.0):
            got = pm.fit_masked_pq(np.where(mask != 0, clean, junk), mask, W0, H0, beta, max_itr=4, **pm.REG)
            for x, y in zip(got, want):
                assert np.isfinite(x).all()
                np.testing.assert_array_equal(x, y)
        if kind == "dead":  # a unit never observed: both of its sums are 0 and its motif entries fall to eps
            assert np.all(want[0][:, shape[0] // 2, :] == pm.EPS)  # (the held-out sample's H entries still see the samples after it)


def test_bad_observed_data_is_refused_with_the_forms_own_message():
    data, clean, mask, W0, H0 = pm.synthetic_case((48, 300, 4, 8), "blocks")
    i, j = np.argwhere(mask != 0)[3]
    for beta, message, bads in ((0.0, ir.MESSAGE, (0.0, -1.0, np.nan, np.inf)), (0.5, br.MESSAGE, (-1.0, np.nan, np.inf))):
        for bad in bads:
            d = data.copy()
            d[i, j] = bad
            with pytest.raises(ValueError, match=re.escape(message)):
                pm.fit_masked_pq(d, mask, W0, H0, beta, max_itr=1)
    d = data.copy()
    d[i, j] = 0.0  # (an exact zero is legal for beta > 0)
    assert np.isfinite(pm.fit_masked_pq(d, mask, W0, H0, 0.5, max_itr=1)[2]).all()
    with pytest.raises(ValueError, match="0 and 1 only"):
        pm.fit_masked_pq(data, 0.5 * mask, W0, H0, 0.0, max_itr=1)
    with pytest.raises(ValueError, match="observes nothing"):
        pm.fit_masked_pq(data, 0.0 * mask, W0, H0, 0.0, max_itr=1)


@pytest.mark.parametrize("shape", [s for s in SMALL_SHAPES if s[1] >= s[3]], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.5, 2.0, 3.0])
def test_loss_is_non_increasing(shape, beta):
    """Unregularised, T >= L: the majorisation-minimisation step does not raise the masked divergence."""
    for kind in pm.MASKS:
        data, _, mask, W0, H0 = pm.synthetic_case(shape, kind)
        lh = pm.fit_masked_pq(data, mask, W0, H0, beta, max_itr=30)[2]
        assert np.all(np.diff(lh) <= 1e-12 * lh[:-1]), (kind, lh)


@pytest.mark.parametrize("beta", pm.BETAS + pm.BETAS_FIRST)
def test_heldout_sums_split_the_divergence(beta):
    data, clean, mask, W0, H0 = pm.synthetic_case((48, 300, 4, 8), "speckle")
    (d1, n1), (d0, n0) = pm.heldout_sums(clean, mask, W0, H0, beta), pm.heldout_sums(clean, mask, W0, H0, beta, complement=True)
    total = (ir.is_loss(clean, W0, H0) if beta == 0 else br.beta_loss(clean, W0, H0, beta)) * clean.size
    assert n1 + n0 == clean.size and n1 == int(mask.sum())
    assert abs((d1 + d0) - total) <= 1e-12 * abs(total)
    xs, count = pm.check_data(data, mask, beta)
    assert count == n1 and pm.masked_loss(xs, mask, count, W0, H0, beta) == d1 / n1


def test_option_is_documented_but_not_listed(cmf):
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert '"pq_mask"' in header and header.index('"kl_mask"') < header.index('"pq_mask"') < header.index("#define CMF_DIV_IS")
    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert lib.cmf_abi_version() == 6  # no new entry
    buf = ctypes.create_string_buffer(4096)
    assert lib.cmf_option_names(buf, 4096) == 0
    assert "pq_mask" not in buf.value.decode().split(",")
    lib.cmf_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    assert lib.cmf_set_option(None, b"pq_mask", 1) == 1  # CMF_ERR_ARG: a NULL handle
    src = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_options.h")).read()
    assert re.search(r'OPT_FLAG\(pq_mask, "[^\n"]*", FX_MU_GATE\)', src)  # (a gate among the 0/1 rows of cmf_set_option's table)
    assert '"pq_mask"' in open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert "pq_mask" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    modes = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_conv_modes.h")).read()
    assert "CONV_FAM_IS_MASKED = 28" in modes and "CONV_FAM_BETA_MASKED = 32" in modes


def test_host_keywords_and_refusal(cmf):
    """Without the option the refusal is the one from before and names the option; raised before anything touches a device."""
    data = np.random.default_rng(0).random((6, 40)) + 0.1
    ones = np.ones((6, 40))
    for kw in (dict(divergence=":itakura_saito"), dict(divergence=":beta", beta=0.5)):
        for options in (None, {}, {"pq_mask": 0}):
            with pytest.raises(NotImplementedError, match="no masked form") as ei:
                cmf.fit_cnmf(data, L=3, K=2, alg=":mult", mask=ones, options=options, **kw)
            assert "pq_mask" in str(ei.value)
        with pytest.raises(NotImplementedError, match="no masked form") as ei:
            cmf.cross_validate(data, [3], [2], **kw)
        assert "pq_mask" in str(ei.value)
        res = cmf.CNMF_results(data, np.ones((2, 6, 3)), np.ones((2, 40)), np.zeros(1), np.zeros(1))
        with pytest.raises(NotImplementedError, match="no masked form") as ei:
            cmf.evaluate_heldout(res, ones, **kw)
        assert "pq_mask" in str(ei.value)
    sig = inspect.signature(cmf.evaluate_heldout).parameters
    assert sig["beta"].default is None and sig["options"].default is None and sig["divergence"].default == ":square"


def test_restatement_is_a_test_helper_only():
    hits = []
    for base in (os.path.join(ROOT, "cmf.jl_amd"), os.path.join(ROOT, "include")):
        for dirpath, _, files in os.walk(base):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".jl")) and "masked_pq_mu_restatement" in open(os.path.join(dirpath, f), errors="replace").read():
                    hits.append(os.path.join(dirpath, f))
    assert not hits and "masked_pq_mu_restatement" not in open(os.path.join(ROOT, "bench.py")).read(), hits


def test_elementwise_profile_is_current_and_meets_its_condition():
    """profiles/mu_masked_pq_elementwise.txt names the forms of tests/exact_masked_pq.py, has a row per (form, shape, family), none below
    four bars, and its bars are 8 x the float32 model's error at least on a row recomputed here; the unmasked forms' file is not this
    tool's to write."""
    import exact_masked_pq as xq
    import exact_problems as ep

    path = os.path.join(ROOT, "profiles", "mu_masked_pq_elementwise.txt")
    bars = xq.read_bars(path)
    assert set(bars["bar"]) == set(xq.FORMS) and not bars["lossbar"]  # (the loss is held to the unmasked twin's lossbar: the header says so)
    twin = xq.read_bars(os.path.join(ROOT, "profiles", "mu_divergence_elementwise.txt"))["lossbar"]
    for form in xq.FORMS:  # ... which covers what an MI355X run observed, and 8 x this file's own model rows
        assert bars["gpuloss"][form] <= twin[xq.FORMS[form][0]] and bars["gpu"][form] <= bars["bar"][form]
    rows = [ln for ln in open(path) if ln.startswith("row ")]
    assert len(rows) == 2 * len(xq.FORMS) * len(xq.SHAPES) and not any("BELOW" in r for r in rows)
    for form in xq.FORMS:
        for family in ("W", "H"):
            W, H, X, mask, data = xq.make_problem((48, 300, 4, 8), family, form)
            assert np.isnan(data[mask == 0]).all()
            a = xq.masked_half(form, family, X, mask, W, H)
            m = xq.masked_half(form, family, X, mask, W, H, cdtype=np.float32, edtype=np.float32)
            assert 8 * float(ep.rel_err(m["new"], a["new"]).max()) <= bars["bar"][form]
            assert xq.sensitivity(form, a) >= 4 * bars["bar"][form]
            # the half is the restatement's own update (to the last bits: the two write the step in another order)
            xs, count = pm.check_data(data, mask, xq.FORMS[form][1])
            W2, H2 = W.copy(), H.copy()
            if family == "W":
                pm.update_motifs(xs, mask, W2, H2, xq.FORMS[form][1], l1W=ep.L1, l2W=ep.L2)
                np.testing.assert_allclose(W2, a["new"], rtol=1e-12, atol=0)
            else:
                loss = pm.update_feature_maps(xs, mask, count, W2, H2, xq.FORMS[form][1], l1H=ep.L1, l2H=ep.L2)
                np.testing.assert_allclose(H2, a["new"], rtol=1e-12, atol=0)
                assert abs(loss - a["loss"]) <= 1e-12 * a["loss"]
    tool = open(os.path.join(ROOT, "tools", "mu_masked_pq_elementwise.py")).read()
    assert 'OUT = os.path.join(ROOT, "profiles", "mu_masked_pq_elementwise.txt")' in tool and tool.count('open(OUT, "w")') == 1 and tool.count('"w")') == 1
