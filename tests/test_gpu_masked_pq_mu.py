"""GPU tests of the Itakura-Saito and beta forms of the MU rule under a 0/1 mask (cmf_set_option "pq_mask" + cmf_mu_set_mask +
cmf_mu_set_divergence / cmf_mu_set_beta_divergence; fit_cnmf(divergence=, mask=, options={"pq_mask": 1}), evaluate_heldout and
cross_validate with the same option) against the fp64 restatement tests/masked_pq_mu_restatement.py and the fixtures
tests/golden/mu_masked_is_*.npz / mu_masked_beta_*_bNNN.npz, at the project's bars:

    REL_FACTORS = 1e-4   Frobenius-relative error of W and of H
    REL_LOSS    = 1e-4   per-entry relative error of loss_hist

How long a fit is compared: the `admit` lines of profiles/mu_masked_pq_precision.txt (tools/mu_masked_pq_precision.py); load()
checks that every fixture was written at a count its line admits.  Data under mask == 0 is NaN throughout unless a test says
otherwise.  Every test sets the option "pq_mask", which the library does not know without the feature.

The loss bar between two tile forms of one loss conv (`lossbar`): the form's line in profiles/mu_divergence_elementwise.txt.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import exact_problems as ep
import masked_pq_mu_restatement as pm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_masked_pq_mu as mg  # noqa: E402

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BARS = ep.read_bars(os.path.join(ROOT, "profiles", "mu_divergence_elementwise.txt"))
LOSSBAR = {0.0: BARS["lossbar"]["is"], 0.5: BARS["lossbar"]["beta050"], 1.5: BARS["lossbar"]["beta150"]}
NOREG = dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
SHAPE_IDS = lambda s: "x".join(map(str, s))  # noqa: E731
# the options the unmasked forms accept that change the conv's tile form only (the first set is the reference), and reuse_est
CONV_OPTIONS = [{}, dict(conv_kernel=2), dict(conv_kernel=3), dict(conv_split=0), dict(conv_split=4)]
SMALL_K_OPTIONS = [dict(small_k=0), dict(small_k=2)]  # (other contraction kernels too: held to the 1e-4 bar, not to the bit)
_seen = {"masked": set(), "unmasked": set()}  # launches:<path> reached, over every handle test_conv_form_options made


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def betas_of(shape):
    return pm.BETAS + (pm.BETAS_FIRST if shape == pm.SHAPES[0] else ())


@functools.lru_cache(maxsize=None)
def load(case):
    g = pm.load_fixture(os.path.join(GOLDEN, pm.fixture_name(*case[:4])))
    assert g["max_itr"] <= mg.admitted()[pm.case_name(*case[:4])], f"{case} was written at a count the precision profile does not admit"
    return g


@functools.lru_cache(maxsize=None)
def synthetic(shape, kind):
    return pm.synthetic_case(shape, kind)


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def set_form(rule, beta):
    rule.set_divergence(":itakura_saito") if beta == 0 else rule.set_divergence(":beta", beta=beta)


def new_rule(cmf, data, mask, W0, H0, beta, options=None, order="mask_first"):
    """A handle in the masked form (mask=None: the unmasked form, on clean data)."""
    rule = cmf.MultUpdate(data, W0, H0)
    try:
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        if mask is None:
            set_form(rule, beta)
            return rule
        rule.set_option("pq_mask", 1)
        if order == "mask_first":
            rule.set_mask(mask)
            set_form(rule, beta)
        else:
            set_form(rule, beta)  # (needs clean raw data: the unmasked check runs first)
            rule.set_mask(mask)
    except Exception:
        rule.close()
        raise
    return rule


def run(rule, iters, reg=None):
    lh = [rule.compute_loss()] + list(rule.iterate(iters, **(reg or {})))
    W, H = rule.download()
    return W, H, np.asarray(lh)


def gpu_fit(cmf, data, mask, W0, H0, beta, iters, reg=None, options=None, order="mask_first"):
    rule = new_rule(cmf, data, mask, W0, H0, beta, options, order)
    try:
        return run(rule, iters, reg)
    finally:
        rule.close()


def assert_same(a, b, what=""):
    for x, y, name in zip(a, b, ("W", "H", "losses")):
        assert np.isfinite(x).all(), (what, name)
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


# ---- 1. the fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mg.CASES, ids=lambda c: pm.fixture_name(*c[:4])[:-4])
def test_fixture_parity(cmf, case):
    g = load(case)
    for order in ("mask_first", "divergence_first"):
        data = g["data"] if order == "mask_first" else g["clean"]
        Wg, Hg, lg = gpu_fit(cmf, data, g["mask"], g["W0"], g["H0"], g["beta"], g["max_itr"], g["reg"], order=order)
        print(case, order, "relW", frob_rel(Wg, g["W"]), "relH", frob_rel(Hg, g["H"]), "max rel loss",
              float(np.max(np.abs(lg - g["loss_hist"]) / g["loss_hist"])))
        np.testing.assert_allclose(lg, g["loss_hist"], rtol=REL_LOSS)
        assert frob_rel(Wg, g["W"]) < REL_FACTORS and frob_rel(Hg, g["H"]) < REL_FACTORS
    if not any(g["reg"].values()) and g["shape"][1] >= g["shape"][3]:  # (unregularised, T >= L: the loss does not increase)
        assert np.all(np.diff(lg) <= 1e-6 * lg[:-1])  # (fp32 sums: a relative 1e-6, as in tests/test_gpu_kl_mu.py)


@pytest.mark.parametrize("case", mg.LIVE, ids=lambda c: pm.fixture_name(*c[:4])[:-4])
def test_parity_with_the_restatement(cmf, case):
    """Every (shape, mask kind, regularised, beta) that has no fixture -- the small shapes, where the fp64 restatement is quick --
    against the restatement itself, at a count the precision profile admits: with test_fixture_parity every shape is held to the
    1e-4 bar under all three mask kinds, with and without the four regularisers, for Itakura-Saito and beta = 0.5 and 1.5."""
    shape, kind, with_reg, beta, _ = case
    itr = mg.count_of(case, mg.admitted())
    assert itr >= 1
    data, _, mask, W0, H0 = synthetic(shape, kind)
    reg = pm.REG if with_reg else NOREG
    Wr, Hr, lr = pm.fit_masked_pq(data, mask, W0, H0, beta, max_itr=itr, **reg)
    Wg, Hg, lg = gpu_fit(cmf, data, mask, W0, H0, beta, itr, reg)
    print(case, "relW", frob_rel(Wg, Wr), "relH", frob_rel(Hg, Hr), "max rel loss", float(np.max(np.abs(lg - lr) / lr)))
    np.testing.assert_allclose(lg, lr, rtol=REL_LOSS)
    assert frob_rel(Wg, Wr) < REL_FACTORS and frob_rel(Hg, Hr) < REL_FACTORS


# ---- 2. what lies under the mask never enters; a unit and a sample never observed ------------------------------------------------
@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", pm.MASKS)
@pytest.mark.parametrize("with_reg", [False, True], ids=["noreg", "reg"])
def test_junk_under_the_mask(cmf, shape, kind, with_reg):
    data, clean, mask, W0, H0 = synthetic(shape, kind)
    reg = pm.REG if with_reg else NOREG
    for beta in betas_of(shape):
        want = gpu_fit(cmf, np.where(mask != 0, clean, 0.0), mask, W0, H0, beta, 3, reg)
        for junk in (np.nan, np.inf, -1.0):
            assert_same(gpu_fit(cmf, np.where(mask != 0, clean, junk), mask, W0, H0, beta, 3, reg), want, f"{shape} {kind} beta {beta} junk {junk}")
        if kind == "dead":  # a unit never observed: both of its sums are 0 and its motif entries fall to eps
            assert np.all(want[0][:, shape[0] // 2, :] == pm.EPS)  # (the held-out sample's H entries still see the samples after it)


# ---- 3. an all-ones mask is the unmasked form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("with_reg", [False, True], ids=["noreg", "reg"])
def test_all_ones_mask_is_the_unmasked_form(cmf, shape, with_reg):
    _, clean, mask, W0, H0 = synthetic(shape, "blocks")
    reg = pm.REG if with_reg else NOREG
    for beta in betas_of(shape):
        a = gpu_fit(cmf, clean, np.ones_like(mask), W0, H0, beta, 3, reg)
        b = gpu_fit(cmf, clean, None, W0, H0, beta, 3, reg)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        bar = LOSSBAR.get(beta, max(LOSSBAR.values()))  # (beta = 0.25, 2, 3 have no line of their own: the widest of the three)
        assert np.all(np.abs(a[2] - b[2]) <= bar * np.abs(b[2])), (shape, beta, a[2], b[2])


# ---- 4. the conv's tile forms ----------------------------------------------------------------------------------------------------
def counters(rule):
    return {p for p in ep.LAUNCH_PATHS if rule.counter("launches:" + p) > 0}


@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("beta", pm.BETAS)
def test_conv_form_options(cmf, shape, beta):
    """W and H do not depend on the tile form the conv runs in, nor on reuse_est (the loss-only and the loss + store modes sum the
    same terms); the losses agree within the form's loss bar (another tile form sums in another order)."""
    data, clean, mask, W0, H0 = synthetic(shape, "dead")
    ref = None
    for options in CONV_OPTIONS + SMALL_K_OPTIONS:
        for reuse_est in (1, 0):
            opts = dict(options, reuse_est=reuse_est)
            for which, d, m in (("masked", data, mask), ("unmasked", clean, None)):
                try:
                    rule = new_rule(cmf, d, m, W0, H0, beta, opts)
                except cmf.CMFError:
                    assert which == "unmasked" or not _accepts(cmf, clean, W0, H0, beta, opts)  # (refused for the unmasked form too)
                    continue
                try:
                    got = run(rule, 2)
                    rule.masked_loss(complement=True) if m is not None else None
                    _seen[which] |= counters(rule)
                finally:
                    rule.close()
                if which == "masked" and options in SMALL_K_OPTIONS:
                    assert frob_rel(got[0], ref[0]) < REL_FACTORS and frob_rel(got[1], ref[1]) < REL_FACTORS, opts
                    np.testing.assert_allclose(got[2], ref[2], rtol=REL_LOSS)
                elif which == "masked":
                    ref = ref or got
                    np.testing.assert_array_equal(got[0], ref[0], err_msg=str(opts))
                    np.testing.assert_array_equal(got[1], ref[1], err_msg=str(opts))
                    assert np.all(np.abs(got[2] - ref[2]) <= LOSSBAR[beta] * np.abs(ref[2])), (opts, got[2], ref[2])


def _accepts(cmf, clean, W0, H0, beta, opts):
    try:
        new_rule(cmf, clean, None, W0, H0, beta, opts).close()
        return True
    except cmf.CMFError:
        return False


def test_every_path_of_the_unmasked_forms_was_reached():
    """(after test_conv_form_options) every launches:<path> the unmasked Itakura-Saito / beta handles reached under the same
    options was reached by the masked ones."""
    assert _seen["unmasked"], "test_conv_form_options has not run"
    print("masked", sorted(_seen["masked"]), "unmasked only", sorted(_seen["unmasked"] - _seen["masked"]))
    assert _seen["unmasked"] <= _seen["masked"]


# ---- 5. cmf_masked_loss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("beta", pm.BETAS)
def test_masked_loss_sums(cmf, shape, beta):
    _, clean, mask, W0, H0 = synthetic(shape, "blocks")
    N, T = shape[:2]
    rule = new_rule(cmf, clean, mask, W0, H0, beta)
    try:
        rule.iterate(2)
        W, H = rule.download()
        before = rule.compute_loss()
        got = [rule.masked_loss(complement=c) for c in (False, True)]
        assert rule.compute_loss() == before  # (nothing stored, the rule's state untouched)
        np.testing.assert_array_equal(rule.download()[0], W)
    finally:
        rule.close()
    for c, (a, b) in zip((False, True), got):
        ra, rb = pm.heldout_sums(clean, mask, W, H, beta, complement=c)
        print(shape, beta, "complement", c, a, ra, b, rb)
        assert b == rb
        assert abs(a - ra) <= 1e-5 * abs(ra)
    assert got[0][1] + got[1][1] == N * T
    assert abs(before - got[0][0] / got[0][1]) <= LOSSBAR[beta] * before
    plain = cmf.MultUpdate(clean, W, H)
    try:
        set_form(plain, beta)
        total = plain.compute_loss() * N * T
    finally:
        plain.close()
    assert abs(got[0][0] + got[1][0] - total) <= LOSSBAR[beta] * total


# ---- 6. a walk on one handle -----------------------------------------------------------------------------------------------------
def test_a_walk_through_the_masked_forms_on_one_handle(cmf):
    """square -> mask -> Itakura-Saito under the mask -> beta = 0.5 under the mask -> mask cleared -> KL -> square on ONE handle.
    After every switch update_motifs! is called at once (an est of the previous form that the switch had not voided would be
    consumed), then update_feature_maps! and two more iterations: W, H and the losses of every segment are bitwise those of a fresh
    handle that was given the segment's starting factors and put directly into that form."""
    _, clean, mask, W0, H0 = synthetic((48, 300, 4, 8), "blocks")
    IS = ":itakura_saito"

    def segment(rule):
        rule.update_motifs()
        lh = [rule.update_feature_maps()] + list(rule.iterate(2))
        return rule.download() + (np.asarray(lh),)

    def beta_half(r):
        r.set_divergence(":beta", beta=0.5)

    walk = [("square", lambda r: None, lambda r: None),
            ("square + mask", lambda r: r.set_mask(mask), lambda r: r.set_mask(mask)),
            ("Itakura-Saito + mask", lambda r: r.set_divergence(IS), lambda r: (r.set_divergence(IS), r.set_mask(mask))),
            ("beta 0.5 + mask", beta_half, lambda r: (r.set_mask(mask), beta_half(r))),
            ("beta 0.5", lambda r: r.set_mask(None), beta_half),
            ("KL", lambda r: r.set_divergence(":kl"), lambda r: r.set_divergence(":kl")),
            ("square again", lambda r: r.set_divergence(":square"), lambda r: None)]
    rule = cmf.MultUpdate(clean, W0, H0)
    rule.set_option("pq_mask", 1)
    try:
        W, H = W0, H0
        seen = []
        for form, switch, install in walk:
            switch(rule)
            got = segment(rule)
            fresh = cmf.MultUpdate(clean, W, H)
            try:
                fresh.set_option("pq_mask", 1)
                install(fresh)
                want = segment(fresh)
            finally:
                fresh.close()
            assert_same(got, want, form)
            seen.append(got[2][-1])
            W, H = got[0].copy(), got[1].copy()
        assert len({float(v) for v in seen}) == len(seen)  # (every segment reported a loss of its own)
    finally:
        rule.close()


# ---- 7. refusals and states ------------------------------------------------------------------------------------------------------
def test_refusals_and_states(cmf):
    data, clean, mask, W0, H0 = synthetic((48, 300, 4, 8), "blocks")
    check = cmf.host.check
    rule = cmf.MultUpdate(clean, W0, H0)
    forms = (lambda r: r.set_divergence(":itakura_saito"), lambda r: r.set_divergence(":beta", beta=0.5))
    # option off (the default, or set back): the refusals of before, code 4
    for off in (False, True):
        if off:
            rule.set_option("pq_mask", 1)
            rule.set_option("pq_mask", 0)
        for form in forms:
            form(rule)
            with pytest.raises(cmf.CMFError, match="no masked form") as ei:
                rule.set_mask(mask)
            assert ei.value.code == 4
            rule.set_divergence(":square")
            rule.set_mask(mask)
            with pytest.raises(cmf.CMFError, match="no masked form") as ei:
                form(rule)
            assert ei.value.code == 4
            rule.set_mask(None)
    with pytest.raises(cmf.CMFError, match="pq_mask must be 0 or 1") as ei:
        rule.set_option("pq_mask", 2)
    assert ei.value.code == 1
    rule.set_option("pq_mask", 1)
    for form in forms:
        rule.set_mask(mask)
        form(rule)
        with pytest.raises(cmf.CMFError, match="both installed") as ei:
            rule.set_option("pq_mask", 0)
        assert ei.value.code == 3
        with pytest.raises(cmf.CMFError, match="Gram") as ei:
            rule.set_option("gram", 1)
        assert ei.value.code == 4
        loss = ctypes.c_double()
        for call in (lambda: rule._lib.cmf_hals_update_motifs(rule._h, 0.0, 0.0),
                     lambda: rule._lib.cmf_hals_update_feature_maps(rule._h, 0.0, 0.0, ctypes.byref(loss)),
                     lambda: rule._lib.cmf_pgd_update_motifs(rule._h, 0.0, 0.0, 1),
                     lambda: rule._lib.cmf_pgd_update_feature_maps(rule._h, 0.0, 0.0, 1, ctypes.byref(loss))):
            with pytest.raises(cmf.CMFError) as ei:
                check(call())
            assert ei.value.code == 3
        assert np.isfinite(rule.iterate(2)).all()  # (none of the refusals disturbed the rule)
        rule.set_divergence(":square")  # cleared in either order: the divergence first here, the mask first in the walk
        rule.set_mask(None)
    rule.close()
    # observed data the form cannot take: refused whichever of the two comes second, code 1, with the form's own text
    i, j = np.argwhere(mask != 0)[3]
    for beta, text, bads in ((0.0, "Itakura-Saito divergence needs", (0.0, -1e-3, np.nan, np.inf)), (0.5, "beta-divergence needs", (-1e-3, np.nan, np.inf))):
        for bad in bads:
            d = data.copy()
            d[i, j] = bad
            with pytest.raises(cmf.CMFError, match=text) as ei:
                new_rule(cmf, d, mask, W0, H0, beta)
            assert ei.value.code == 1
        # a mask that fails leaves the handle usable and unchanged
        d = clean.copy()
        d[i, j] = -1.0
        other = mask.copy()
        other[i, j] = 0.0
        rule = new_rule(cmf, d, other, W0, H0, beta)  # (valid under `other`, which holds the bad entry out)
        want = gpu_fit(cmf, d, other, W0, H0, beta, 4)
        lh = list(run(rule, 2)[2])
        with pytest.raises(cmf.CMFError, match=text) as ei:
            rule.set_mask(mask)  # observes the bad entry: refused, the old mask stays
        assert ei.value.code == 1
        with pytest.raises(cmf.CMFError, match=text) as ei:
            rule.set_mask(None)  # the raw data are checked before the rule goes back to them
        assert ei.value.code == 1
        lh += list(rule.iterate(2))
        assert_same(rule.download() + (np.asarray(lh),), want, f"beta {beta}: after a refused mask")
        rule.close()
    group = cmf.MultUpdate(clean, W0, H0, devices=[0, 0])
    for call in (lambda: group.set_option("pq_mask", 1), lambda: group.set_mask(mask), lambda: group.set_divergence(":itakura_saito")):
        with pytest.raises(cmf.CMFError) as ei:
            call()
        assert ei.value.code == 4
    group.close()


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("divergence,beta", [(":itakura_saito", None), (":beta", 0.5)])
def test_fit_evaluate_and_cross_validate(cmf, divergence, beta):
    b = 0.0 if beta is None else beta
    data, clean, mask, W0, H0 = synthetic((48, 300, 4, 8), "blocks")
    kw = dict(divergence=divergence, options={"pq_mask": 1}, **({} if beta is None else dict(beta=beta)))
    with pytest.raises(NotImplementedError, match="pq_mask"):
        cmf.fit_cnmf(data, L=8, K=4, alg=":mult", mask=mask, max_itr=5, **{k: v for k, v in kw.items() if k != "options"})
    r = cmf.fit_cnmf(data, L=8, K=4, alg=":mult", mask=mask, max_itr=5, W_init=W0, H_init=H0, **kw)
    Wr, Hr, lr = pm.fit_masked_pq(data, mask, W0, H0, b, max_itr=len(r.loss_hist) - 1)
    np.testing.assert_allclose(r.loss_hist, lr, rtol=REL_LOSS)
    assert frob_rel(r.W, Wr) < REL_FACTORS and frob_rel(r.H, Hr) < REL_FACTORS
    full = cmf.CNMF_results(clean, r.W, r.H, np.zeros(1), np.zeros(1))
    train, test = cmf.evaluate_heldout(full, mask, divergence=divergence, beta=beta, options={"pq_mask": 1})
    for got, comp in ((train, False), (test, True)):
        a, n = pm.heldout_sums(clean, mask, np.asarray(r.W, dtype=np.float64), np.asarray(r.H, dtype=np.float64), b, complement=comp)
        assert abs(got - a / n) <= 1e-5 * (a / n)
    scores = cmf.cross_validate(clean, [6, 8], [2, 3], frac=0.2, seed=5, max_itr=5, **kw)
    assert set(scores) == {(6, 2), (6, 3), (8, 2), (8, 3)}
    for idx, (L, K) in enumerate([(6, 2), (6, 3), (8, 2), (8, 3)]):  # (redone by hand: seed' = seed + index)
        m = cmf.holdout_mask(48, 300, frac=0.2, block=L, seed=5 + idx)
        rr = cmf.fit_cnmf(clean, L=L, K=K, alg=":mult", mask=m, seed=5 + idx, max_itr=5, **kw)
        for key, comp in (("train", False), ("test", True)):
            a, n = pm.heldout_sums(clean, m, np.asarray(rr.W, dtype=np.float64), np.asarray(rr.H, dtype=np.float64), b, complement=comp)
            assert abs(scores[(L, K)][key][0] - a / n) <= 1e-5 * (a / n), ((L, K), key)
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.cross_validate(clean, [6], [2], divergence=divergence, **({} if beta is None else dict(beta=beta)))


# ---- 9. the element-wise bar on the integer problems -----------------------------------------------------------------------------
import exact_masked_pq as xq  # noqa: E402

XBARS = xq.read_bars(os.path.join(ROOT, "profiles", "mu_masked_pq_elementwise.txt"))
# The loss bar of this section is the UNMASKED twin's `lossbar` (profiles/mu_divergence_elementwise.txt, the file the all-ones test reads too):
# the masked loss is a sub-sum of the very same float32 terms, divided by a count.  The float32 model's loss error is a nearly
# cancelling sum of roundings, so its worst over the 7 rows of this file's profile (beta150_mask: 4.4e-08, 8 x = 4e-07) understates
# its worst over the 100+ rows the twin's line was taken from (8.0e-08, 7e-07); what the device adds, the bias of v_exp_f32 /
# v_log_f32, is the same for both (`gpuloss beta150 4.82e-07` there; 4.00e-07 was observed here on 130x700x32x20).
XLOSSBAR = {form: BARS["lossbar"][xq.FORMS[form][0]] for form in xq.FORMS}
CONV_ONLY = {"conv_kernel", "conv_split"}
_xworst = {form: [0.0, 0.0] for form in xq.FORMS}


@functools.lru_cache(maxsize=None)
def xreference(form, shape, family):
    """The fp64 half of the form on the shape's integer problem, with the sensitivity condition asserted from these very arrays."""
    W, H, X, mask, data = xq.make_problem(shape, family, form)
    a = xq.masked_half(form, family, X, mask, W, H)
    sens = xq.sensitivity(form, a, exact=False)
    if sens < 4 * XBARS["bar"][form]:  # (the closed-form bound is a lower bound: the exact value only where it does not decide)
        sens = xq.sensitivity(form, a)
    assert sens >= 4 * XBARS["bar"][form], f"{form} {shape} {family}: one term moves an element by {sens:.2e} only (bar {XBARS['bar'][form]:g})"
    return W, H, data, mask, a["new"], a.get("loss")


@pytest.mark.parametrize("form", list(xq.FORMS))
@pytest.mark.parametrize("N,T,K,L,configs,why", xq.SHAPES, ids=[SHAPE_IDS(s[:4]) for s in xq.SHAPES])
def test_elementwise_on_the_integer_problems(cmf, N, T, K, L, configs, why, form):
    """One update_motifs! and one update_feature_maps! per configuration of the row, each element of the updated factor within the
    form's bar of the fp64 half (8 x the float32 model's worst element: profiles/mu_masked_pq_elementwise.txt), the loss within the
    unmasked twin's lossbar (XLOSSBAR above); bit-identical across the configurations that change the conv's tile form only."""
    shape, beta = (N, T, K, L), xq.FORMS[form][1]
    Ww, Hw, dw, mask, W_ref, _ = xreference(form, shape, "W")
    Wh, Hh, dh, _, H_ref, loss_ref = xreference(form, shape, "H")
    base = None
    for cfg in ep.divergence_configs(configs, form):
        rule = new_rule(cmf, dw, mask, Ww, Hw, beta, cfg)
        try:
            rule.update_motifs(l1W=ep.L1, l2W=ep.L2)
            Wg, _ = rule.download()
        finally:
            rule.close()
        rule = new_rule(cmf, dh, mask, Wh, Hh, beta, cfg)
        try:
            loss = rule.update_feature_maps(l1H=ep.L1, l2H=ep.L2)
            _, Hg = rule.download()
            reached = sorted(counters(rule))
        finally:
            rule.close()
        for got, ref, names in ((Wg, W_ref, "knl"), (Hg, H_ref, "kt")):
            assert np.isfinite(got).all() and got.min() >= pm.EPS, (form, cfg)
            _xworst[form][0] = max(_xworst[form][0], float(ep.rel_err(got, ref).max()))
            msg = ep.check_elementwise(got, ref, XBARS["bar"][form], names)
            assert msg is None, f"{form} {shape} {cfg}: {msg}; launches {reached}"
        err = abs(loss - loss_ref) / loss_ref
        _xworst[form][1] = max(_xworst[form][1], err)
        assert err <= XLOSSBAR[form], f"{form} {shape} {cfg}: loss {loss!r}, want {loss_ref!r} (rel {err:.2e}); launches {reached}"
        if base is None:
            base = (cfg, Wg, Hg)
        elif set(cfg) <= CONV_ONLY and set(base[0]) <= CONV_ONLY:
            np.testing.assert_array_equal(Wg, base[1], err_msg=f"{form} {shape}: W under {cfg} and under {base[0]}")
            np.testing.assert_array_equal(Hg, base[2], err_msg=f"{form} {shape}: H under {cfg} and under {base[0]}")
    print(f"gpu {form} {_xworst[form][0]:.3g}\ngpuloss {form} {_xworst[form][1]:.3g}")
