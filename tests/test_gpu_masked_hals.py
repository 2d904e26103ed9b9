"""GPU tests of the HALS rule under a 0/1 mask by imputation (library option "hals_mask"): cmf_hals_update_motifs and
cmf_hals_update_feature_maps with a mask of cmf_mu_set_mask installed, fit_cnmf(alg=":hals", mask=), cross_validate(alg=":hals").
Every case needs the option, which the library did not know before: each fails without the feature.

Shapes (the smallest that reach each path):
  A  (70, 4130, 32, 5)   K % 32 == 0 and 65 tile rows: the masked residual conv CHASES the persistent H pipeline on a whole chip
                         (conv3_chase_kernel<6, true> and its rest launch <6, false>); N and T ragged against the 64-wide tiles.  Also
                         run under hals_persist = 0 (stage pipeline), hals_general = 3 (general sweeps) and hals_chase = 0.
  B  (37, 150, 3, 4)     few components: conv_small_kernel
  C  (20, 200, 33, 3)    two k blocks, no chase: conv_kernel
Masks (tests/masked_hals_restatement.py: masks): 30 % speckle, 20 % in blocks of L, one unit entirely held out, one column entirely
held out.

Bars: the project's (tests/test_gpu_parity.py) -- REL_FACTORS = REL_LOSS = 1e-4 against the fp64 restatement.  Admission: a
(shape, mask) case is compared only over the iterations where the float32 model of the rule (tools/hals_masked_precision.py,
profiles/hals_masked_precision.txt: planted data, init_rand start -- the problems below) stays within a third of the bar (3.3e-5).
23 of the table's 24 rows hold that through 10 iterations (at most 2.1e-5) and are compared after 1 and after 10.  ONE is shortened:
shape C under the held-out column without regularisers, whose model is at 3.1e-6 after 2 iterations and at 1.3e-4 after 5 -- it is
compared after 1 and after 2 iterations (SHORTENED)."""
import functools

import numpy as np
import pytest

import masked_hals_restatement as hr

pytestmark = pytest.mark.gpu

REL_FACTORS = 1e-4
REL_LOSS = 1e-4
FULL_ITERS = 10
SHORTENED = {((20, 200, 33, 3), "column", False): 2}  # (shape, mask, regularised): compared up to (see above)
REG = dict(l1W=0.1, l2W=0.5, l1H=0.1, l2H=0.2)
A, B, C = (70, 4130, 32, 5), (37, 150, 3, 4), (20, 200, 33, 3)
MASKS = ("speckle30", "blocks20", "unit", "column")
# (shape, options): every path the rule runs on
PATHS = [pytest.param(A, {}, id="A-chased"), pytest.param(A, {"hals_persist": 0}, id="A-stage"), pytest.param(A, {"hals_general": 3}, id="A-general"),
         pytest.param(A, {"hals_chase": 0}, id="A-unchased"), pytest.param(B, {}, id="B-few"), pytest.param(C, {}, id="C-two-k-blocks")]


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    lib = m.load_library()
    assert lib.cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(shape):
    """Planted sequences and the least-squares-scaled random start (the problems of the HALS parity tests): computed once, left unchanged."""
    from oracle import cmf_oracle as o

    N, T, K, L = shape
    data, _, _ = o.c_gen_synthetic(N=N, T=T, K=3, L=L, seed=1234)
    data = np.asfortranarray(np.maximum(data, 0.0))
    W0, H0 = o.c_init_rand(data, L=L, K=K, seed=0)
    return frozen(data, W0, H0)


@functools.lru_cache(maxsize=None)
def mask_of(shape, name):
    N, T, K, L = shape
    return frozen(hr.masks(N, T, L)[name])[0]


@functools.lru_cache(maxsize=None)
def integer_problem(shape):
    """Integer W, H, X small enough that every conv value is an integer below 2^24: exact in float32, so two handles that read the
    same residual run the same bits."""
    N, T, K, L = shape
    rng = np.random.default_rng(7)
    W = rng.integers(0, 3, (K, N, L)).astype(np.float64)
    H = (rng.integers(0, 4, (K, T)) * (rng.random((K, T)) < 0.5)).astype(np.float64)
    X = rng.integers(0, 10, (N, T)).astype(np.float64)
    return frozen(np.asfortranarray(X), np.asfortranarray(W), np.asfortranarray(H))


@functools.lru_cache(maxsize=None)
def compare_iters(shape, mname, regged):
    return (1, SHORTENED.get((shape, mname, regged), FULL_ITERS))


@functools.lru_cache(maxsize=None)
def reference(shape, mname, regged):
    """The fp64 restatement (its half-updates through the oracle's C code) after each of the case's compare_iters: {it: (W, H)}, loss_hist."""
    from oracle import cmf_oracle as o

    data, W0, H0 = problem(shape)
    reg = REG if regged else {}
    mask = mask_of(shape, mname)
    iters = compare_iters(shape, mname, regged)
    W, H, lh, snaps = np.array(W0), np.array(H0), [hr.masked_loss(o, data, mask, W0, H0)], {}
    for it in range(1, max(iters) + 1):
        hr.masked_hals_half_W(o, data, mask, W, H, l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0), use_c=True)
        lh.append(hr.masked_hals_half_H(o, data, mask, W, H, l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0), use_c=True))
        if it in iters:
            snaps[it] = (W.copy(), H.copy())
    return snaps, np.asarray(lh)


def masked_rule(cmf, data, W0, H0, mask, options=None):
    rule = cmf.HALSUpdate(data, W0, H0)
    try:
        rule.set_option("hals_mask", 1)
        for k, v in (options or {}).items():
            rule.set_option(k, v)
        if mask is not None:
            rule.set_mask(mask)
    except Exception:
        rule.close()
        raise
    return rule


def plain_rule(cmf, data, W0, H0, options=None):
    rule = cmf.HALSUpdate(data, W0, H0)
    for k, v in dict({"hals_gram": 0}, **(options or {})).items():
        rule.set_option(k, v)
    return rule


def run(rule, iters, reg=None, snaps=()):
    reg = reg or {}
    lh, out = [], {}
    for it in range(1, iters + 1):
        rule.update_motifs(l1W=reg.get("l1W", 0), l2W=reg.get("l2W", 0))
        lh.append(rule.update_feature_maps(l1H=reg.get("l1H", 0), l2H=reg.get("l2H", 0)))
        if it in snaps:
            out[it] = rule.download()
    W, H = rule.download()
    return (W, H, np.asarray(lh), out) if snaps else (W, H, np.asarray(lh))


def same_bits(a, b, what=""):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), what


# ---- 1. identity against the plain rule on integer problems, bitwise -----------------------------------------------------------------
@pytest.mark.parametrize("shape,options", PATHS)
def test_integer_problems_run_the_plain_rules_bits_on_the_imputed_data(cmf, shape, options):
    """One update_motifs, and one update_feature_maps from the integer factors, on the masked handle against a plain HALSUpdate with
    hals_gram = 0 created on X~ = where(M, X, conv(W, H)): the same residual, exactly, so the same W and the same H bit for bit.  The
    losses are two different quantities (the plain handle's residual keeps est_new - X~ at the held-out entries and is divided by
    norm(X~)); each is held to its own fp64 value from the downloaded factors at REL_LOSS."""
    from oracle import cmf_oracle as o

    X, W0, H0 = integer_problem(shape)
    est = o.tensor_conv(W0, H0)
    assert np.array_equal(est, np.rint(est)) and est.max() < 2 ** 24 and X.max() < 2 ** 24
    for mname in MASKS:
        mask = mask_of(shape, mname)
        Xt = np.asfortranarray(np.where(mask != 0, X, est))
        m, p = masked_rule(cmf, X, W0, H0, mask, options), plain_rule(cmf, Xt, W0, H0, options)
        try:
            m.update_motifs()
            p.update_motifs()
            Wm, Wp = m.download()[0], p.download()[0]
            assert np.array_equal(Wm, Wp) and not np.array_equal(Wm, W0), (mname, "W")
            for r in (m, p):
                r.upload(W0, H0)
            lm, lp = m.update_feature_maps(), p.update_feature_maps()
            Hm, Hp = m.download()[1], p.download()[1]
            assert np.array_equal(Hm, Hp) and not np.array_equal(Hm, H0), (mname, "H")
            en = o.tensor_conv(W0, Hm)
            want_m = np.linalg.norm(np.where(mask != 0, en - X, 0.0)) / np.linalg.norm(np.where(mask != 0, X, 0.0))
            want_p = np.linalg.norm(en - Xt) / np.linalg.norm(Xt)
            print(shape, options, mname, "loss masked", lm, want_m, "plain on X~", lp, want_p)
            assert abs(lm - want_m) <= REL_LOSS * want_m and abs(lp - want_p) <= REL_LOSS * want_p
            assert m.counter("hals_masked_convs") > 0 and p.counter("hals_masked_convs") == 0
            if shape == A and not options:
                assert m.counter("launches:conv3_chase_kernel") > 0 and m.counter("launches:conv3_chase_kernel:rest") > 0
            if options.get("hals_chase", -1) == 0 or shape != A or options:
                assert m.counter("launches:conv3_chase_kernel") == 0
            assert m.counter("hals_pipeline_reruns") == 0
        finally:
            m.close()
            p.close()


# ---- 2. all-ones mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,options", PATHS)
def test_all_ones_mask_is_the_plain_rule_under_hals_gram_0(cmf, shape, options):
    data, W0, H0 = problem(shape)
    N, T, K, L = shape
    m, p = masked_rule(cmf, data, W0, H0, np.ones((N, T), order="F"), options), plain_rule(cmf, data, W0, H0, options)
    try:
        a, b = run(m, 3, REG), run(p, 3, REG)
        same_bits(a[:2], b[:2])
        # The same residual sums, divided by norm(Xm) here and by norm(data) there: the first is summed from the float32 copy on the
        # device, the second from the fp64 data at upload.  Rounding an entry to float32 moves it by at most 2^-24 of itself, so the
        # two norms, and with them the losses, differ by at most 2^-24 relative (fp64 sums: nothing else enters).
        np.testing.assert_allclose(a[2], b[2], rtol=2.0 ** -24)
        assert m.counter("hals_masked_convs") > 0
    finally:
        m.close()
        p.close()


# ---- the chase against the unchased masked conv -----------------------------------------------------------------------------------------
def test_the_chased_masked_conv_is_the_unchased_one_bit_for_bit(cmf):
    """Shape A with default options chases (both chase counters and hals_masked_convs counted); again with hals_chase = 0: W and H bit for
    bit, the losses to 1e-10 (the same per-tile sums, added in another order).  The chased plan runs three pullers per row where the
    unchased one would take four (hals_plan), which associates the cross-row sums differently; hals_persist = 3 holds the unchased run
    to the same three, so that what is compared is the conv alone."""
    data, W0, H0 = problem(A)
    mask = mask_of(A, "blocks20")
    out = {}
    for name, options in (("chased", {}), ("chased again", {}), ("unchased", {"hals_chase": 0, "hals_persist": 3})):
        rule = masked_rule(cmf, data, W0, H0, mask, options)
        try:
            out[name] = run(rule, 3, REG)
            chased = name != "unchased"
            assert (rule.counter("launches:conv3_chase_kernel") == 3) == chased and (rule.counter("launches:conv3_chase_kernel:rest") == 3) == chased
            assert rule.counter("launches:hals_h_persist_kernel:P3") == 3 and rule.counter("hals_pipeline_reruns") == 0
            # per iteration: the residual of the W half is the one the H half left (the first: one mode-6 conv), mode 7 for P, and the
            # mode-6 conv behind the sweep in two launches (chasing + rest) or one
            assert rule.counter("hals_masked_convs") == 1 + 3 * (3 if chased else 2)
        finally:
            rule.close()
    same_bits(out["chased"], out["chased again"])
    same_bits(out["chased"][:2], out["unchased"][:2])
    np.testing.assert_allclose(out["chased"][2], out["unchased"][2], rtol=1e-10)


# ---- 3. against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,options", PATHS)
@pytest.mark.parametrize("regged", [False, True], ids=["noreg", "reg"])
def test_against_the_fp64_restatement(cmf, shape, options, regged):
    data, W0, H0 = problem(shape)
    for mname in MASKS:
        mask = mask_of(shape, mname)
        snaps_r, lr = reference(shape, mname, regged)
        iters = compare_iters(shape, mname, regged)
        rule = masked_rule(cmf, data, W0, H0, mask, options)
        try:
            l0 = rule.compute_loss()
            _, _, lg, snaps_g = run(rule, max(iters), REG if regged else {}, snaps=iters)
        finally:
            rule.close()
        lg = np.concatenate(([l0], lg))
        for it in iters:
            relW, relH = frob_rel(snaps_g[it][0], snaps_r[it][0]), frob_rel(snaps_g[it][1], snaps_r[it][1])
            rell = float(np.max(np.abs(lg[:it + 1] - lr[:it + 1]) / lr[:it + 1]))
            print(shape, options, mname, "reg" if regged else "", "it", it, "relW", relW, "relH", relH, "max rel loss", rell)
            assert relW < REL_FACTORS and relH < REL_FACTORS, (mname, it)
            np.testing.assert_allclose(lg[:it + 1], lr[:it + 1], rtol=REL_LOSS)
        if not regged:  # the majorisation argument on the device: fp32, so the slack is the bar's, not fp64's
            assert np.all(np.diff(lg) <= REL_LOSS * lg[:-1]), mname


# ---- 4. garbage at the held-out entries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,options", PATHS)
def test_nan_and_inf_at_held_out_entries_change_no_bit(cmf, shape, options):
    data, W0, H0 = problem(shape)
    for mname in MASKS:
        mask = mask_of(shape, mname)
        bad = hr.garbage(data, mask)
        assert np.isnan(bad).any() and np.isinf(bad).any()
        out = []
        for X in (np.where(mask != 0, data, 0.0), bad):
            rule = masked_rule(cmf, np.asfortranarray(X), W0, H0, mask, options)
            try:
                l0 = rule.compute_loss()
                out.append(run(rule, 2, REG) + (l0,))
            finally:
                rule.close()
        same_bits(out[0], out[1], mname)
        assert np.isfinite(out[1][2]).all() and np.isfinite(out[1][0]).all() and np.isfinite(out[1][1]).all()


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_the_option_can_be_switched_and_the_mask_cleared(cmf, shape):
    data, W0, H0 = problem(shape)
    mask = mask_of(shape, "speckle30")
    ref = masked_rule(cmf, data, W0, H0, mask)
    rule = masked_rule(cmf, data, W0, H0, mask)
    try:
        want = run(ref, 3, REG)
        run(rule, 2, REG)
        rule.set_option("hals_mask", 0)  # off after a masked run: the old refusal, from both entries, nothing changed
        for call in (rule.update_motifs, rule.update_feature_maps):
            with pytest.raises(cmf.CMFError, match="HALS rule has no masked form") as ei:
                call()
            assert ei.value.code == 3  # CMF_ERR_STATE
        rule.set_option("hals_mask", 1)  # on again: continues where it was
        got = run(rule, 1, REG)
        same_bits(got[:2], want[:2])
        assert got[2][0] == want[2][2]
        # clearing the mask: the plain rule (default hals_gram = 2), bit-identical to a fresh handle on the same factors
        rule.set_mask(None)
        fresh = cmf.HALSUpdate(data, got[0], got[1])
        try:
            same_bits(run(rule, 2, REG), run(fresh, 2, REG))
            before = rule.counter("hals_masked_convs")
            assert rule.counter("launches:hals_p_init_kernel:den") > 0  # (hals_gram = 2 applies again)
            assert before == ref.counter("hals_masked_convs") + 1  # (one more than the uninterrupted run: the residual the switch voided)
        finally:
            fresh.close()
        # a divergence other than the squared error stays refused, option or not
        rule.set_mask(mask)
        rule.set_option("kl_mask", 1)
        rule.set_divergence(":kl")
        with pytest.raises(cmf.CMFError, match="minimises the squared error only"):
            rule.update_motifs()
    finally:
        ref.close()
        rule.close()


def test_a_mask_of_the_pgd_rule_is_not_the_hals_rules(cmf):
    """cmf_set_mask (real-valued weights, the PGD rule's) leaves the HALS entries on the plain rule, as before."""
    data, W0, H0 = problem(B)
    N, T, K, L = B
    weights = np.asfortranarray(0.25 + 0.5 * np.random.default_rng(1).random((N, T)))
    a, b = cmf.HALSUpdate(data, W0, H0), cmf.HALSUpdate(data, W0, H0)
    try:
        a.set_option("hals_mask", 1)
        from cmf_jl_amd import _lib

        _lib.check(a._lib.cmf_set_mask(a._h, _lib.ptr(weights)))
        same_bits(run(a, 2, REG), run(b, 2, REG))
        assert a.counter("hals_masked_convs") == 0
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_calls_alone_alternated_and_speculated_give_the_same_bits(cmf, shape):
    data, W0, H0 = problem(shape)
    mask = mask_of(shape, "blocks20")
    out = {}
    for spec in (1, 0):
        rule = masked_rule(cmf, data, W0, H0, mask, {"speculate": spec})
        try:
            rule.update_feature_maps(**{k: REG[k] for k in ("l1H", "l2H")})  # alone
            rule.update_feature_maps(**{k: REG[k] for k in ("l1H", "l2H")})
            rule.update_motifs(**{k: REG[k] for k in ("l1W", "l2W")})          # alone, twice
            rule.update_motifs(**{k: REG[k] for k in ("l1W", "l2W")})
            out[spec] = run(rule, 3, REG)                                          # alternated
            hits = rule.counter("speculated_contractions")
            assert hits == (2 if spec else 0), hits  # (the W halves of the alternated iterations 2 and 3 found their contraction done)
            assert rule.counter("launches:hals_w_speculate") == (3 if spec else 0)
        finally:
            rule.close()
    same_bits(out[1], out[0])


def test_an_armed_writeback_delivers_the_factors(cmf):
    data, W0, H0 = problem(A)
    mask = mask_of(A, "unit")
    ref, rule = masked_rule(cmf, data, W0, H0, mask), masked_rule(cmf, data, W0, H0, mask)
    rule.sync_every_call = True
    rule.verify_args = "none"  # (NaN-filled caller arrays: the write-back is what is pinned here)
    W, H = np.full(W0.shape, np.nan, order="F"), np.full(H0.shape, np.nan, order="F")
    try:
        for it in range(2):
            ref.update_motifs()
            want = ref.update_feature_maps()
            rule.update_motifs(data, W, H)
            assert rule.update_feature_maps(data, W, H) == want
            Wd, Hd = rule.download()
            assert np.array_equal(W, Wd) and np.array_equal(H, Hd), it
        assert rule.counter("writeback_overlapped") == 2
    finally:
        ref.close()
        rule.close()


# ---- 6. host ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [B, C], ids=["B", "C"])
def test_fit_cnmf_is_the_call_by_call_loop(cmf, shape):
    data, W0, H0 = problem(shape)
    N, T, K, L = shape
    mask = mask_of(shape, "blocks20")
    bad = hr.garbage(data, mask)
    r = cmf.fit_cnmf(bad, L=L, K=K, alg=":hals", mask=mask, options={"hals_mask": 1}, max_itr=4, check_convergence=False,
                     W_init=np.array(W0), H_init=np.array(H0), **REG)
    rule = masked_rule(cmf, data, W0, H0, mask)
    try:
        l0 = rule.compute_loss()
        W, H, lh = run(rule, 4, REG)
    finally:
        rule.close()
    assert np.array_equal(r.W, W) and np.array_equal(r.H, H)
    np.testing.assert_array_equal(r.loss_hist, np.concatenate(([l0], lh)))
    with pytest.raises(NotImplementedError, match="no masked form"):
        cmf.fit_cnmf(data, L=L, K=K, alg=":hals", mask=mask, max_itr=1)


def test_cross_validate_with_the_hals_rule(cmf):
    data = cmf.gen_synthetic(N=30, T=400, K=3, L=4, seed=5)
    data = np.maximum(data, 0.0)
    out = cmf.cross_validate(data, L_vals=(4,), K_vals=(2, 6), frac=0.2, repeats=2, seed=3, alg=":hals", options={"hals_mask": 1},
                             max_itr=15, check_convergence=False)
    assert set(out) == {(4, 2), (4, 6)}
    for scores in out.values():
        assert scores["train"].shape == (2,) and scores["test"].shape == (2,)
        assert np.isfinite(scores["train"]).all() and np.isfinite(scores["test"]).all()
        assert np.all(scores["train"] > 0) and np.all(scores["train"] < 1.5) and np.all(scores["test"] > 0)
    # the fit that cross_validate made for the first pair, redone by hand: its masked HALS fit, scored by evaluate_heldout
    mask = cmf.holdout_mask(30, 400, frac=0.2, block=4, seed=3)
    r = cmf.fit_cnmf(data, L=4, K=2, alg=":hals", mask=mask, seed=3, options={"hals_mask": 1}, max_itr=15, check_convergence=False)
    train, test = cmf.evaluate_heldout(r, mask)
    assert (train, test) == (out[(4, 2)]["train"][0], out[(4, 2)]["test"][0])
    assert abs(train - r.loss_hist[-1]) <= REL_LOSS * train  # loss_hist of a masked HALS fit is the masked MU rule's loss
