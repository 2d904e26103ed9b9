"""The MU rule under a 0/1 mask (conv family CONV_FAM_MU_MASKED, modes 8-11) against its fp64 restatement BIT FOR BIT on every kernel
path: the shape table of tests/test_exact_parity.py (exact_problems.SHAPES) under every configuration the masked rule accepts, with
what that file does to the plain rule done under rule.set_mask(mask).

With a 0/1 mask, mask .* est, mask .* X, both numerators, both denominators and the loss tile sums are sums of small non-negative
integers, so the argument of tests/test_exact_parity.py holds unchanged: the contractions are exact in fp32 in any order, the updated
factor is the fp64 update up to cmf_mu's one division and one multiply (2 ulp), and every configuration gives the same bits.  A mask
tile read one strip off, or not read in the cut pieces of one tile form, stays far below the Frobenius-relative 1e-4 of
tests/test_gpu_masked_mu.py at these sizes and fails here (tests/test_exact_problems.py shows both).

masked_loss() and masked_loss(complement=True) -- the held-out score behind evaluate_heldout, the p.loss_abs branch of modes 10 / 11 --
return the restatement's sums exactly.  Reference: tests/masked_mu_restatement.py (MaskedMult, update_motifs, update_feature_maps,
masked_loss, heldout_sums)."""
import time

import numpy as np
import pytest

import exact_problems as ep
import masked_mu_restatement as mr
from exact_problems import EXACT, L1, L2, LAUNCH_PATHS, SHAPES, conv3_form, make_problem
from test_exact_parity import ULP_BAR, check_factor, check_same, counters, make_rule, reached

pytestmark = pytest.mark.gpu

EPS = ep.EPS
REG = dict(l1W=L1, l2W=L2, l1H=L1, l2H=L2)
_seen = {}
_worst = {"W": 0.0, "H": 0.0}
_done = set()


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def record(c):
    for p, v in c.items():
        _seen[p] = _seen.get(p, 0) + v


def masked_rule(cmf, cfg, X, W, H, mask):
    rule = make_rule(cmf, cfg, X, W, H)
    try:
        rule.set_mask(mask)
    except Exception:
        rule.close()
        raise
    return rule


def reference(family, W, H, X, mask, shape, holes=False, closed_form=False):
    """(updated factor, loss before, loss after the H update or None, (resid, data) sums over the observed and over the held-out
    entries, whether the loss tile sums are exact) by the restatement, with the preconditions asserted from the masked sums
    (closed_form, config 2: from exact_problems.preconditions instead -- a masked sum of non-negative terms is at most the unmasked
    one -- and without the held-out sums)."""
    if closed_form:
        b = ep.preconditions(*shape, family)
        assert b["exact"] and b["sensitive"], (shape, family, b)
    else:
        a = ep.masked_mu_half(family, W, H, X, mask)
        ep.assert_masked_mu_preconditions(a, f"{shape} {family}", holes=holes)
    rule = mr.MaskedMult(X, mask)
    Wr, Hr = W.copy(order="K"), H.copy(order="K")
    loss0 = mr.masked_loss(rule, Wr, Hr)
    sums = [] if closed_form else [mr.heldout_sums(X, mask, Wr, Hr, complement=c) for c in (False, True)]
    est = ep._conv(W, H)
    exact = max(ep.max_tile_sum((est - X) ** 2), ep.max_tile_sum(X ** 2)) <= EXACT
    if family == "W":
        mr.update_motifs(rule, Wr, Hr, l1W=L1, l2W=L2)
        new, loss1 = Wr, None
    else:
        loss1 = mr.update_feature_maps(rule, Wr, Hr, l1H=L1, l2H=L2)
        new = Hr
    assert closed_form or np.array_equal(new, a["new"])
    return new, loss0, loss1, sums, exact


def run_w_half(rule, W, H):
    """(loss, (observed sums, held-out sums), W after update_motifs!, W after iterate(1), iterate(2) vs the call-by-call loop)."""
    lw = rule.compute_loss()
    sums = [rule.masked_loss(complement=c) for c in (False, True)]
    rule.update_motifs(l1W=L1, l2W=L2)
    Wg, _ = rule.download()
    rule.upload(W, H)
    rule.iterate(1, **REG)
    Wi, _ = rule.download()
    rule.upload(W, H)
    li = list(rule.iterate(2, **REG))
    Wi2, Hi2 = rule.download()
    rule.upload(W, H)
    lc = []
    for _ in range(2):
        rule.update_motifs(l1W=L1, l2W=L2)
        lc.append(rule.update_feature_maps(l1H=L1, l2H=L2))
    Wc2, Hc2 = rule.download()
    return lw, sums, Wg, Wi, (li, Wi2, Hi2), (lc, Wc2, Hc2)


def check_losses(got, want, exact, what, cfg, c):
    if exact:
        assert got == want, f"{what} {cfg}: {got} != {want}; launches {reached(c)}"
    else:  # (some 64 x 64 tile sum may exceed 2^24: not exact by construction -- the fallback of tests/test_exact_parity.py)
        np.testing.assert_allclose(got, want, rtol=1e-6)


def flat(loss, sums):
    return [loss] + [v for pair in sums for v in pair]


def references(shape):
    """(mask, X, the W family's (W, H) and reference(), the H family's) of a row, once per shape."""
    N, T, K, L = shape
    mask = ep.mu_mask(N, T)
    Ww, Hw, X = make_problem(N, T, K, L, "W")
    ref_w = reference("W", Ww, Hw, X, mask, shape)
    Wh, Hh, _ = make_problem(N, T, K, L, "H")
    ref_h = reference("H", Wh, Hh, X, mask, shape)
    return mask, X, (Ww, Hw, ref_w), (Wh, Hh, ref_h)


def run_masked_config(cmf, cfg, refs, record=record, worst=_worst):
    """One configuration of a row against references(shape): (W after the W half, H after the H half, launch counters), everything
    test_exact_masked_mu_paths asserts per configuration asserted."""
    mask, X, (Ww, Hw, (W_ref, lw_ref, _, sums_w_ref, exact_w)), (Wh, Hh, (H_ref, lh_ref, lossH_ref, sums_h_ref, exact_h)) = refs
    rule = masked_rule(cmf, cfg, X, Ww, Hw, mask)
    try:
        lw, sums_w, Wg, Wi, (li, Wi2, Hi2), (lc, Wc2, Hc2) = run_w_half(rule, Ww, Hw)
        c = counters(rule)
    finally:
        rule.close()
    assert li == lc, f"{cfg}: iterate(2) losses {li} != call by call {lc}"
    check_same(Wi2, Wc2, "knl", "W after iterate(2)", cfg, "the call-by-call loop", c)
    check_same(Hi2, Hc2, "kt", "H after iterate(2)", cfg, "the call-by-call loop", c)
    rule = masked_rule(cmf, cfg, X, Wh, Hh, mask)
    try:
        lh = rule.compute_loss()
        sums_h = [rule.masked_loss(complement=comp) for comp in (False, True)]
        lh1 = rule.update_feature_maps(l1H=L1, l2H=L2)
        _, Hg = rule.download()
        ch = counters(rule)
    finally:
        rule.close()
    c = {p: c[p] + ch[p] for p in c}
    record(c)
    check_losses(flat(lw, sums_w), flat(lw_ref, sums_w_ref), exact_w, "loss and held-out sums, W family", cfg, c)
    check_losses(flat(lh, sums_h), flat(lh_ref, sums_h_ref), exact_h, "loss and held-out sums, H family", cfg, c)
    np.testing.assert_allclose(lh1, lossH_ref, rtol=1e-5)  # (H is no longer integer: the bar of tests/test_exact_parity.py)
    check_factor(Wg, W_ref, "knl", "masked W half: W", cfg, c)
    check_factor(Hg, H_ref, "kt", "masked H half: H", cfg, c)
    worst["W"] = max(worst["W"], float(ep.ulps(Wg, W_ref).max()))
    worst["H"] = max(worst["H"], float(ep.ulps(Hg, H_ref).max()))
    check_same(Wi, Wg, "knl", "W after iterate(1)", cfg, "update_motifs!", c)
    return Wg, Hg, c


@pytest.mark.parametrize("N,T,K,L,configs,why", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
def test_exact_masked_mu_paths(cmf, N, T, K, L, configs, why):
    shape = (N, T, K, L)
    t0 = time.perf_counter()
    refs = references(shape)
    t_ref = time.perf_counter() - t0
    base = None
    for cfg in ep.divergence_configs(configs, "masked"):
        Wg, Hg, c = run_masked_config(cmf, cfg, refs)
        if base is None:
            base = (cfg, Wg, Hg)
        else:
            check_same(Wg, base[1], "knl", "masked W half: W", cfg, base[0], c)
            check_same(Hg, base[2], "kt", "masked H half: H", cfg, base[0], c)
    _done.add(shape)
    print(f"{shape} {why}: reference {t_ref:.2f} s, total {time.perf_counter() - t0:.2f} s; worst so far W {_worst['W']:.2f} ulp, H {_worst['H']:.2f} ulp")


def test_exact_masked_holes(cmf):
    """One unit and one sample never observed: the unit's entries of W have no term and equal eps exactly, the rest within 2 ulp."""
    N, T, K, L = shape = (130, 700, 32, 20)
    mask = ep.holes_mask(N, T)
    Ww, Hw, X = make_problem(N, T, K, L, "W")
    W_ref, lw_ref, _, sums_ref, exact = reference("W", Ww, Hw, X, mask, shape, holes=True)
    Wh, Hh, _ = make_problem(N, T, K, L, "H")
    H_ref, lh_ref, lossH_ref, sums_h_ref, exact_h = reference("H", Wh, Hh, X, mask, shape, holes=True)
    assert exact and exact_h and np.all(W_ref[:, N // 2, :] == EPS)
    for cfg in (dict(), dict(conv_kernel=2), dict(conv_split=0)):
        rule = masked_rule(cmf, cfg, X, Ww, Hw, mask)
        try:
            lw = rule.compute_loss()
            sums = [rule.masked_loss(complement=comp) for comp in (False, True)]
            rule.update_motifs(l1W=L1, l2W=L2)
            Wg, _ = rule.download()
            c = counters(rule)
        finally:
            rule.close()
        rule = masked_rule(cmf, cfg, X, Wh, Hh, mask)
        try:
            lh1 = rule.update_feature_maps(l1H=L1, l2H=L2)
            _, Hg = rule.download()
        finally:
            rule.close()
        record(c)
        assert flat(lw, sums) == flat(lw_ref, sums_ref), (cfg, flat(lw, sums), flat(lw_ref, sums_ref))
        assert np.all(Wg[:, N // 2, :] == EPS), f"{cfg}: the unobserved unit's entries of W are not eps; launches {reached(c)}"
        check_factor(Wg, W_ref, "knl", "holes: W", cfg, c)
        check_factor(Hg, H_ref, "kt", "holes: H", cfg, c)
        np.testing.assert_allclose(lh1, lossH_ref, rtol=1e-5)


def test_exact_masked_config2_once(cmf):
    """Config 2 itself (N = 2000, T = 50000, K = 32, L = 20) under the mask: the W half and the loss (beside
    tests/test_exact_parity.py::test_exact_config2_once)."""
    N, T, K, L = shape = (2000, 50000, 32, 20)
    mask = ep.mu_mask(N, T)
    W, H, X = make_problem(N, T, K, L, "W")
    W_ref, l_ref, _, sums_ref, exact = reference("W", W, H, X, mask, shape, closed_form=True)
    assert exact and conv3_form(N, T) == "whole+4"
    rule = masked_rule(cmf, {}, X, W, H, mask)
    try:
        lw = rule.compute_loss()
        rule.update_motifs(l1W=L1, l2W=L2)
        Wg, _ = rule.download()
        c = counters(rule)
    finally:
        rule.close()
    record(c)
    assert lw == l_ref, (lw, l_ref)
    check_factor(Wg, W_ref, "knl", "config 2, masked: W", {}, c)
    _done.add("config2")


def test_configurations_the_masked_rule_refuses(cmf):
    """cmf_mu_set_mask refuses the Gram forms and the groups: the configurations exact_problems.divergence_configs leaves out."""
    N, T, K, L, configs, _ = SHAPES[0]
    W, H, X = make_problem(N, T, K, L, "W")
    mask = ep.mu_mask(N, T)
    refused = [c for c in configs if c not in ep.divergence_configs(configs, "masked")]
    assert any("gram" in c for c in refused) and any("devices" in c for c in refused)
    for cfg in refused:
        rule = make_rule(cmf, cfg, X, W, H)
        try:
            with pytest.raises(cmf.CMFError, match="T-sharded groups" if "devices" in cfg else "Gram") as ei:
                rule.set_mask(mask)
            assert ei.value.code == 4
        finally:
            rule.close()


# The paths the masked rule cannot reach, from cmf_mu_set_mask's refusals (cmf_api.hip) -- one reason each:
NOT_UNDER_A_MASK = {
    "gram_w_kernel": "the Gram forms are refused under a mask",
    "gram_lag_corr": "the Gram forms are refused",
    "gram_w_taps": "the Gram forms are refused",
    "gram_h_mfma_kernel": "the Gram forms are refused",
    "gram_h_kernel": "the Gram forms are refused",
    "halo_pack2_kernel": "groups are refused: one device",
    "halo_unpack2_kernel": "groups are refused",
    "halo_pack3_kernel": "groups are refused",
    "halo_unpack3_kernel": "groups are refused",
    "transconv_kernel:front_block": "a shard that updates the columns in front of its own (h_update_impl front = true): groups only",
    "hxt_kernel:nsrc1": "the masked form contracts its two sources (Xm, mask .* est) in one launch (kMuForms: c2_nsrc = 2); one-source "
                        "launches are the groups' halves and the Gram forms, both refused",
    "slab_sum_small_kernel": "with few components the masked form keeps the square fusions (kMuForms: square_fusions): w_update_small_kernel "
                             "sums the C2 slabs itself; the slab sum of its own is launched by the Gram forms and the groups, both refused",
    "slab_sum_small_kernel:carry": "as slab_sum_small_kernel",
}


def test_every_launch_path_reached_under_the_mask():
    """The union of launches:* over this file reaches every named path but those the masked rule refuses."""
    print(f"gpu masked_mu W {_worst['W']:.3g}\ngpu masked_mu H {_worst['H']:.3g}")
    print({p: _seen.get(p, 0) for p in LAUNCH_PATHS})
    if len(_done) < len(SHAPES) + 1:
        pytest.skip("runs after the whole table (the file as a whole)")
    missing = [p for p in LAUNCH_PATHS if p not in NOT_UNDER_A_MASK and not _seen.get(p)]
    extra = [p for p in NOT_UNDER_A_MASK if _seen.get(p)]
    assert not missing, f"launch paths no shape reached under the mask: {missing}"
    assert not extra, f"reached paths the test says the masked rule cannot: {extra}"
