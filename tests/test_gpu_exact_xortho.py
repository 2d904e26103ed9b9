"""seqNMF's cross-orthogonality penalties on the MU rule against fp64 ELEMENT BY ELEMENT, on every kernel path (cmf_mu_set_xortho,
cmf_xortho.hip, cmf_xortho.h; the norm-wise tests and the exact terms by another route are in tests/test_gpu_xortho_mu.py).

On the integer problems of tests/exact_problems.py with data % 4 every quantity the penalties add -- G = off(S(H)), xW = hxt(G, data),
xH = off(S(numH)), oW = off(Wflat) -- is a sum of non-negative integers below 2^24, and with the dyadic weights XO_WEIGHTS the weighted
denominators are exact in fp32 in any order and under any fma contraction (exact_problems.xortho_preconditions asserts it from the
arrays of every row before the GPU is asked).  The only rounding left is cmf_mu's one division and one multiply: the bar is the 2 ulp
of tests/test_exact_parity.py, and one unit of any of the sums moves its element by at least four bars.  What is compared is what the
UPDATE computes: the two-source C3 slabs summed into the penalties' table, xo_off_kernel in its fused form base + (lam off + lam2 g),
xo_fold_w_kernel, and the penalty contraction hxt_contract(left = G) with its chunk tails -- under every configuration of the shape
table the penalties accept, each of which must give the bits of the first.  tests/test_gpu_exact_cu_plans.py runs run_xortho_config
under plans for fewer compute units.

The state tests hold the bookkeeping around G (g_gen against est_gen, w_g, xo_after_w) and the scratch tables the cost and terms entries
share with the update (S, AD, xW) bitwise to a fresh handle, and to fp64 where the factors are integers."""
import time

import numpy as np
import pytest

import exact_problems as ep
from exact_problems import L1, L2, LAUNCH_PATHS, SHAPES, XO_FOLD_ROW, XO_WEIGHTS, first_bad, ulps

pytestmark = pytest.mark.gpu

ULP_BAR = 2  # tests/test_exact_parity.py's, taken over
REG = dict(l1W=L1, l2W=L2, l1H=L1, l2H=L2)
XO_COUNTERS = ("xortho_launches", "small_k_fused_h_updates", "speculated_contractions")

_seen = {}                     # launches:<path> summed over every handle of the table and the fold row
_done = set()
_worst = {"W": 0.0, "H": 0.0}  # the worst ulp observed per half over the file


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def counters(rule):
    return {p: rule.counter("launches:" + p) for p in LAUNCH_PATHS}


def record(c):
    for p, v in c.items():
        _seen[p] = _seen.get(p, 0) + v


def reached(c):
    return {p: v for p, v in c.items() if v}


def make_rule(cmf, cfg, X, W, H, weights, **kw):
    rule = cmf.MultUpdate(X, W, H, **kw)
    try:
        for name, value in cfg.items():
            rule.set_option(name, value)
        rule.set_xortho(*weights)
    except Exception:
        rule.close()
        raise
    return rule


def check_factor(got, ref, names, what, cfg, c, half=None, worst=_worst):
    u = ulps(got, ref)
    if half:
        worst[half] = max(worst[half], float(u.max()))
    if not (u.max() <= ULP_BAR):
        i = tuple(np.argwhere(~(u <= ULP_BAR))[0])
        raise AssertionError(f"{what} {cfg}: {u.max():.1f} ulp from fp64 at {first_bad(~(u <= ULP_BAR), names)} (got {got[i]!r}, want {ref[i]!r}; "
                             f"{int((~(u <= ULP_BAR)).sum())} elements over the bar); launches {reached(c)}")


def check_same(got, base, names, what, cfg, base_cfg, c=None):
    if not np.array_equal(got, base):
        raise AssertionError(f"{what} {cfg} differs from {base_cfg} at {first_bad(got != base, names)}" + (f"; launches {reached(c)}" if c else ""))


def xortho_references(shape, both=True):
    """The two integer problems of a shape and their fp64 halves under XO_WEIGHTS with every table kept (exact_problems.xortho_half),
    the preconditions asserted from the arrays: once per shape.  reference() finishes them under other weights."""
    r = dict(shape=shape, refs={})
    for family in ("W", "H") if both else ("W",):
        W, H, X = ep.make_xortho_problem(*shape, family)
        r[family] = ep.xortho_half(family, X, W, H, XO_WEIGHTS)
    return r


def reference(r, family, weights):
    """xortho_half of the family under the weights (from the tables of xortho_references), its preconditions asserted."""
    key = (family, tuple(weights))
    if key not in r["refs"]:
        a = ep.xortho_finish(r[family], weights)
        a["pre"] = ep.xortho_preconditions(a, f"{r['shape']} {family} {tuple(weights)}")
        r["refs"][key] = a
    return r["refs"][key]


def run_xortho_config(cmf, cfg, refs, weights=XO_WEIGHTS, record=record, worst=_worst):
    """One configuration of a row under the weights against xortho_references(): (W after the W half, H after the H half, launch
    counters), everything test_exact_xortho_paths asserts per configuration asserted."""
    aw, ah = reference(refs, "W", weights), reference(refs, "H", weights)
    what = f"{refs['shape']} weights {tuple(weights)}"
    rule = make_rule(cmf, cfg, aw["X"], aw["W"], aw["H"], weights)
    try:
        rule.update_motifs(l1W=L1, l2W=L2)
        Wg, _ = rule.download()
        rule.upload(aw["W"], aw["H"])
        rule.iterate(1, **REG)
        Wi, _ = rule.download()
        # pipelined iterations (the loss reduction deferred onto the next launch) are the call-by-call loop, bit for bit
        rule.upload(aw["W"], aw["H"])
        li = list(rule.iterate(2, **REG))
        Wi2, Hi2 = rule.download()
        rule.upload(aw["W"], aw["H"])
        lc = []
        for _ in range(2):
            rule.update_motifs(l1W=L1, l2W=L2)
            lc.append(rule.update_feature_maps(l1H=L1, l2H=L2))
        Wc2, Hc2 = rule.download()
        c = counters(rule)
        xc = {n: rule.counter(n) for n in XO_COUNTERS}
    finally:
        rule.close()
    rule = make_rule(cmf, cfg, ah["X"], ah["W"], ah["H"], weights)
    try:
        lh1 = rule.update_feature_maps(l1H=L1, l2H=L2)
        _, Hg = rule.download()
        ch = counters(rule)
        xh = {n: rule.counter(n) for n in XO_COUNTERS}
    finally:
        rule.close()
    c = {p: c[p] + ch[p] for p in c}
    record(c)
    # (lambda_W alone launches nothing of the penalties' on the H side: the handle that ran update_feature_maps! only has none to count)
    h_side = weights[0] > 0 or weights[1] > 0
    assert xc["xortho_launches"] > 0 and (xh["xortho_launches"] > 0) == h_side, f"{what} {cfg}: {xc} {xh}"
    for x in (xc, xh):
        assert x["small_k_fused_h_updates"] == 0 and x["speculated_contractions"] == 0, f"{what} {cfg}: {x}"
    assert li == lc, f"{what} {cfg}: iterate(2) losses {li} != call by call {lc}"
    assert np.isfinite(li).all()
    check_same(Wi2, Wc2, "knl", f"{what}: W after iterate(2)", cfg, "the call-by-call loop", c)
    check_same(Hi2, Hc2, "kt", f"{what}: H after iterate(2)", cfg, "the call-by-call loop", c)
    uw, uh = float(ulps(Wg, aw["new"]).max()), float(ulps(Hg, ah["new"]).max())
    print(f"{what} {cfg}: W half {uw:.2f} ulp, H half {uh:.2f} ulp, loss rel {abs(lh1 - ah['loss']) / ah['loss']:.2e}")
    check_factor(Wg, aw["new"], "knl", f"{what}: W half: W", cfg, c, "W", worst)
    check_factor(Hg, ah["new"], "kt", f"{what}: H half: H", cfg, c, "H", worst)
    np.testing.assert_allclose(lh1, ah["loss"], rtol=1e-5, err_msg=f"{what} {cfg}: the loss update_feature_maps! returns")
    check_same(Wi, Wg, "knl", f"{what}: W after iterate(1)", cfg, "update_motifs!", c)
    return Wg, Hg, c


IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES]


@pytest.mark.parametrize("N,T,K,L,configs,why", SHAPES, ids=IDS)
def test_exact_xortho_paths(cmf, N, T, K, L, configs, why):
    shape = (N, T, K, L)
    t0 = time.perf_counter()
    refs = xortho_references(shape)
    t_ref = time.perf_counter() - t0
    base = None
    for cfg in ep.xortho_configs(configs):
        Wg, Hg, c = run_xortho_config(cmf, cfg, refs)
        if base is None:
            base = (cfg, Wg, Hg)
            for weights in ep.xo_weight_sets()[1:]:  # each weight alone: the other sides launch nothing of their own
                run_xortho_config(cmf, cfg, refs, weights)
        else:  # num and den are exact and the same cmf_mu is applied: every configuration gives the bits of the first
            check_same(Wg, base[1], "knl", "W half: W", cfg, base[0], c)
            check_same(Hg, base[2], "kt", "H half: H", cfg, base[0], c)
    weakest = min((a["pre"]["weakest"][::-1] + (k,) for k, a in refs["refs"].items()))
    _done.add(shape)
    print(f"{shape} {why}: references {t_ref:.2f} s, total {time.perf_counter() - t0:.2f} s; the weakest term of the row: {weakest[1]} "
          f"{weakest[0]:.1f} ulp under {weakest[2]}; worst so far W {_worst['W']:.2f} ulp, H {_worst['H']:.2f} ulp")


def test_fold_takes_a_second_pass(cmf):
    """xo_fold_w_kernel's grid-stride loop comes round a second time: L K32 Np / 4 float4 lanes against 2048 x 256 threads.  No row of
    the table is that large in W (config 2 itself is not); the W half of XO_FOLD_ROW at the same bar."""
    N, T, K, L = XO_FOLD_ROW
    refs = xortho_references(XO_FOLD_ROW, both=False)
    a = reference(refs, "W", XO_WEIGHTS)
    rule = make_rule(cmf, {}, a["X"], a["W"], a["H"], XO_WEIGHTS)
    try:
        K32, Np = ep.rup(rule.K, 32), ep.rup(rule.N, 128)  # (the handle's padded dimensions: cmf_create)
        assert ep.xo_fold_passes(K32, Np, rule.L) >= 2, (K32, Np, rule.L)
        rule.update_motifs(l1W=L1, l2W=L2)
        Wg, _ = rule.download()
        c = counters(rule)
        assert rule.counter("xortho_launches") > 0
    finally:
        rule.close()
    record(c)
    print(f"{XO_FOLD_ROW}: W half {float(ulps(Wg, a['new']).max()):.2f} ulp; the weakest term {a['pre']['weakest']}")
    check_factor(Wg, a["new"], "knl", "the fold's second pass: W", {}, c, "W")
    _done.add(XO_FOLD_ROW)


# ---- the state around G and the shared scratch tables -----------------------------------------------------------------------------
STATE_ROWS = [(90, 610, 5, 7), (130, 700, 32, 20)]  # one row of the few-component kernels, one of the general ones


def fresh(cmf, X, W, H, weights, calls):
    """The factors after `calls` ("W": update_motifs!, "H": update_feature_maps!) on a new handle."""
    rule = make_rule(cmf, {}, X, W, H, weights)
    try:
        for call in calls:
            rule.update_motifs(l1W=L1, l2W=L2) if call == "W" else rule.update_feature_maps(l1H=L1, l2H=L2)
        return rule.download()
    finally:
        rule.close()


def second_H(family, shape):
    """Another integer H for the same W and data: the family's H of seed 1."""
    return ep.make_problem(*shape, family, seed=1)[1]


@pytest.mark.parametrize("between", ["nothing", "terms", "cost"])
@pytest.mark.parametrize("family,weights", [("W", XO_WEIGHTS), ("H", (0.0, XO_WEIGHTS[1], 0.0))], ids=["W_side_all_weights", "H_side_lambda_H_alone"])
@pytest.mark.parametrize("shape", STATE_ROWS, ids=str)
def test_G_follows_H(cmf, shape, family, weights, between):
    """G is rebuilt when H has changed and only then: a rule call on (W, H_a), the terms or cost entry (G becomes current for the H of
    that moment), upload(W, H_b), the rule call again -- the result is that of a fresh handle on (W, H_b), bit for bit, and the fp64
    update of (W, H_b) at 2 ulp.  With lambda_H alone it is the H side that builds G."""
    W, H_a, X = ep.make_xortho_problem(*shape, family)
    H_b = second_H(family, shape)
    assert not np.array_equal(H_a, H_b)
    a = ep.xortho_half(family, X, W, H_b, weights)
    ep.xortho_preconditions(a, f"{shape} {family} second H")
    i, names = (0, "knl") if family == "W" else (1, "kt")
    rule = make_rule(cmf, {}, X, W, H_a, weights)
    try:
        step = (lambda: rule.update_motifs(l1W=L1, l2W=L2)) if family == "W" else (lambda: rule.update_feature_maps(l1H=L1, l2H=L2))
        step()
        if between == "terms":
            rule.xortho_terms()
        elif between == "cost":
            rule.xortho_cost()
        rule.upload(W, H_b)
        step()
        got = rule.download()[i]
    finally:
        rule.close()
    check_same(got, fresh(cmf, X, W, H_b, weights, family)[i], names, f"{shape} {family}: after upload(W, H_b)", between, "a fresh handle")
    check_factor(got, a["new"], names, f"{shape} {family}: after upload(W, H_b), {between} in between", {}, {})


@pytest.mark.parametrize("shape", STATE_ROWS, ids=str)
def test_terms_and_cost_between_rule_calls_change_nothing(cmf, shape):
    """xortho_terms() and xortho_cost() pass through S, AD, xW, the C2 and the C3 slabs, which the update uses too: called between
    update_motifs! and update_feature_maps! and between two iterations, they leave W, H and the losses those of an uninterrupted run."""
    W, H, X = ep.make_xortho_problem(*shape, "W")
    want = None
    for probe in (None, "terms", "cost", "both"):
        rule = make_rule(cmf, {}, X, W, H, XO_WEIGHTS)
        try:
            losses = []
            for it in range(2):
                rule.update_motifs(l1W=L1, l2W=L2)
                if probe in ("terms", "both"):
                    rule.xortho_terms()
                if probe in ("cost", "both"):
                    rule.xortho_cost()
                losses.append(rule.update_feature_maps(l1H=L1, l2H=L2))
                if probe in ("cost", "both"):
                    rule.xortho_cost()
                if probe in ("terms", "both"):
                    rule.xortho_terms()
            got = rule.download() + (losses,)
        finally:
            rule.close()
        if want is None:
            want = got
            continue
        check_same(got[0], want[0], "knl", f"{shape}: W after two iterations", probe, "the uninterrupted run")
        check_same(got[1], want[1], "kt", f"{shape}: H after two iterations", probe, "the uninterrupted run")
        assert got[2] == want[2], (probe, got[2], want[2])


@pytest.mark.parametrize("shape", STATE_ROWS, ids=str)
def test_weights_changed_between_calls(cmf, shape):
    """lambda alone, all three, lambda_W alone on ONE handle, the factors uploaded again in between: each update_motifs! and each
    update_feature_maps! is that of a fresh handle with those weights, and the W half is the fp64 one at 2 ulp."""
    refs = xortho_references(shape, both=False)
    aw = refs["W"]
    X, W, H = aw["X"], aw["W"], aw["H"]
    lam, lamH, lamW = XO_WEIGHTS
    rule = make_rule(cmf, {}, X, W, H, (0.0, 0.0, 0.0))
    try:
        for weights in ((lam, 0.0, 0.0), XO_WEIGHTS, (0.0, 0.0, lamW)):
            rule.set_xortho(*weights)
            rule.upload(W, H)
            rule.update_motifs(l1W=L1, l2W=L2)
            W1, _ = rule.download()
            rule.update_feature_maps(l1H=L1, l2H=L2)
            W2, H2 = rule.download()
            Wf, Hf = fresh(cmf, X, W, H, weights, "WH")
            check_same(W1, Wf, "knl", f"{shape}: W after update_motifs!", weights, "a fresh handle")
            check_same(W2, Wf, "knl", f"{shape}: W after update_feature_maps!", weights, "a fresh handle")
            check_same(H2, Hf, "kt", f"{shape}: H after update_feature_maps!", weights, "a fresh handle")
            check_factor(W1, reference(refs, "W", weights)["new"], "knl", f"{shape}: W half under {weights} on a handle that had other weights", {}, {})
    finally:
        rule.close()


@pytest.mark.parametrize("shape", STATE_ROWS, ids=str)
def test_an_H_edited_in_the_callers_array_rebuilds_G(cmf, shape):
    """Under sync_every_call the rule reads the arrays it is handed: an H edited in place reaches the device
    through cmf_set_factors(NULL, H), and G must follow it like it follows upload()."""
    W, H_a, X = ep.make_xortho_problem(*shape, "W")
    H_b = second_H("W", shape)
    a = ep.xortho_half("W", X, W, H_b, XO_WEIGHTS)
    ep.xortho_preconditions(a, f"{shape} W second H")
    Wc, Hc = W.copy(order="F"), H_a.copy(order="F")
    rule = make_rule(cmf, {}, X, Wc, Hc, XO_WEIGHTS, sync_every_call=True, verify_args="full")
    try:
        rule.xortho_terms()  # G is current for H_a
        Hc[...] = H_b
        rule.update_motifs(X, Wc, Hc, l1W=L1, l2W=L2)
        assert rule.reuploads == 1
        W1, H1 = rule.download()
        np.testing.assert_array_equal(H1, H_b)
        check_same(W1, fresh(cmf, X, W, H_b, XO_WEIGHTS, "W")[0], "knl", f"{shape}: W after an H edited in place", {}, "a fresh handle")
        check_factor(W1, a["new"], "knl", f"{shape}: W after an H edited in place", {}, {})
        # ... and once more behind an update (w_g / xo_after_w have run): H_a back in the caller's array, the W of the device kept
        Hc[...] = H_a
        rule.update_motifs(X, Wc, Hc, l1W=L1, l2W=L2)
        W2, _ = rule.download()
    finally:
        rule.close()
    check_same(W2, fresh(cmf, X, W1, H_a, XO_WEIGHTS, "W")[0], "knl", f"{shape}: W after a second edit of H", {}, "a fresh handle on the first result")


# ---- coverage -------------------------------------------------------------------------------------------------------------------
# The paths the penalised rule cannot reach, from cmf_mu_set_xortho's refusals and mu_fusions (cmf_internal.h) -- one reason each:
NOT_FOR_PENALTIES = {
    "gram_w_kernel": "the Gram form is refused under the penalties (cmf_mu_install.h)",
    "gram_lag_corr": "the Gram form is refused",
    "gram_w_taps": "the Gram form is refused",
    "gram_h_mfma_kernel": "the Gram form is refused",
    "gram_h_kernel": "the Gram form is refused",
    "halo_pack2_kernel": "groups are refused: one device",
    "halo_unpack2_kernel": "groups are refused",
    "halo_pack3_kernel": "groups are refused",
    "halo_unpack3_kernel": "groups are refused",
    "transconv_kernel:front_block": "a shard that updates the columns in front of its own (h_update_impl front = true): groups only",
    "g_gemm_fold_small_kernel:fused_h": "the H update inside the C3 launch is a fusion, and mu_fusions is false while a weight is positive: "
                                        "the penalised H update needs numH as a finished table before it can form the denominator",
}
# Everything else is expected: hxt_kernel:nsrc2 is the rule's own C2 contraction and hxt_kernel:nsrc1 the penalty contraction with G as
# the left operand; both slab sums and their :carry forms run because the unfused W phase sums its slabs in a launch of its own, which
# takes the loss deferred by iterate(2).


def expected_paths():
    return [p for p in LAUNCH_PATHS if p not in NOT_FOR_PENALTIES]


def test_every_path_the_penalised_rule_can_reach():
    """The union of launches:* over the table and the fold row is exactly the expected set: a new instance, or the penalised rule gaining
    a path, cannot land untested.  Prints the worst ulp observed per half (DESIGN.md 6a-X quotes it)."""
    print(f"worst W half {_worst['W']:.3g} ulp, worst H half {_worst['H']:.3g} ulp (bar {ULP_BAR})")
    if len(_done) < len(SHAPES) + 1:
        pytest.skip("runs after the whole table (the file as a whole)")
    got = {p for p, v in _seen.items() if v}
    print({p: _seen.get(p, 0) for p in LAUNCH_PATHS})
    missing = [p for p in expected_paths() if p not in got]
    extra = sorted(got - set(expected_paths()))
    assert not missing, f"launch paths no row reached under the penalties: {missing}"
    assert not extra, f"reached paths the test says the penalised rule cannot: {extra}"
