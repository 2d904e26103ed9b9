"""The divergence forms of the MU rule (KL, KL under a mask, Itakura-Saito, beta = 0.5 and 1.5, and Itakura-Saito, beta = 0.5 and 1.5
under a 0/1 mask) ELEMENT BY ELEMENT on every kernel path: the shape table of tests/test_exact_parity.py (exact_problems.SHAPES) under
every configuration a form accepts.

On the integer problems of tests/exact_problems.py est = tensor_conv(W, H) is exact in fp32 on every conv path, so

  1. R, P and Q are element-wise functions of exact operands: every conv tile form stores the same bits, and configurations of one shape
     that differ only in the conv form (conv_kernel, conv_split, reuse_est) give bit-identical W and H;
  2. the contractions that follow sum positive terms, so the updated factor meets the fp64 restatement per element at the form's bar
     (profiles/mu_divergence_elementwise.txt: 8 x the float32 model's worst element, measured on the CPU by
     tools/mu_divergence_elementwise.py).  One positive term missing from one sum moves its element by at least 4 bars
     (exact_problems.sensitivity, asserted here from the arrays generated); the Frobenius-relative 1e-4 of the other divergence tests
     passes a lost strip, lag block or time row (tests/test_exact_problems.py).

The loss: update_feature_maps! returns the restatement's at the form's loss bar; a spotlight problem (data = est but for 64 entries in
each of six chosen tiles) holds compute_loss() to 1e-5 where each spotlight is 1e-3 of the sum, so that one lost or doubled partial
of a cut tile fails by two orders of magnitude.  The launch counters are read per handle, so per form; the last test asserts that
each form reached every path it can reach.

The masked two-array forms (is_mask, beta050_mask, beta150_mask: the option pq_mask) read a sentinel copy of data in two layouts, written
once at install.  The library is handed NaN, +inf, -1 and 0 under the mask (exact_problems.junk_under_mask) while the fp64 reference is
computed from the clean array: one raw value let through, one strip of Q = 1 / e kept where 0 belongs, or the two copies disagreeing is a
surplus or missing term of some sum -- many bars.  The first row installs in the other order too (divergence, then mask), and an
all-ones mask gives the bits of the unmasked form on the large conv forms (test_all_ones_mask_is_the_unmasked_form_on_the_large_forms)."""
import os
import time

import numpy as np
import pytest

import exact_problems as ep
from exact_problems import FORMS, L1, L2, LAUNCH_PATHS, SHAPES, first_bad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = ep.read_bars(os.path.join(ROOT, "profiles", "mu_divergence_elementwise.txt"))
EPS = ep.EPS
SPOT_BAR = 1e-5
VARIANTS = [(form, zeros) for form, f in FORMS.items() for zeros in ((False, True) if f[3] else (False,))]
REG = dict(l1W=L1, l2W=L2, l1H=L1, l2H=L2)
CONV_ONLY = {"conv_kernel", "conv_split", "reuse_est"}  # options that change the conv form alone: the same bits

_seen = {form: {} for form in FORMS}      # launches:<path> per form, summed over every handle of the file
_worst = {form: [0.0, 0.0] for form in FORMS}  # the largest element-wise error and loss error observed per form
_done = set()


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def make_rule(cmf, form, cfg, X, mask, W, H, junk=False, divergence_first=False):
    """A handle in the form.  junk: a masked two-array form is handed exact_problems.junk_under_mask(X, mask) instead of X.
    divergence_first: the divergence is installed before the mask (on the clean array: the unmasked check runs first)."""
    kind, beta, masked = FORMS[form][:3]
    assert not (junk and divergence_first)
    rule = cmf.MultUpdate(ep.junk_under_mask(X, mask) if junk and ep.pq_masked(form) else X, W, H)
    set_divergence = lambda: rule.set_divergence(kind, beta=beta) if beta else rule.set_divergence(kind)  # noqa: E731
    try:
        for name, value in cfg.items():
            rule.set_option(name, value)
        if masked:
            rule.set_option("pq_mask" if ep.pq_masked(form) else "kl_mask", 1)
            if divergence_first:
                set_divergence()
            rule.set_mask(mask)
        if not (masked and divergence_first):
            set_divergence()
    except Exception:
        rule.close()
        raise
    return rule


def counters(rule):
    return {p: rule.counter("launches:" + p) for p in LAUNCH_PATHS}


def record(form, c):
    for p, v in c.items():
        _seen[form][p] = _seen[form].get(p, 0) + v


def reached(c):
    return {p: v for p, v in c.items() if v}


def check_factor(form, got, ref, names, what, cfg, c):
    assert np.isfinite(got).all() and got.min() >= EPS, f"{form} {what} {cfg}: not finite or below eps; launches {reached(c)}"
    _worst[form][0] = max(_worst[form][0], float(ep.rel_err(got, ref).max()))
    msg = ep.check_elementwise(got, ref, BARS["bar"][form], names)
    assert msg is None, f"{form} {what} {cfg}: {msg}; launches {reached(c)}"


def check_same(got, base, names, what, cfg, base_cfg, c):
    if not np.array_equal(got, base):
        raise AssertionError(f"{what} {cfg} differs from {base_cfg} at {first_bad(got != base, names)}; launches {reached(c)}")


def check_loss(form, got, ref, what, cfg, c):
    err = abs(got - ref) / ref
    _worst[form][1] = max(_worst[form][1], err)
    assert err <= BARS["lossbar"][form], f"{form} {what} {cfg}: loss {got!r}, want {ref!r} (rel {err:.2e}, bar {BARS['lossbar'][form]:g}); launches {reached(c)}"


def reference(form, shape, family, zeros):
    """The fp64 half of the form on the shape's problem, with the sensitivity condition asserted from these very arrays."""
    W, H, X, mask = ep.make_divergence_problem(*shape, family, zeros=zeros, relative=FORMS[form][4])
    a = ep.divergence_half(form, family, X, mask, W, H)
    sens = ep.sensitivity(form, a, exact=False)
    if sens < 4 * BARS["bar"][form]:  # (the closed-form bound is a lower bound: the exact value only where it does not decide)
        sens = ep.sensitivity(form, a)
    assert sens >= 4 * BARS["bar"][form], f"{form} {shape} {family}: one term moves an element by {sens:.2e} only (bar {BARS['bar'][form]:g})"
    return W, H, X, mask, a


IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES]


def references(form, shape, zeros):
    """(the W family's reference(), the H family's) of a form on a row, once per shape."""
    return reference(form, shape, "W", zeros), reference(form, shape, "H", zeros)


def run_divergence_config(cmf, form, cfg, K, refs, record=record):
    """One configuration of a row under a form against references(): (W after the W half, H after the H half, launch counters),
    everything test_divergence_mu_paths asserts per configuration asserted."""
    (Ww, Hw, Xw, mask, aw), (Wh, Hh, Xh, _, ah) = refs
    W_ref, H_ref, lossH_ref = aw["new"], ah["new"], ah["loss"]
    rule = make_rule(cmf, form, cfg, Xw, mask, Ww, Hw, junk=True)
    try:
        rule.update_motifs(l1W=L1, l2W=L2)
        Wg, _ = rule.download()
        rule.upload(Ww, Hw)
        rule.iterate(1, **REG)
        Wi, _ = rule.download()
        # pipelined iterations (the loss reduction deferred onto the next launch) are the call-by-call loop, bit for bit
        rule.upload(Ww, Hw)
        li = list(rule.iterate(2, **REG))
        Wi2, Hi2 = rule.download()
        rule.upload(Ww, Hw)
        lc = []
        for _ in range(2):
            rule.update_motifs(l1W=L1, l2W=L2)
            lc.append(rule.update_feature_maps(l1H=L1, l2H=L2))
        Wc2, Hc2 = rule.download()
        c = counters(rule)
    finally:
        rule.close()
    assert li == lc, f"{form} {cfg}: iterate(2) losses {li} != call by call {lc}"
    assert np.isfinite(li).all() and np.isfinite(Wi2).all() and np.isfinite(Hi2).all() and min(Wi2.min(), Hi2.min()) >= EPS
    check_same(Wi2, Wc2, "knl", "W after iterate(2)", cfg, "the call-by-call loop", c)
    check_same(Hi2, Hc2, "kt", "H after iterate(2)", cfg, "the call-by-call loop", c)
    rule = make_rule(cmf, form, cfg, Xh, mask, Wh, Hh, junk=True)
    try:
        lh1 = rule.update_feature_maps(l1H=L1, l2H=L2)
        Wd, Hg = rule.download()
        if cfg == dict(conv_kernel=3) and K % 32 == 0:
            # The loss + store base (what update_feature_maps! ran: est is kept) and the loss-only base (reuse_est = 0) run on the
            # same one-wave tiles with the same cut, and their terms are rounded alike (cmf_kernels.h at cmf_is_term): the same
            # partials in the same order, so the same bits.  The factors are uploaded again so that the loss is computed anew.
            rule.set_option("reuse_est", 0)
            rule.upload(Wd, Hg)
            l_only = rule.compute_loss()
            assert l_only == lh1, f"{form} {cfg}: the loss-only base gives {l_only!r}, loss + store gave {lh1!r}"
        ch = counters(rule)
    finally:
        rule.close()
    c = {p: c[p] + ch[p] for p in c}
    record(form, c)
    check_loss(form, lh1, lossH_ref, "update_feature_maps!", cfg, c)
    check_factor(form, Wg, W_ref, "knl", "W half: W", cfg, c)
    check_factor(form, Hg, H_ref, "kt", "H half: H", cfg, c)
    check_same(Wi, Wg, "knl", "W after iterate(1)", cfg, "update_motifs!", c)
    return Wg, Hg, c


@pytest.mark.parametrize("form,zeros", VARIANTS, ids=[f + ("+zeros" if z else "") for f, z in VARIANTS])
@pytest.mark.parametrize("N,T,K,L,configs,why", SHAPES, ids=IDS)
def test_divergence_mu_paths(cmf, N, T, K, L, configs, why, form, zeros):
    shape = (N, T, K, L)
    t0 = time.perf_counter()
    refs = references(form, shape, zeros)
    t_ref = time.perf_counter() - t0
    base = None
    for cfg in ep.divergence_configs(configs, form):
        Wg, Hg, c = run_divergence_config(cmf, form, cfg, K, refs)
        if base is None:
            base = (cfg, Wg, Hg)
        elif set(cfg) <= CONV_ONLY and set(base[0]) <= CONV_ONLY:
            check_same(Wg, base[1], "knl", "W half: W", cfg, base[0], c)
            check_same(Hg, base[2], "kt", "H half: H", cfg, base[0], c)
    if ep.pq_masked(form) and shape == SHAPES[0][:4]:
        # The other order of installation: divergence first (on the clean array, which the unmasked check reads), then the mask.  Both end in
        # the same form, but the sentinel copies are written at another moment: the same bits.
        for (W0, H0, X, mask, _), half, names in ((refs[0], 0, "knl"), (refs[1], 1, "kt")):
            rule = make_rule(cmf, form, base[0], X, mask, W0, H0, divergence_first=True)
            try:
                rule.update_motifs(l1W=L1, l2W=L2) if half == 0 else rule.update_feature_maps(l1H=L1, l2H=L2)
                got, c = rule.download()[half], counters(rule)
            finally:
                rule.close()
            check_same(got, base[1 + half], names, "divergence installed before the mask: " + "WH"[half], base[0], "mask first", c)
    _done.add((shape, form, zeros))
    print(f"{form}{'+zeros' if zeros else ''} {shape} {why}: reference {t_ref:.2f} s, total {time.perf_counter() - t0:.2f} s; "
          f"worst so far {_worst[form][0]:.2e} (bar {BARS['bar'][form]:g}), loss {_worst[form][1]:.2e} (bar {BARS['lossbar'][form]:g})")


# ---- the spotlight loss --------------------------------------------------------------------------------------------------------
SPOT_SHAPES = [s[:4] + (dict(),) for s in SHAPES[:5]] + [(1000, 4100, 8, 10, dict()), (200, 1500, 32, 33, dict(conv_kernel=2, reuse_est=0))]
assert all(s[:4] in [r[:4] for r in SHAPES] for s in SPOT_SHAPES)
IS_BACKGROUND = 2.0 ** -44  # |(r - 1) - log r| of a background entry in fp32: r = est * fl(1 / est) is within an ulp of 1, the term within a few ulp(2^-23) of 0


def spotlight_tiles(N, T, K, n_cu=ep.N_CU):
    """(t block, n block) of the six chosen 64 x 64 tiles of the loss conv's one-wave grid (tile index = n block fastest): the first, the
    last whole tile before the cut, the first and last cut tile, one of the last (partial) tile row, one of the last, partly padded
    n block.  Grids without a cut take the middle and the last tile instead.  n_cu: the CU count the grid is planned for."""
    gx, rows = ep.rup(N, 128) // 64, (T + 63) // 64
    live_gx = (N + 63) // 64  # (n blocks that are all padding hold no entry)
    n_full, cut = ep.conv3_cut(N, T, n_cu=n_cu)[:2] if K % 32 == 0 else ep.conv_small_form(N, T, n_cu=n_cu)
    tiles = gx * rows
    ids = [0, max(n_full - 1, 0), n_full % tiles, tiles - 1] if 0 < cut < tiles else [0, tiles // 3, tiles // 2, tiles - 1]
    out = [(i // gx, min(i % gx, live_gx - 1)) for i in ids]
    out += [(rows - 1, 0), (rows // 2, live_gx - 1)]
    return list(dict.fromkeys(out))


def spotlight_problem(form, N, T, K, L, n_cu=ep.N_CU):
    """(W, H, X, mask, spots, held): the W family's factors with H's first column raised to L (est is then 20 ... 78 at L = 20 from the
    first column on, not 1 ...), data = est except at the spotlights: 64 per chosen tile, one per row and per column and four in every
    16 x 16 block, each 2 est or est / 2.  held: the
    spotlights under mask == 0 (every fourth; all ones elsewhere)."""
    import kl_mu_restatement as kr

    W, H, _ = ep.make_problem(N, T, K, L, "W")
    H[np.argmax(H[:, 0]), 0] = float(L)
    est = kr.tensor_conv(W, H)
    assert est.min() >= 1 and est.max() < ep.EXACT and np.all(est == np.round(est))
    i = np.arange(64)
    nn, tt = [], []
    for tb, nb in spotlight_tiles(N, T, K, n_cu):
        n, t = nb * 64 + i, tb * 64 + (i % 4) * 16 + i // 4
        ok = (n < N) & (t < T)
        nn.append(n[ok]), tt.append(t[ok])
    nn, tt = np.concatenate(nn), np.concatenate(tt)
    e = est[nn, tt]
    X = est.copy()
    mask = np.ones((N, T))
    # every other spotlight on an est above the spotlights' median is halved, the rest are doubled: both kinds occur, and the halved
    # ones (the smaller term of the two) sit where est is large, which keeps the terms within an order of magnitude of each other
    half = (np.arange(len(nn)) % 2 == 1) & (e >= np.median(e))
    X[nn, tt] = np.where(half, 0.5, 2.0) * e
    terms = spot_terms(form, X[nn, tt], e)
    held = np.arange(len(nn)) % 4 == 3
    mask[nn[held], tt[held]] = 0.0
    return W, H, np.asfortranarray(X), np.asfortranarray(mask), (nn, tt, terms, half), held


def spot_terms(form, x, e):
    """The divergence term of each entry in fp64 (e = est: est + eps is est in fp64 from 1 on)."""
    import beta_mu_restatement as br

    kind, beta = FORMS[form][:2]
    if kind == ":kl":
        return x * np.log(x / e) - x + e
    if kind == ":itakura_saito":
        return (x / e - 1.0) - np.log(x / e)
    return br.terms_direct(x, e, beta)


def run_spotlight(cmf, N, T, K, L, cfg, form, n_cu=ep.N_CU, record=record):
    """The spotlight loss of a form on a shape whose handle is planned for n_cu CUs: everything test_spotlight_loss asserts."""
    W, H, X, mask, (nn, tt, terms, half), held = spotlight_problem(form, N, T, K, L, n_cu)
    masked = FORMS[form][2]
    counted = ~held if masked else np.ones(len(nn), bool)
    total = terms[counted].sum()
    # every spotlight is at least 1e-3 of the sum, both kinds occur, and the background is nothing beside the bar
    assert terms[counted].min() >= 1e-3 * total and half.any() and not half.all(), (terms.min() / total, half.mean())
    background = IS_BACKGROUND * N * T if FORMS[form][0] == ":itakura_saito" else 0.0
    assert background <= 0.1 * SPOT_BAR * total
    want = ep.divergence_loss(form, X, mask, W, H)
    # (what the loss is divided by: the data's sum under KL, the number of entries -- observed entries under a mask -- otherwise)
    norm = (X[mask != 0].sum() if masked else X.sum()) if FORMS[form][0] == ":kl" else float((mask != 0).sum()) if masked else float(N * T)
    out = X[mask == 0].sum() if FORMS[form][0] == ":kl" else float((mask == 0).sum())  # cmf_masked_loss's second return over the held-out entries
    assert abs(want * norm - total) <= 1e-9 * total  # (the restatement's loss is the spotlights' terms: the background is 0 in fp64)
    rule = make_rule(cmf, form, cfg, X, mask, W, H)
    try:
        got = rule.compute_loss()
        if masked:  # the complement score counts the held-out spotlights and only them
            d, s = rule.masked_loss(complement=True)
            assert abs(d - terms[held].sum()) <= SPOT_BAR * terms[held].sum() and abs(s - out) <= 1e-6 * s, (d, terms[held].sum(), s, out)
            d1, s1 = rule.masked_loss(complement=False)
            assert abs(d1 - total) <= SPOT_BAR * total and abs(s1 - norm) <= 1e-6 * norm
        c = counters(rule)
    finally:
        rule.close()
    record(form, c)
    print(f"spotlight {form} {(N, T, K, L)} {cfg}: {len(nn)} spotlights, smallest {terms[counted].min() / total:.2e} of the sum, loss rel {abs(got - want) / want:.2e}; {reached(c)}")
    assert abs(got - want) <= SPOT_BAR * want, f"{form} {cfg}: compute_loss {got!r}, want {want!r}; launches {reached(c)}"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("N,T,K,L,cfg", SPOT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SPOT_SHAPES])
def test_spotlight_loss(cmf, N, T, K, L, cfg, form):
    run_spotlight(cmf, N, T, K, L, cfg, form)
    _done.add(("spot", (N, T, K, L), form))


# ---- an all-ones mask is the unmasked form, on the table's large conv forms -------------------------------------------------------
# tests/test_gpu_masked_pq_mu.py holds this on seven small shapes; here the shapes of exact_problems.CU_EPILOGUE_ROWS (one per conv3 form
# at 32 CUs, two few-component rows) under the default configuration at the chip's own CU count.  With nothing held out the sentinel
# copies are the data, so the masked families' epilogues must store the bits of the unmasked ones: W after the W half, H after the H half.
ONES_SHAPES = [r[:4] for r in ep.CU_EPILOGUE_ROWS]
ONES_FORMS = {"is": "is_mask", "beta050": "beta050_mask"}
assert len(ONES_SHAPES) == 7


@pytest.mark.parametrize("form", list(ONES_FORMS))
@pytest.mark.parametrize("N,T,K,L", ONES_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in ONES_SHAPES])
def test_all_ones_mask_is_the_unmasked_form_on_the_large_forms(cmf, N, T, K, L, form):
    conv = [p for p in LAUNCH_PATHS if p.startswith("conv")]
    for family, half, names in (("W", 0, "knl"), ("H", 1, "kt")):
        W, H, X, mask = ep.make_divergence_problem(N, T, K, L, family, relative=FORMS[form][4])
        got = []
        for f, m in ((form, mask), (ONES_FORMS[form], np.ones_like(mask))):
            rule = make_rule(cmf, f, dict(), X, m, W, H)
            try:
                rule.update_motifs(l1W=L1, l2W=L2) if half == 0 else rule.update_feature_maps(l1H=L1, l2H=L2)
                got.append((rule.download()[half], counters(rule)))
            finally:
                rule.close()
        (plain, cp), (ones, c) = got
        assert np.isfinite(plain).all() and plain.min() >= EPS
        check_same(ones, plain, names, f"{ONES_FORMS[form]} under an all-ones mask: " + "WH"[half], dict(), f"the unmasked {form}", c)
        assert {p for p in conv if c[p]} == {p for p in conv if cp[p]}, (reached(c), reached(cp))
        # (which conv forms the chip's own plan gave this shape: several of these rows share one at the full CU count)
        print(f"all-ones {form} {(N, T, K, L)} {family} half: conv forms reached {sorted(p for p in conv if c[p])}")
    _done.add(("ones", (N, T, K, L), form))


# ---- coverage -------------------------------------------------------------------------------------------------------------------
# The paths NO divergence form reaches, from kMuForms and launch_conv (cmf_internal.h) -- one reason each:
NOT_FOR_DIVERGENCES = {
    "gram_w_kernel": "the Gram form is refused under a divergence (cmf_mu_set_divergence)",
    "gram_lag_corr": "the Gram form is refused",
    "gram_w_taps": "the Gram form is refused",
    "gram_h_mfma_kernel": "the Gram form is refused",
    "gram_h_kernel": "the Gram form is refused",
    "halo_pack2_kernel": "groups are refused: one device",
    "halo_unpack2_kernel": "groups are refused",
    "halo_pack3_kernel": "groups are refused",
    "halo_unpack3_kernel": "groups are refused",
    "transconv_kernel:front_block": "a shard that updates the columns in front of its own (h_update_impl front = true): groups only",
    "g_gemm_fold_small_kernel:fused_h": "the H update inside the C3 launch is a square fusion (MuForm::square_fusions is false)",
}
# ... and per form: KL contracts one source in C2 (its denominators are sums), every other form two; the masked KL terms have no
# 128 x 128 tiles (conv_on_tiles128: family KL_MASKED is not on them; the other forms reach conv2_kernel through the loss-only base alone,
# which is what the spotlight handle with conv_kernel = 2 and reuse_est = 0 runs)
# The masked two-array families are on the 128 x 128 tiles in their loss-only mode alone as well (conv_on_tiles128), the held-out score included.
NOT_FOR_FORM = {"kl": {"hxt_kernel:nsrc2"}, "kl_mask": {"hxt_kernel:nsrc1", "conv2_kernel"}, "is": {"hxt_kernel:nsrc1"},
                "beta050": {"hxt_kernel:nsrc1"}, "beta150": {"hxt_kernel:nsrc1"}, "is_mask": {"hxt_kernel:nsrc1"},
                "beta050_mask": {"hxt_kernel:nsrc1"}, "beta150_mask": {"hxt_kernel:nsrc1"}}


def expected_paths(form):
    return [p for p in LAUNCH_PATHS if p not in NOT_FOR_DIVERGENCES and p not in NOT_FOR_FORM[form]]


def test_every_form_reached_every_path_it_can():
    """Per form, the union of launches:* over the table and the spotlight handles is exactly the expected set: a new instance, or a form
    gaining a path, cannot land untested.  Also prints the worst element-wise and loss errors observed per form (the `gpu` lines of
    profiles/mu_divergence_elementwise.txt)."""
    for form in FORMS:
        print(f"gpu {form} {_worst[form][0]:.3g}\ngpuloss {form} {_worst[form][1]:.3g}")
    want = len(SHAPES) * len(VARIANTS) + len(SPOT_SHAPES) * len(FORMS) + len(ONES_SHAPES) * len(ONES_FORMS)
    if len(_done) < want:
        pytest.skip("runs after the whole table (the file as a whole)")
    for form in FORMS:
        got = {p for p, v in _seen[form].items() if v}
        print(form, {p: _seen[form].get(p, 0) for p in LAUNCH_PATHS})
        missing = [p for p in expected_paths(form) if p not in got]
        extra = sorted(got - set(expected_paths(form)))
        assert not missing, f"{form}: launch paths no shape reached: {missing}"
        assert not extra, f"{form}: reached paths the test says it cannot: {extra}"
