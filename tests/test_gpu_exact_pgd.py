"""The PGD rule (conv family CONV_FAM_PGD, modes 4-7: the residual, its transpose, the masked residual, the AbsoluteLoss sign; the
one-source contractions hxt_kernel:nsrc1 and launch_transconv(h, 1, ...)) against the fp64 oracle ELEMENT BY ELEMENT on every kernel
path: the shape table of tests/test_exact_parity.py (exact_problems.SHAPES) under every option of its configurations a PGDUpdate
handle takes.

On the near-fit integer problems of exact_problems.make_pgd_problem the residual est - data is a small signed integer, gradW =
hxt(H, resid) and gradH = transconv(W, resid) are signed integer sums whose every partial sum is bounded by the sum of absolute values
(below 2^24: exact in fp32 in any order), g = gscale G + 2 pen x + pen_abs sign(x) is a multiple of 1/2, and pgd_w_grad_kernel /
pgd_h_grad_kernel sum g^2 in DOUBLE: an exact number below 2^53 in any order, across blocks and across shards (group_sum_doubles).  So
alpha = (float)(step / (sqrt(sum g^2) + eps)) is one float32 number on every path, and x - alpha g, fused or not, is within 2 ulp of the
oracle's fp64 step (exact_problems' PGD section; tests/test_exact_problems.py confirms it with a float32 model on every row).  Hence:

  * the updated factor is within 2 ulp of oracle.pgd_update_motifs / pgd_update_feature_maps on a fresh oracle.PGDUpdate, per element;
  * it is BIT-IDENTICAL across all configurations of a row, groups included;
  * rule.steps equals the oracle's (stepW, stepH) exactly; compute_loss() on the integer factors equals the oracle exactly.

One unit of one contraction moves an element by at least 200 ulp (profiles/exact_masked_pgd.txt; at least 8 asserted), so a lost term, a
mask tile read one block off or a weight read as a flag fails here, where the norm-wise 1e-4 of tests/test_gpu_parity.py passes them.

Not covered, and why: the HALS sweeps have a file of their own (tests/test_gpu_exact_hals.py; their CONV_RESID conv is the one reached here);
UnitNormConstraint (its per-component norms are not exact); several PGD iterations from non-integer factors (tests/test_gpu_parity.py,
norm-wise)."""
import os
import time

import numpy as np
import pytest

import exact_problems as ep
from exact_problems import LAUNCH_PATHS, PGD_VARIANTS, SHAPES, first_bad
from test_exact_parity import ULP_BAR, check_same, reached

pytestmark = pytest.mark.gpu

_seen = {}
_worst = {"W": 0.0, "H": 0.0}
_done = set()
IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES]


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def pgd_configs(configs):
    """The configurations of a table row as a PGDUpdate handle takes them.  "gram" and "reuse_est" belong to the MU entries: the PGD
    entries of a single handle never read them (pgd_w_phase / pgd_h_phase, cmf_rules.hip: est is reused by its kind alone) and a group
    refuses the rule under gram (group_pgd_prepare) -- test_options_the_pgd_entries_ignore_or_refuse; they are left out."""
    out = []
    for c in configs:
        c = {k: v for k, v in c.items() if k not in ("gram", "reuse_est")}
        if c not in out:
            out.append(c)
    return out


def counters(rule):
    return {p: rule.counter("launches:" + p) for p in LAUNCH_PATHS}


def record(c):
    for p, v in c.items():
        _seen[p] = _seen.get(p, 0) + v


def make_rule(cmf, cfg, X, W, H):
    cfg = dict(cfg)
    devices = cfg.pop("devices", None)
    rule = cmf.PGDUpdate(X, W, H, devices=devices) if devices else cmf.PGDUpdate(X, W, H)
    try:
        for name, value in cfg.items():
            rule.set_option(name, value)
    except Exception:
        rule.close()
        raise
    return rule


def fresh(cmf, rule, W, H):
    """The state of a new handle again: the factors, stepW = stepH = 5, no cur_loss, est void (test_reset_handle_is_a_fresh_handle)."""
    rule.upload(W, H)
    cmf.host.check(rule._lib.cmf_pgd_reset(rule._h))


class Variant:
    """The arguments of a PGDUpdate call for a variant of exact_problems.PGD_VARIANTS (one MaskedLoss object per problem: the handle
    uploads the mask when the object changes)."""

    def __init__(self, cmf, name, mask):
        loss, masked, penW, penH, nonneg = PGD_VARIANTS[name]
        base = cmf.AbsoluteLoss() if loss == "abs" else cmf.SquareLoss()
        self.loss_func = cmf.MaskedLoss(base, mask) if masked else base
        self.penW = [cmf.SquarePenalty(w) for w in penW[0]] + [cmf.AbsolutePenalty(w) for w in penW[1]]
        self.penH = [cmf.SquarePenalty(w) for w in penH[0]] + [cmf.AbsolutePenalty(w) for w in penH[1]]
        self.constr = cmf.NonnegConstraint if nonneg else None

    def w_half(self, rule):
        rule.update_motifs(loss_func=self.loss_func, constrW=self.constr, penaltiesW=self.penW)

    def h_half(self, rule):
        return rule.update_feature_maps(loss_func=self.loss_func, constrH=self.constr, penaltiesH=self.penH)


def check_factor(got, ref, names, what, cfg, c):
    u = ep.ulps(got, ref)
    if not np.isfinite(got).all() or u.max() > ULP_BAR:
        i = tuple(np.argwhere(~(u <= ULP_BAR))[0])
        raise AssertionError(f"{what} {cfg}: {np.nanmax(u):.1f} ulp from the fp64 oracle at {first_bad(~(u <= ULP_BAR), names)} "
                             f"(got {got[i]!r}, want {ref[i]!r}; {int((~(u <= ULP_BAR)).sum())} elements over the bar); launches {reached(c)}")
    return float(u.max())


def references(oracle, shape, family, check):
    """(W, H, X, mask, est loss of the integer factors, {variant: (factor, steps, loss)}) by the oracle; check: the preconditions from
    the arrays generated (the rows with N >= 1000 leave them to tests/test_exact_problems.py, which asserts them on the whole table)."""
    W, H, X, mask = ep.make_pgd_problem(*shape, family)
    assert ep.max_tile_sum((ep._conv(W, H) - X) ** 2) <= ep.EXACT
    refs = {}
    for variant in ep.pgd_variants(shape[0]):
        if check:
            ep.assert_pgd_preconditions(ep.pgd_half(variant, family, W, H, X, mask), X, mask, f"{shape} {family} {variant}")
        refs[variant] = ep.pgd_oracle_half(oracle, variant, family, W, H, X, mask)
    return W, H, X, mask, oracle.compute_loss(X, W, H), refs


def run_pgd_config(cmf, cfg, ref_w, ref_h, variants_w, variants_h, record=record, worst=_worst):
    """One configuration of a row against references(..., "W") and references(..., "H"): {(family, variant): updated factor}, launch
    counters; everything test_exact_pgd_paths asserts per configuration asserted."""
    Ww, Hw, Xw, mask_w, loss_w_ref, refs_w = ref_w
    Wh, Hh, Xh, mask_h, loss_h_ref, refs_h = ref_h
    got = {}
    rule = make_rule(cmf, cfg, Xw, Ww, Hw)
    try:
        lw = rule.compute_loss()
        for v, var in variants_w.items():
            fresh(cmf, rule, Ww, Hw)
            var.w_half(rule)
            got[("W", v)] = (rule.download()[0], rule.steps, None)
        c = counters(rule)
    finally:
        rule.close()
    rule = make_rule(cmf, cfg, Xh, Wh, Hh)
    try:
        lh = rule.compute_loss()
        for v, var in variants_h.items():
            fresh(cmf, rule, Wh, Hh)
            loss = var.h_half(rule)  # (est is void: the transposing conv CONV_RESID_T / CONV_MASKED_RESID_T)
            got[("H", v)] = (rule.download()[1], rule.steps, loss)
        ch = counters(rule)
    finally:
        rule.close()
    c = {p: c[p] + ch[p] for p in c}
    record(c)
    assert (lw, lh) == (loss_w_ref, loss_h_ref), f"loss {cfg}: {(lw, lh)} != {(loss_w_ref, loss_h_ref)}; launches {reached(c)}"
    for (family, v), (x, steps, loss) in got.items():
        ref, steps_ref, loss_ref = (refs_w if family == "W" else refs_h)[v]
        names = "knl" if family == "W" else "kt"
        what = f"{family} half, {v}"
        worst[family] = max(worst[family], check_factor(x, ref, names, what, cfg, c))
        assert steps == steps_ref, f"{what} {cfg}: steps {steps}, the oracle's {steps_ref}; launches {reached(c)}"
        if family == "H":
            np.testing.assert_allclose(loss, loss_ref, rtol=1e-5)  # (H is no longer integer: the bar of tests/test_exact_parity.py)
    return {key: x for key, (x, _, _) in got.items()}, c


@pytest.mark.parametrize("N,T,K,L,configs,why", SHAPES, ids=IDS)
def test_exact_pgd_paths(cmf, oracle, N, T, K, L, configs, why):
    shape = (N, T, K, L)
    t0 = time.perf_counter()
    ref_w = references(oracle, shape, "W", N < 1000)
    ref_h = references(oracle, shape, "H", N < 1000)
    variants_w = {v: Variant(cmf, v, ref_w[3]) for v in ref_w[5]}
    variants_h = {v: Variant(cmf, v, ref_h[3]) for v in ref_h[5]}
    t_ref = time.perf_counter() - t0
    base = {}
    for cfg in pgd_configs(configs):
        if T // len(cfg.get("devices", [0])) < 2 * L:
            continue  # (shards shorter than two lag windows: not a shape a group takes)
        got, c = run_pgd_config(cmf, cfg, ref_w, ref_h, variants_w, variants_h)
        for (family, v), x in got.items():
            names = "knl" if family == "W" else "kt"
            if (family, v) not in base:
                base[(family, v)] = (cfg, x)
            else:
                check_same(x, base[(family, v)][1], names, f"{family} half, {v}", cfg, base[(family, v)][0], c)
    _done.add(shape)
    print(f"{shape} {why}: oracle {t_ref:.2f} s, total {time.perf_counter() - t0:.2f} s; worst so far W {_worst['W']:.2f} ulp, H {_worst['H']:.2f} ulp")


# No entry leaves est at the residual WITHOUT changing the factors: est_kind becomes a residual kind in resid_and_loss alone, which
# only the closing step of a half (pgd_finish, the HALS phases) calls, after the factor has moved; cmf_compute_loss is the MU entry and
# leaves the MU kind.  So the transpose_rows_kernel route of pgd_h_phase always starts from a non-integer factor and has no exact
# reference.  It is held to the other route instead: after a W half the resident residual is the CONV_RESID / CONV_MASKED_RESID store
# of (W', H); uploading the very same factors again voids est and sends the H half through CONV_RESID_T / CONV_MASKED_RESID_T.  Both
# convs form each entry from the same products in the same order (the transposing modes swap the two MFMA operands, cmf_kernels.h), the
# epilogues apply the same subtraction, sign and mask, and transpose_rows_kernel moves bits: the two H halves must give the same bits.
TRANSPOSE_ROWS = [s for s in SHAPES if s[:4] in {(130, 700, 32, 20), (70, 600, 20, 10), (250, 1500, 5, 20), (1000, 4100, 8, 10), (2000, 6250, 32, 20)}]


@pytest.mark.parametrize("N,T,K,L,configs,why", TRANSPOSE_ROWS, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in TRANSPOSE_ROWS])
def test_h_half_on_the_resident_residual(cmf, N, T, K, L, configs, why):
    W, H, X, mask = ep.make_pgd_problem(N, T, K, L, "W")
    for cfg in [{}] + [c for c in pgd_configs(configs) if "devices" in c][:1]:
        for v in ("square", "abs_masked"):
            var = Variant(cmf, v, mask)
            rule = make_rule(cmf, cfg, X, W, H)
            try:
                var.w_half(rule)
                W1, _ = rule.download()
                loss_a = var.h_half(rule)  # the residual is resident: transpose_rows_kernel
                _, Ha = rule.download()
                steps_a = rule.steps
                c = counters(rule)
            finally:
                rule.close()
            rule = make_rule(cmf, cfg, X, W, H)
            try:
                var.w_half(rule)
                rule.upload(W1, H)  # the same factors, est void: the transposing conv
                loss_b = var.h_half(rule)
                _, Hb = rule.download()
                steps_b = rule.steps
            finally:
                rule.close()
            record(c)
            check_same(Ha, Hb, "kt", f"H half on the resident residual, {v}", cfg, "the H half through the transposing conv", c)
            assert (loss_a, steps_a) == (loss_b, steps_b), (v, cfg, loss_a, loss_b, steps_a, steps_b)


def test_reset_handle_is_a_fresh_handle(cmf):
    """What test_exact_pgd_paths relies on between variants: upload + cmf_pgd_reset give the bits and the steps of a new handle."""
    N, T, K, L = 130, 700, 32, 20
    for family in ("W", "H"):
        W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
        used = make_rule(cmf, {}, X, W, H)
        try:
            Variant(cmf, "square_l1", mask).w_half(used)
            Variant(cmf, "square_l1", mask).h_half(used)
            for v in ("abs_masked", "square"):
                var = Variant(cmf, v, mask)
                fresh(cmf, used, W, H)
                loss_u = var.w_half(used) if family == "W" else var.h_half(used)
                new = make_rule(cmf, {}, X, W, H)
                try:
                    loss_n = var.w_half(new) if family == "W" else var.h_half(new)
                    assert used.steps == new.steps and loss_u == loss_n
                    for a, b in zip(used.download(), new.download()):
                        np.testing.assert_array_equal(a, b)
                finally:
                    new.close()
        finally:
            used.close()


def test_options_the_pgd_entries_ignore_or_refuse(cmf):
    """gram and reuse_est: the same bits on a single handle (the PGD entries never read them), CMF_ERR_STATE on a group under gram."""
    N, T, K, L = 130, 700, 32, 20
    W, H, X, mask = ep.make_pgd_problem(N, T, K, L, "W")
    var = Variant(cmf, "abs_masked", mask)
    out = []
    for cfg in (dict(), dict(gram=1), dict(gram=2), dict(reuse_est=0)):
        rule = make_rule(cmf, cfg, X, W, H)
        try:
            var.w_half(rule)
            var.h_half(rule)
            out.append(rule.download() + (rule.steps,))
        finally:
            rule.close()
    for o in out[1:]:
        np.testing.assert_array_equal(o[0], out[0][0])
        np.testing.assert_array_equal(o[1], out[0][1])
        assert o[2] == out[0][2]
    group = make_rule(cmf, dict(devices=[0, 0], gram=1), X, W, H)
    try:
        for call in (lambda: var.w_half(group), lambda: var.h_half(group)):
            with pytest.raises(cmf.CMFError, match="gram") as ei:
                call()
            assert ei.value.code == 3
    finally:
        group.close()


@pytest.mark.parametrize("N,T,K,L", [(130, 700, 32, 20), (130, 700, 5, 20), (70, 600, 20, 10)])
def test_exact_pgd_long_recordings(cmf, oracle, N, T, K, L):
    """A recording longer than a handle holds (CMF_MAX_COLUMNS under CMF_TEST_HOOKS=1: sharded automatically on one device) gives the
    unsharded handle's bits, and so the oracle's within 2 ulp."""
    shape = (N, T, K, L)
    for family, names in (("W", "knl"), ("H", "kt")):
        W, H, X, mask, _, refs = references(oracle, shape, family, True)
        for v in ("square", "abs_masked", "square_l1"):
            var = Variant(cmf, v, mask)
            got = []
            for sharded in (False, True):
                if sharded:
                    os.environ["CMF_TEST_HOOKS"] = "1"
                    os.environ["CMF_MAX_COLUMNS"] = "300"
                try:
                    rule = cmf.PGDUpdate(X, W, H)
                    try:
                        loss = var.w_half(rule) if family == "W" else var.h_half(rule)
                        got.append((rule.download()[0 if family == "W" else 1], rule.steps, loss))
                        c = counters(rule)
                        record(c)
                    finally:
                        rule.close()
                finally:
                    os.environ.pop("CMF_MAX_COLUMNS", None)
                    os.environ.pop("CMF_TEST_HOOKS", None)
            assert c["halo_pack2_kernel"] + c["halo_pack3_kernel"] > 0, "the recording was not sharded"
            check_factor(got[0][0], refs[v][0], names, f"{family} half, {v}", {}, c)
            check_same(got[1][0], got[0][0], names, f"{family} half, {v}", {"CMF_MAX_COLUMNS": 300}, "the unsharded handle", c)
            assert got[1][1] == got[0][1] == refs[v][1], (family, v, got[1][1], got[0][1], refs[v][1])
            if family == "H":  # (the loss after the update sums non-integer terms shard by shard: the bar of tests/test_exact_parity.py)
                np.testing.assert_allclose([got[0][2], got[1][2]], refs[v][2], rtol=1e-5)
    _done.add(("long", shape))


@pytest.mark.parametrize("N,T,K,L", [(48, 300, 4, 8), (37, 150, 33, 7)])
def test_lone_handle_is_a_group_of_one_shard(cmf, N, T, K, L):
    """A lone PGDUpdate and PGDUpdate(devices=[0]) run the same per-shard code (pgd_w_phase / pgd_h_phase, cmf_rules.hip); between the
    shards a one-rank all-reduce sums one buffer and group_sum_doubles one double.  From the same non-integer data and factors they give
    W, H, steps and every loss bit for bit equal over three iterations."""
    data = cmf.gen_synthetic(N=N, T=T, K=3, L=L, seed=1234 + N)
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=T)
    masked = cmf.MaskedLoss(cmf.SquareLoss(), cmf.holdout_mask(N, T, frac=0.2, block=L, seed=K))
    for loss_func, constr in ((cmf.SquareLoss(), cmf.NonnegConstraint), (cmf.AbsoluteLoss(), cmf.UnitNormConstraint), (masked, None)):
        got = []
        for devices in (None, [0]):
            rule = cmf.PGDUpdate(data, W0, H0, devices=devices)
            try:
                trace = []
                for _ in range(3):
                    rule.update_motifs(loss_func=loss_func, constrW=constr)
                    trace.append(rule.steps)
                    trace.append((rule.update_feature_maps(loss_func=loss_func, constrH=constr), rule.steps))
                got.append(rule.download() + (trace,))
            finally:
                rule.close()
        what = f"{type(loss_func).__name__}, {getattr(constr, '__name__', None)}"
        check_same(got[1][0], got[0][0], "knl", f"W after three iterations, {what}", {"devices": [0]}, "the lone handle", {})
        check_same(got[1][1], got[0][1], "kt", f"H after three iterations, {what}", {"devices": [0]}, "the lone handle", {})
        assert got[1][2] == got[0][2], f"{what}: steps and losses {got[1][2]} on the group, {got[0][2]} on the lone handle"


# The paths the PGD entries cannot reach, from pgd_w_phase / pgd_h_phase (cmf_rules.hip: one statement for a lone handle and a group) and launch_conv
# (cmf_internal.h) -- one reason each.  Everything else of LAUNCH_PATHS must be reached by this file.  (conv_small_kernel:pre, the
# preloaded data tile of the MU loss + store modes, is no PGD path either -- conv_has_pre -- but compute_loss(), the MU entry these
# handles call for the loss of the integer factors, launches it: it is neither asked for nor forbidden.)
BY_COMPUTE_LOSS = {"conv_small_kernel:pre"}
NOT_FOR_PGD = {
    "conv2_kernel": "the 128 x 128 tiles do not exist for the residual modes (conv_on_tiles128): option conv_kernel = 2 falls to the one-wave kernel",
    "hxt_kernel:nsrc2": "the gradient contracts ONE source, the residual (hxt_contract(h, est, est, 1, ...))",
    "g_gemm_fold_small_kernel:fused_h": "the H update inside the C3 launch is an MU fusion (launch_transconv never passes update_h)",
    "slab_sum_kernel:carry": "a deferred loss reduction rides on the slab sum in cmf_iterate alone, which runs the MU rule",
    "slab_sum_small_kernel:carry": "cmf_iterate alone",
    "transconv_kernel:front_block": "a shard that updates the columns in front of its own (h_update_impl front = true): the MU groups only",
    "gram_w_kernel": "the Gram forms rewrite the MU denominators; the PGD entries never read option gram",
    "gram_lag_corr": "the Gram forms are MU only",
    "gram_w_taps": "the Gram forms are MU only",
    "gram_h_mfma_kernel": "the Gram forms are MU only",
    "gram_h_kernel": "the Gram forms are MU only",
}


def test_every_launch_path_pgd_can_reach_is_reached():
    """The union of launches:* over this file is exactly LAUNCH_PATHS minus NOT_FOR_PGD.  Also prints the worst element-wise error
    observed per family (the `gpu` lines of profiles/exact_masked_pgd.txt)."""
    print(f"gpu pgd W {_worst['W']:.3g}\ngpu pgd H {_worst['H']:.3g}")
    print({p: _seen.get(p, 0) for p in LAUNCH_PATHS})
    if len(_done) < len(SHAPES) + 3:
        pytest.skip("runs after the whole table (the file as a whole)")
    missing = [p for p in LAUNCH_PATHS if p not in NOT_FOR_PGD and p not in BY_COMPUTE_LOSS and not _seen.get(p)]
    extra = [p for p in NOT_FOR_PGD if _seen.get(p)]
    assert not missing, f"launch paths the PGD rule can reach and no shape did: {missing}"
    assert not extra, f"reached paths the test says the PGD rule cannot: {extra}"
