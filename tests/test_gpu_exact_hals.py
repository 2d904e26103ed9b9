"""The HALS sweeps against the fp64 restatement ELEMENT BY ELEMENT on every kernel path: the ten register instances of the W sweep and
its general form, the persistent H pipeline with one to four pullers per row, the same with the residual conv chasing it, the stage
pipeline at both lags, the general row sweep, the four ways hals_hh_kernel forms an entry and the three forms of the projections
(option hals_gram) -- the table exact_problems.HALS_SHAPES, chosen by the plan rules restated in exact_problems.hals_plan and confirmed
here by the launch counters "launches:<name>" of the HALS entries (cmf_internal.h kHalsLaunchNames).

On the integer problems of exact_problems every contraction in front of a sweep is an exact integer in fp32 (G, HH, the lag correlations,
P, the lag Grams and their taps; tests/test_exact_problems.py proves it from the arrays), so the projections reach the sweeps
bit-identical on every path and the only rounding left is inside the sequential recurrences.  Hence, per row, sweep configuration,
regulariser pair ((0, 0) and (0.5, 0.25)) and half -- update_motifs on the "W" family, update_feature_maps on a fresh upload of the "H"
family:

  * every element of the updated factor is within the bar of hals_gram_form.w_half / h_half in fp64, in units of the fp32 spacing at
    scale = max(|value before the clamp|, |old value|).  The bar is 4 times the worst error of the float32 MODEL of the restatement over
    the table, at least 8 (profiles/exact_hals.txt; never a GPU result);
  * the zero pattern is the reference's, apart from the few elements that decide their clamp within the bar (counted in the profile);
  * the loss after the H half is within its bar (made the same way from a float32 conv);
  * under hals_gram = 2, 0 and 1 the results are equal BIT FOR BIT, and so is a second run of the same configuration;
  * every handle reaches exactly the launch names its plan expects and reports no hals_pipeline_reruns (a persistent sweep whose wait
    ran out is silently redone on the stage pipeline: its result would pass, its path would not have been tested).

One lost cross-row term, one same-row push, one stale HH row, one truncated window taken at full length or a regulariser left out
moves an element by at least 4 bars (the mutation tests of tests/test_exact_problems.py), where the Frobenius bars of
tests/test_gpu_parity.py admit them."""
import time

import numpy as np
import pytest

import exact_problems as ep
from exact_problems import HALS_LAUNCH_PATHS, HALS_REGS, HALS_SHAPES

pytestmark = pytest.mark.gpu

BAR_W, BAR_H, BAR_LOSS = ep.hals_bars()
GRAMS = (2, 0, 1)
IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in HALS_SHAPES]
_seen = {}
_worst = {}
_worst_loss = [0.0]
_done = set()
_attempted = set()


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def counters(rule):
    return {p: rule.counter("launches:" + p) for p in HALS_LAUNCH_PATHS}


def reached(c):
    return sorted(p for p, v in c.items() if v)


def record(c, seen=None):
    seen = _seen if seen is None else seen
    for p, v in c.items():
        seen[p] = seen.get(p, 0) + v


def make_rule(cmf, cfg, X, W, H):
    rule = cmf.HALSUpdate(X, W, H)
    try:
        for name, value in cfg.items():
            rule.set_option(name, value)
    except Exception:
        rule.close()
        raise
    return rule


def pipelines(plan):
    """(name of the W sweep, name of the H sweep) a plan of exact_problems.hals_plan runs: the keys of the `gpu` lines."""
    w = "general" if plan["w_general"] else "register"
    h = "general" if plan["h_general"] else "stage" if plan["P"] == 0 else "chased" if plan["chase"] else "persistent"
    return w, h


def expected_launches(plan, gram, K, lag):
    """The HALS launch names a handle that runs W halves only, and one that runs H halves only, reach under a plan, by the plan
    mirror: exactly these and no other (a persistent sweep redone on the stage pipeline, another puller count, a chase that was not
    planned all show as a name that is not expected)."""
    w = {"hals_w_sweep_gen_kernel"} if plan["w_general"] else {f"hals_w_sweep_reg_kernel<{plan['NQ']}>"}
    w.add("hals_g:difference" if gram == 1 else "hals_g:residual")
    h = {"hals_p_init_kernel:den" if gram and plan["gram_window"] else "hals_p_init_kernel:residual"}
    if plan["h_general"]:
        h |= {"hals_h_row_gen_kernel"} | ({"hals_h_push_gen_kernel"} if K > 1 else set())
    elif plan["P"] == 0:
        h |= {"hals_h_stage_kernel", f"hals_h_stage_kernel:lag{lag}"}
    else:
        h |= {"hals_h_persist_kernel", f"hals_h_persist_kernel:P{plan['P']}", "hals_p_init_kernel:snapshot"}
        if plan["chase"]:
            h |= {"hals_h_persist_kernel:chased", "conv3_chase_kernel"} | ({"conv3_chase_kernel:rest"} if plan["chase"] < plan["nblk"] else set())
    return w, h


def same_bits(got, ref, names, what, launches):
    if not np.array_equal(got, ref):
        bad = got != ref
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at {ep.first_bad(bad, names)}: {got[i]!r} != {ref[i]!r}; launches {launches}")


def references(shape):
    """{family: (W, H, X, [fp64 half per regulariser pair])}, once per row."""
    out = {}
    for family in ("W", "H"):
        W, H, X = ep.make_hals_problem(*shape, family)
        out[family] = (W, H, X, [ep.hals_half(family, W, H, X, reg) for reg in HALS_REGS])
    return out


def run_half(rule, family, W, H, reg):
    """(updated factor, loss or None) of one half from a fresh upload of (W, H)."""
    rule.upload(W, H)
    if family == "W":
        rule.update_motifs(l1W=reg[0], l2W=reg[1])
        return rule.download()[0], None
    loss = rule.update_feature_maps(l1H=reg[0], l2H=reg[1])
    return rule.download()[1], loss


def run_hals_row(cmf, shape, configs, refs, n_cu=ep.N_CU, seen=None, worst=None, worst_loss=None):
    """Every sweep configuration of a row under hals_gram = 2, 0 and 1 against the references refs (references(shape)): the list of
    element-wise, zero-pattern and loss failures; the launch names, the reruns and the bit-identities are asserted on the spot.
    n_cu: the CU count the handles are planned for (the plan mirror's);
    seen, worst, worst_loss: where the counters and the worst errors are kept (default: this file's)."""
    N, T, K, L = shape
    seen, worst, worst_loss = _seen if seen is None else seen, _worst if worst is None else worst, _worst_loss if worst_loss is None else worst_loss
    failures = []
    for cfg in configs:
        base, base_loss = {}, {}
        for gram in GRAMS:
            opts = dict(cfg, hals_gram=gram)
            plan = ep.hals_plan(N, T, K, L, opts, n_cu=n_cu)
            want_w, want_h = expected_launches(plan, gram, K, 3 if opts.get("hals_lag") == 3 else 2)
            for family, names, bar, want in (("W", "knl", BAR_W, want_w), ("H", "kt", BAR_H, want_h)):
                W, H, X, halves = refs[family]
                pipe = pipelines(plan)[0 if family == "W" else 1]
                rule = make_rule(cmf, opts, X, W, H)
                try:
                    for r, reg in enumerate(HALS_REGS):
                        got, loss = run_half(rule, family, W, H, reg)
                        again, loss2 = run_half(rule, family, W, H, reg)
                        c = counters(rule)
                        what = f"{family} half {shape} {opts} reg {reg}"
                        if r == 0:
                            record(c, seen)  # (the names do not depend on the regularisers: counted before anything can fail)
                        assert set(reached(c)) == want, (f"{what}: the plan mirror expects exactly {sorted(want)}; missing {sorted(want - set(reached(c)))}, "
                                                         f"not expected {sorted(set(reached(c)) - want)}")
                        assert rule.counter("hals_pipeline_reruns") == 0, f"{what}: a wait of the persistent pipeline ran out and the sweep was redone on the stage pipeline"
                        a = halves[r]
                        u, msg = ep.check_hals(got, a, bar, names, reached(c))
                        key = (family, pipe)
                        worst[key] = max(worst.get(key, 0.0), u if np.isfinite(u) else 1e30)
                        print(f"{what}: worst {u:.2f} units (bar {bar:g})" + (f", loss {loss!r} want {a['loss']!r}" if family == "H" else ""))
                        if msg:
                            failures.append(f"{what}: {msg}")
                        if family == "H":
                            rel = abs(loss - a["loss"]) / a["loss"]
                            worst_loss[0] = max(worst_loss[0], rel)
                            if not rel <= BAR_LOSS:
                                failures.append(f"{what}: loss {loss!r}, want {a['loss']!r}: {rel:.2e} relative (bar {BAR_LOSS:.2e}); launches {reached(c)}")
                        same_bits(again, got, names, f"{what}: the second run against the first", reached(c))
                        assert loss2 == loss, f"{what}: the second run's loss {loss2!r} != {loss!r}"
                        if (family, r) not in base:
                            base[(family, r)] = (gram, got)
                        else:
                            g0, ref = base[(family, r)]
                            same_bits(got, ref, names, f"{what}: against hals_gram = {g0}", reached(c))
                        if family == "H":  # (the loss: the same tiles in the same order wherever the same launches form it)
                            g0, loss0 = base_loss.setdefault((r, pipe), (gram, loss))
                            assert loss == loss0, f"{what}: loss {loss!r}, under hals_gram = {g0} on the same pipeline {loss0!r}"
                finally:
                    rule.close()
    return failures


@pytest.mark.parametrize("N,T,K,L,configs,why", HALS_SHAPES, ids=IDS)
def test_exact_hals_paths(cmf, N, T, K, L, configs, why):
    shape = (N, T, K, L)
    _attempted.add(shape)
    t0 = time.perf_counter()
    refs = references(shape)
    t_ref = time.perf_counter() - t0
    failures = run_hals_row(cmf, shape, configs, refs)
    assert not failures, "\n".join(failures)
    _done.add(shape)
    print(f"{shape} {why}: reference {t_ref:.2f} s, total {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("N,T,K,L", [(37, 700, 32, 20), (37, 150, 5, 4)])
def test_speculated_projection_is_the_contracted_one(cmf, N, T, K, L):
    """update_feature_maps! enqueues G and HH of the next update_motifs! behind its loss (hals_w_speculate).  The factors are no longer
    integers there, so there is no exact reference: the speculated W half is held to the same W half on the same factors uploaded again
    (which voids the speculation) -- the same contractions of the same operands, launched earlier: bit for bit."""
    _attempted.add(("speculated", N, T, K, L))
    W, H, X = ep.make_hals_problem(N, T, K, L, "W")
    l1, l2 = HALS_REGS[1]
    out = []
    for void in (False, True):
        rule = make_rule(cmf, {}, X, W, H)
        try:
            rule.update_motifs(l1W=l1, l2W=l2)
            rule.update_feature_maps(l1H=l1, l2H=l2)
            if void:
                rule.upload(*rule.download())
            rule.update_motifs(l1W=l1, l2W=l2)
            out.append(rule.download()[0])
            c = counters(rule)
            record(c)
            assert c["hals_w_speculate"] == 1 and c["hals_g:speculated"] == (0 if void else 1) and c["hals_g:residual"] == (2 if void else 1), reached(c)
            assert rule.counter("speculated_contractions") == (0 if void else 1)
        finally:
            rule.close()
    same_bits(out[0], out[1], "knl", "the speculated W half against the contracted one", reached(c))
    _done.add(("speculated", N, T, K, L))


def test_every_hals_launch_path_is_reached():
    """The union of launches:* over this file is all of HALS_LAUNCH_PATHS.  Also prints the worst element-wise error observed per half
    and pipeline and the worst relative error of the loss (the `gpu` lines of profiles/exact_hals.txt)."""
    for (family, pipe), u in sorted(_worst.items()):
        print(f"gpu {family}:{pipe} {u:.4g}")
    print(f"gpu loss {_worst_loss[0]:.4g}")
    print({p: _seen.get(p, 0) for p in HALS_LAUNCH_PATHS})
    if len(_attempted) < len(HALS_SHAPES) + 2:
        pytest.skip("runs after the whole table (the file as a whole)")
    assert len(_done) == len(_attempted), f"{len(_attempted) - len(_done)} tests of the table failed: the coverage below is of what ran before they did"
    missing = [p for p in HALS_LAUNCH_PATHS if not _seen.get(p)]
    assert not missing, f"HALS launch paths no row reached: {missing}"
    assert all(u <= (BAR_W if family == "W" else BAR_H) for (family, _), u in _worst.items())
