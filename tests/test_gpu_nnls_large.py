"""The NNLS solver for 129 .. 1024 unknowns (option "nnls_large": nnls_large_kernel behind cmf_anls_update_motifs and
cmf_sep_nnls) against the fp64 restatements tests/anls_restatement.py and tests/sep_restatement.py.

Bars: the project's fp64 rule, unchanged (test_gpu_anls.py, test_gpu_sep.py).  A single call must land within
anls_restatement.bar(floor, 1e-8) of the restatement -- 1000 x the literal-vs-Gram difference of the same call, at least one
ulp, never looser than 1e-8 -- and a fit within bar(floor, 1e-6); zero patterns are identical off the entries the restatement
itself calls near-degenerate, of which a shape has at most 1 %; no problem is capped.  Every shape is first checked on the CPU
(check_step / check_problem: both modes agree to 1e-10 with equal patterns, tol and tol = 1e-12 end on the same passive sets).
Every test prints the measured distance beside its bar, and the GPU's pivoting rounds beside the restatement's.
"""
import functools

import numpy as np
import pytest

import anls_restatement as R
import sep_restatement as S

pytestmark = pytest.mark.gpu

# name: (N, T, K, L) -- R.problem(..., seed=0), update_motifs only.  songbird.jl:11-18 has K, L = 3, 50; speech.jl:40-48 has 20, 12;
# kl640 has the K, L of the project's headline shape.
SHAPES = {
    "kl129": (16, 1400, 3, 43),
    "song_kl150": (24, 1600, 3, 50),
    "speech_kl240": (32, 2400, 20, 12),
    "kl320": (24, 3000, 16, 20),
    "kl640": (12, 5000, 32, 20),
}
SEP_CASES = {"r160": (200, 1500, 5, 32, 0.1, None, 1), "r150": (200, 1500, 3, 50, 0.1, None, 1)}
FIT_SEED, FIT_ITERS = 2, 4


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build(quiet=True)
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def same(name, X, Xr, near, tol):
    """X (GPU) against Xr (restatement): norm-wise within tol, the zero pattern identical off the near-degenerate entries."""
    d = R.rel(X, Xr)
    mism = ((X > 0) != (Xr > 0)) & ~near
    print(f"{name}: rel {d:.3e} (bar {tol:.3e}), pattern mismatches {int(mism.sum())}, near-degenerate {int(near.sum())} of {X.size}")
    assert (X >= 0).all(), name
    assert d <= tol, (name, d, tol)
    assert not mism.any(), (name, np.argwhere(mism)[:5].tolist())


def close(name, X, Xr, floor):
    d, tol = R.rel(X, Xr), R.bar(floor, 1e-8)
    print(f"{name}: rel {d:.3e} (bar {tol:.3e}, floor {floor:.3e})")
    assert np.isfinite(X).all() and d <= tol, (name, d, tol)


def large_rule(cmf, data, W0, H0, backup_only=0):
    rule = cmf.ANLSUpdate(data, W0, H0)
    try:
        rule.set_option("nnls_large", 1)
        if backup_only:
            rule.set_option("anls_backup_only", 1)
    except BaseException:
        rule.close()
        raise
    return rule


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's W, its near-degenerate mask, floor and pivoting rounds for one shape (CPU; shared by the solver modes)."""
    N, T, K, L = SHAPES[name]
    data, W0, H0 = R.problem(N, T, K, L, seed=0)
    sl, sg = {}, {}
    Wl = R.update_motifs(data, H0, L, mode="literal", stats=sl)
    W = R.update_motifs(data, H0, L, stats=sg)
    floor = R.check_step(name + " W", Wl, W, sl, sg, R.update_motifs(data, H0, L, tol=1e-12), R.bar(R.rel(Wl, W), 1e-8))
    return data, W0, H0, W, sg["near"], floor, sg["exchanges"]


def run_w(cmf, name, backup_only):
    data, W0, H0, Wr, near, floor, exchanges = reference(name)
    rule = large_rule(cmf, data, W0, H0, backup_only)
    try:
        W = W0.copy(order="F")
        rule.update_motifs(data, W, H0)
        print(f"{name} backup_only={backup_only}: pivoting rounds {rule.last_W_exchanges} (restatement, default mode: {exchanges})")
        same(f"{name} W", W, Wr, near, R.bar(floor, 1e-8))
        assert rule.counter("anls_capped") == 0 and rule.last_W_exchanges > 0
        if backup_only:
            assert rule.counter("anls_backup") > 0
        return W
    finally:
        rule.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_single_w_calls_match_the_restatement(cmf, name):
    run_w(cmf, name, 0)


@pytest.mark.parametrize("name", ["kl129", "song_kl150", "speech_kl240"])
def test_single_w_calls_under_backup_only(cmf, name):
    """Plain principal pivoting ends on the same W (the two largest shapes are left out: hundreds of factorisations per problem)."""
    run_w(cmf, name, 1)


def test_two_runs_are_bit_identical(cmf):
    assert np.array_equal(run_w(cmf, "kl320", 0), run_w(cmf, "kl320", 0))


def restated_fit(data, W0, H0, L, iters, variant):
    """make_golden_anls.fit: the literal and the Gram fit side by side, every half step through check_step."""
    Wl, Hl, W, H = W0, H0, W0, H0
    hist = [np.linalg.norm(R.conv(W, H) - data) / np.linalg.norm(data)]
    floor = 0.0
    for it in range(iters):
        sl, sg = {}, {}
        W12 = R.update_motifs(data, H, L, tol=1e-12)
        Wl, W = R.update_motifs(data, Hl, L, mode="literal", stats=sl), R.update_motifs(data, H, L, stats=sg)
        R.check_step(f"{variant} it {it} W", Wl, W, sl, sg, W12, 1e-8)
        nearW = sg["near"]
        H12, _ = R.update_feature_maps(data, W, H, variant=variant, tol=1e-12)
        (Hl, _), (H, loss) = (R.update_feature_maps(data, Wl, Hl, variant=variant, mode="literal", stats=sl),
                              R.update_feature_maps(data, W, H, variant=variant, stats=sg))
        R.check_step(f"{variant} it {it} H", Hl, H, sl, sg, H12, 1e-8)
        nearH = sg["near"]
        floor = max(floor, R.rel(Wl, W), R.rel(Hl, H))
        hist.append(loss)
    return W, H, np.array(hist), nearW, nearH, floor


def test_a_fit_past_the_bound(cmf):
    """songbird's K, L = 3, 50 (K*L = 150), four iterations of the block variant."""
    N, T, K, L = SHAPES["song_kl150"]
    data, W0, H0 = R.problem(N, T, K, L, seed=FIT_SEED)
    Wr, Hr, hist, nearW, nearH, floor = restated_fit(data, W0, H0, L, FIT_ITERS, "block")
    r = cmf.fit_cnmf(data, L=L, K=K, alg=cmf.ANLSUpdate, variant=":block", max_itr=FIT_ITERS, check_convergence=False, W_init=W0, H_init=H0,
                     options={"nnls_large": 1})
    tol = R.bar(floor, 1e-6)
    print(f"fit: floor {floor:.3e}, loss_hist {r.loss_hist.tolist()} vs {hist.tolist()}")
    assert len(r.loss_hist) == FIT_ITERS + 1 and (np.diff(r.loss_hist) <= 1e-12).all(), r.loss_hist
    same("fit W", r.W, Wr, nearW, tol)
    same("fit H", r.H, Hr, nearH, tol)
    print(f"fit: losses differ by {np.abs(r.loss_hist[1:] - hist[1:]).max():.3e} (bar {tol:.3e})")
    assert np.abs(r.loss_hist[1:] - hist[1:]).max() <= tol


def test_the_switch(cmf):
    N, T, K, L = SHAPES["kl129"]
    data, W0, H0 = R.problem(N, T, K, L, seed=0)
    rule = cmf.ANLSUpdate(data, W0, H0)
    try:
        def refused():
            W = W0.copy(order="F")
            with pytest.raises(cmf.CMFError) as ei:
                rule.update_motifs(data, W, H0)
            assert ei.value.code == 4 and "128" in str(ei.value) and np.array_equal(W, W0)

        refused()  # off: as before
        rule.set_option("nnls_large", 1)
        W = W0.copy(order="F")
        rule.update_motifs(data, W, H0)
        assert np.isfinite(W).all() and not np.array_equal(W, W0)
        rule.set_option("nnls_large", 0)
        refused()  # off again
        with pytest.raises(cmf.CMFError) as ei:
            rule.set_option("nnls_large", 2)
        assert ei.value.code == 1
        with pytest.raises(NotImplementedError, match="anls_backup_only"):
            rule.set_option("gram", 1)
    finally:
        rule.close()
    # up to 128 unknowns the option changes nothing, bit for bit
    n, t, k, l = R.CASES["kl128"][:4]
    data, W0, H0 = R.problem(n, t, k, l, seed=sorted(R.CASES).index("kl128"))
    out = []
    for on in (0, 1):
        rule = cmf.ANLSUpdate(data, W0, H0)
        try:
            rule.set_option("nnls_large", on)
            W = W0.copy(order="F")
            rule.update_motifs(data, W, H0)
            out.append((W, rule.last_W_exchanges))
        finally:
            rule.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    # beyond 1024 unknowns the entry refuses and names the bound
    data, W0, H0 = R.problem(4, 1100, 1, 1025, seed=0)
    rule = large_rule(cmf, data, W0, H0)
    try:
        W = W0.copy(order="F")
        with pytest.raises(cmf.CMFError) as ei:
            rule.update_motifs(data, W, H0)
        print("K*L = 1025:", ei.value)
        assert ei.value.code == 4 and "1024" in str(ei.value) and np.array_equal(W, W0)
    finally:
        rule.close()


def test_a_rank_deficient_problem_ends_with_an_error_and_leaves_the_factor(cmf):
    """At K*L = 150: two identical rows of H make G singular on any passive set that holds both; the call ends with code 4 -- by a
    non-positive pivot or, where rounding leaves a tiny positive one, by the cap on rounds -- and W is untouched.  A dead row is
    no such case: its component of W is zero and nothing is capped."""
    N, T, K, L = SHAPES["song_kl150"]
    data, W0, H0 = R.problem(N, T, K, L, seed=9)
    H = H0.copy(order="F")
    H[1] = H[0]
    rule = large_rule(cmf, data, W0, H0)
    try:
        W = W0.copy(order="F")
        with pytest.raises(cmf.CMFError) as ei:
            rule.update_motifs(data, W, H)
        print(f"identical rows: {ei.value}; anls_capped {rule.counter('anls_capped')}, rounds {rule.last_W_exchanges}")
        assert ei.value.code == 4 and np.array_equal(W, W0)
        H[1] = 0.0
        rule.update_motifs(data, W, H)
        assert np.isfinite(W).all() and (W[1] == 0).all() and rule.counter("anls_capped") == 0
    finally:
        rule.close()


# ---- the separable fit -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sep_reference(case):
    tup = SEP_CASES[case]
    data, tW, tH, K, L, thresh = S.case_data(tup)
    ol, orw, floors, margins = S.check_problem(case, data, K, L, noise_free=False, thresh=thresh)
    worst = {k: min(v) for k, v in margins["rewritten"].items()}
    print(f"{case}: least margins {worst}; near-degenerate {int(orw['near'].sum())} of {orw['near'].size}; floors {floors}")
    return data, K, L, thresh, orw, floors


@pytest.mark.parametrize("case", list(SEP_CASES))
def test_separable_fit_stage_by_stage(cmf, case):
    """R = K*L = 160 and 150: test_gpu_sep.run_case with the option on."""
    data, K, L, thresh, ref, floors = sep_reference(case)
    rule = cmf.Separable(data, K, L)
    try:
        vertices = rule.spa(thresh=thresh)
        assert vertices == ref["vertices"], (case, vertices, ref["vertices"])
        with pytest.raises(cmf.CMFError) as ei:  # off: refused as before
            rule.nnls(vertices)
        assert ei.value.code == 4 and "128" in str(ei.value)
        with pytest.raises(NotImplementedError, match="nnls_large"):
            rule.set_option("gram", 1)
        rule.set_option("nnls_large", 1)
        V, G = rule.nnls(vertices)
        close(case + " V", V, ref["V"], floors["V"])
        close(case + " G", G, ref["G"], floors["G"])
        mism = ((G > 0) != (ref["G"] > 0)) & ~ref["near"]
        print(f"{case} G: pattern mismatches {int(mism.sum())} off {int(ref['near'].sum())} near-degenerate entries; exchanges {rule.last_nnls_exchanges}")
        assert (G >= 0).all() and not mism.any() and rule.last_nnls_exchanges > 0
        P, head = rule.shift_table(ref["G"])  # (each stage on the restatement's input, so that its bar is its own)
        close(case + " P", P, ref["P"], floors["P"])
        close(case + " head", head, ref["head"], floors["P"])
        groups = rule.cluster(*rule.shift_table(G))
        assert groups == ref["groups"], (case, groups, ref["groups"])
        W, H = rule.construct(ref["V"], ref["G"], ref["groups"])
        close(case + " construct W", W, ref["W0"], 0.0)
        close(case + " construct H", H, ref["H0"], floors["H0"])
    finally:
        rule.close()
    with pytest.raises(cmf.CMFError) as ei:
        cmf.separable_fit(data, K, L, thresh=thresh)
    assert ei.value.code == 4
    stages = {}
    W, H = cmf.separable_fit(data, K, L, thresh=thresh, stages=stages, nnls_large=True)
    assert stages["vertices"] == ref["vertices"] and stages["groups"] == ref["groups"], case
    close(case + " fit W", W, ref["W0"], floors["W0"])
    close(case + " fit H", H, ref["H0"], floors["H0"])


def test_fit_cnmf_passes_the_switch_on(cmf):
    import warnings

    data, K, L, thresh, ref, floors = sep_reference("r150")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (the keyword is a known one)
        r = cmf.fit_cnmf(data, K=K, L=L, alg=":sep", thresh=thresh, nnls_large=True)
    close("fit_cnmf W", r.W, ref["W0"], floors["W0"])
    close("fit_cnmf H", r.H, ref["H0"], floors["H0"])


def test_refit_w_past_the_bound(cmf):
    """refit_W at R = 150 = the ANLS W step on the fit's H (test_gpu_sep.test_refits): one round per unit with all 150 unknowns
    passive, the largest factorisation the kernel can meet at that shape."""
    data, K, L, thresh, ref, floors = sep_reference("r150")
    sg = {}
    Wr = R.update_motifs(data, ref["H0"], L, stats=sg)
    # the floor of the refitted W: the two modes of the whole fit, so that what the earlier stages differ by is carried along
    Wl, _ = S.fit(data, K, L, thresh=thresh, refit_W=True, mode="literal")
    Wg, _ = S.fit(data, K, L, thresh=thresh, refit_W=True)
    assert np.array_equal(Wg, Wr)
    floor = R.rel(Wl, Wr)
    print(f"refit_W: restatement rounds {sg['exchanges']}, near-degenerate {int(sg['near'].sum())} of {Wr.size}, capped {sg['capped']}")
    assert sg["capped"] == 0 and sg["near"].sum() <= 0.01 * Wr.size
    W, H = cmf.separable_fit(data, K, L, thresh=thresh, refit_W=True, nnls_large=True)
    close("refit_W W", W, Wr, floor)
    mism = ((W > 0) != (Wr > 0)) & ~sg["near"]
    print(f"refit_W: pattern mismatches {int(mism.sum())} off {int(sg['near'].sum())} near-degenerate entries")
    assert not mism.any()
    close("refit_W H (untouched)", H, ref["H0"], floors["H0"])
