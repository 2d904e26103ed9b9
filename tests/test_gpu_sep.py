"""The separable fit on the GPU (cmf_sep_*; Separable; separable_fit; fit_cnmf(alg=":sep")) against the fp64 restatement
tests/sep_restatement.py (src/algs/separable.jl), stage by stage and end to end.

Decisions (vertices, groups, the order inside a group) are compared exactly.  That is meaningful because every input is first
checked on the CPU (sep_restatement.check_problem): the restatement's two modes take the same decisions and every decision has a
margin of at least 1e-6.  Values (V, G, P, head, W, H) follow the project's fp64 rule: within 1000 x the literal-vs-rewritten
difference of the same input, never looser than 1e-8 (anls_restatement.bar); the zero pattern of G is identical off the entries
the solver itself calls near-degenerate.  After refit_H (the fp32 HALS sweep) H is held to 1e-4 norm-wise against the oracle's
sweep from the same factors.  Every test prints the measured distance beside its bar.
"""
import functools

import numpy as np
import pytest

import anls_restatement as A
import sep_restatement as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build(quiet=True)
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


@functools.lru_cache(maxsize=None)
def reference(case, pre=None, spectral=False):
    """The restatement's stages, floors and margins for one input (CPU).  `case`: a name of sep_restatement.CASES or a tuple."""
    data, tW, tH, K, L, thresh = S.case_data(case)
    noise = (S.CASES[case] if case in S.CASES else case)[4]
    ol, orw, floors, margins = S.check_problem(str(case), data, K, L, noise_free=(noise == 0), thresh=thresh, pre=pre, spectral=spectral)
    worst = {k: min(v) for k, v in margins["rewritten"].items()}
    print(f"{case} pre={pre} spectral={spectral}: least margins {worst}; near-degenerate {int(orw['near'].sum())} of {orw['near'].size}")
    return data, K, L, thresh, orw, floors


def close(name, X, Xr, floor):
    d, tol = A.rel(X, Xr), A.bar(floor, 1e-8)
    print(f"{name}: rel {d:.3e} (bar {tol:.3e}, floor {floor:.3e})")
    assert np.isfinite(X).all() and d <= tol, (name, d, tol)


def run_case(cmf, case, pre=None, spectral=False):
    data, K, L, thresh, ref, floors = reference(case, pre, spectral)
    name = f"{case} pre={pre} spectral={spectral}"
    rule = cmf.Separable(data, K, L)
    try:
        vertices = rule.spa(thresh=thresh, pre=pre)
        assert vertices == ref["vertices"], (name, vertices, ref["vertices"])
        V, G = rule.nnls(vertices)
        close(name + " V", V, ref["V"], floors["V"])
        close(name + " G", G, ref["G"], floors["G"])
        mism = ((G > 0) != (ref["G"] > 0)) & ~ref["near"]
        print(f"{name} G: pattern mismatches {int(mism.sum())} off {int(ref['near'].sum())} near-degenerate entries; exchanges {rule.last_nnls_exchanges}")
        assert (G >= 0).all() and not mism.any() and rule.last_nnls_exchanges > 0
        P, head = rule.shift_table(ref["G"])  # (each stage on the restatement's input, so that its bar is its own)
        close(name + " P", P, ref["P"], floors["P"])
        close(name + " head", head, ref["head"], floors["P"])
        groups = rule.cluster(*rule.shift_table(G), spectral=spectral)
        assert groups == ref["groups"], (name, groups, ref["groups"])
        W, H = rule.construct(ref["V"], ref["G"], ref["groups"])
        close(name + " construct W", W, ref["W0"], 0.0)
        close(name + " construct H", H, ref["H0"], floors["H0"])
    finally:
        rule.close()
    stages = {}
    W, H = cmf.separable_fit(data, K, L, thresh=thresh, pre=pre, spectral=spectral, stages=stages)
    assert stages["vertices"] == ref["vertices"] and stages["groups"] == ref["groups"], name
    close(name + " fit W", W, ref["W0"], floors["W0"])
    close(name + " fit H", H, ref["H0"], floors["H0"])
    return data, K, L, thresh, ref, W, H


@pytest.mark.parametrize("pre", [None, ":svd", ":svdcond"])
@pytest.mark.parametrize("case", ["ref_clean", "ref_noisy"])
def test_reference_shape(cmf, case, pre):
    """N=100, T=250, K=3, L=5 (test/sep_test.jl:10): noise-free (every pure column occurs twice: the col2 tie-break decides) and
    with noise_level * rand and thresh = 0.2 N - noise_level (sep_test.jl:14-17)."""
    data, K, L, thresh, ref, W, H = run_case(cmf, case, pre=pre)
    tH = S.case_data(case)[2]
    score = cmf.cos_score(tH, H[cmf.permute_factors(tH, H)])
    print(f"{case} pre={pre}: cos_score against the planted H {score:.4f}")
    assert score > 0.99


def test_spectral_grouping(cmf):
    run_case(cmf, "ref_noisy", spectral=True)


@pytest.mark.parametrize("case", ["k1", "l1", "r128", "t_prime"])
def test_edge_shapes(cmf, case):
    """K = 1; L = 1; R = K*L = 128 (the bound of the NNLS step); a prime T."""
    run_case(cmf, case)


def test_figure_shape(cmf):
    """N=250, T=50 000, K=5, L=20."""
    run_case(cmf, S.FIG + (0.1, None, 1))


def test_fit_cnmf_maps_sep(cmf):
    data, K, L, thresh, ref, floors = reference("ref_noisy", ":svdcond")
    r = cmf.fit_cnmf(data, K=K, L=L, alg=":sep", thresh=thresh, pre=":svdcond", max_itr=7)
    close("fit_cnmf W", r.W, ref["W0"], floors["W0"])
    close("fit_cnmf H", r.H, ref["H0"], floors["H0"])
    loss = np.linalg.norm(A.conv(ref["W0"], ref["H0"]) - data) / np.linalg.norm(data)
    print(f"fit_cnmf loss {r.loss_hist[0]!r} vs {loss!r}")
    assert len(r.loss_hist) == 1 and len(r.time_hist) == 1 and r.time_hist[0] > 0
    assert abs(r.loss_hist[0] - loss) <= 1e-5  # (compute_loss is the fp32 MU path)


def test_refits(cmf, oracle):
    """refit_W = the ANLS W step (fp64) on the fit's H; refit_H = refit_H_itr fp32 HALS sweeps from the refitted W."""
    data, K, L, thresh, ref, floors = reference("ref_noisy")
    sg = {}
    Wr = A.update_motifs(data, ref["H0"], L, stats=sg)
    # the floor of the refitted W: the two modes of the whole fit, so that what the earlier stages differ by is carried along
    Wl, _ = S.fit(data, K, L, thresh=thresh, refit_W=True, mode="literal")
    Wg, _ = S.fit(data, K, L, thresh=thresh, refit_W=True)
    assert np.array_equal(Wg, Wr)
    floor = A.rel(Wl, Wr)
    W, H = cmf.separable_fit(data, K, L, thresh=thresh, refit_W=True)
    close("refit_W W", W, Wr, floor)
    mism = ((W > 0) != (Wr > 0)) & ~sg["near"]
    print(f"refit_W: pattern mismatches {int(mism.sum())} off {int(sg['near'].sum())} near-degenerate entries")
    assert not mism.any()
    close("refit_W H (untouched)", H, ref["H0"], floors["H0"])
    for kw, W0, wfloor in ((dict(refit_H=True), ref["W0"], floors["W0"]), (dict(refit_H=True, refit_W=True, refit_H_itr=4), Wr, floor)):
        W, H = cmf.separable_fit(data, K, L, thresh=thresh, **kw)
        Wo, Ho = np.array(W0, order="F"), np.array(ref["H0"], order="F")
        rule = oracle.HALSUpdate(data, Wo, Ho)
        for _ in range(kw.get("refit_H_itr", 10)):
            oracle.hals_update_feature_maps(rule, data, Wo, Ho, 0.0, 0.0)
        d = A.rel(H, Ho)
        print(f"refit_H {kw}: H rel {d:.3e} (bar 1e-4); moved from the fit's H by {A.rel(Ho, ref['H0']):.3e}")
        assert d <= 1e-4 and A.rel(Ho, ref["H0"]) > 1e-3
        close(f"refit_H {kw} W", W, W0, wfloor)


def test_refusals(cmf):
    rng = np.random.default_rng(0)
    data = np.asfortranarray(rng.random((160, 400)))
    rule = cmf.Separable(data, 129, 1)
    try:
        with pytest.raises(cmf.CMFError) as ei:  # R = 129 is beyond the NNLS step
            rule.nnls(list(range(129)))
        assert ei.value.code == 4 and "128" in str(ei.value)
        with pytest.raises(cmf.CMFError) as ei:  # a vertex that is no column
            rule.nnls([0, 400])
        assert ei.value.code == 1
        G = np.asfortranarray(rng.random((6, 400)))
        G[4] = 0.0
        with pytest.raises(cmf.CMFError) as ei:  # a zero row: its cosines are 0/0
            rule.shift_table(G, 3)
        assert ei.value.code == 4 and "row 4" in str(ei.value)
        with pytest.raises(ValueError):  # R <= min(N, T)
            rule.spa(R=161)
        lib = cmf.load_library()
        v = np.zeros(161, dtype=np.int64)
        import ctypes

        assert lib.cmf_sep_spa(rule._h, 161, 0.0, 0, None, v.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 1
    finally:
        rule.close()
    with pytest.raises(cmf.CMFError) as ei:
        cmf.separable_fit(data, 129, 1)
    assert ei.value.code == 4
    with pytest.raises(cmf.CMFError) as ei:  # every column below thresh: the residual is zero from the first round on
        cmf.Separable(data, 4, 1).spa(thresh=1e9)
    print("vanished residual:", ei.value)
    assert ei.value.code == 4


def test_spa_is_bit_repeatable(cmf):
    data, K, L, thresh, ref, floors = reference("ref_clean")
    outs = []
    for _ in range(2):
        rule = cmf.Separable(data, K, L)
        try:
            v = rule.spa(thresh=thresh)
            outs.append((v,) + rule.nnls(v) + rule.shift_table(ref["G"]))
        finally:
            rule.close()
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)
