"""The ANLS rule on the GPU (cmf_anls_*; ANLSUpdate; fit_cnmf(alg=ANLSUpdate)) against the fp64 restatement
tests/anls_restatement.py (src/algs/anls.jl).

Bars.  Both sides are fp64; the floor of a call is what the restatement's own two modes (two summation orders of the same
arithmetic) differ by on the same inputs.  A single call must land within 1000 x that floor and in no case looser than 1e-8
(the loss: 1e-10); the 10-iteration fit within 1000 x the floor of the fit, in no case looser than 1e-6 (anls_restatement.bar).
Zero patterns must be identical except on entries the restatement itself calls near-degenerate (a zero with
|y| < 1e-6 max|c|, a positive entry below 1e-6 max|x| of its problem), of which every shape has at most 1 %.  Every shape is
first checked on the CPU (anls_restatement.check_step): tol = 1e-5 and tol = 1e-12 end on the same passive sets, so what the
reference's package does with `tol` cannot change an answer here.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import anls_restatement as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


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


@functools.lru_cache(maxsize=None)
def reference(name, N, T, K, L, steps, variants, seed):
    """The restatement's answers, floors and near-degenerate masks for one shape (CPU; shared by the two solver modes)."""
    data, W0, H0 = R.problem(N, T, K, L, seed)
    out = {"data": data, "W0": W0, "H0": H0}
    W = W0
    if "w" in steps:
        sl, sg = {}, {}
        Wl = R.update_motifs(data, H0, L, mode="literal", stats=sl)
        W = R.update_motifs(data, H0, L, stats=sg)
        floor = R.check_step(name + " W", Wl, W, sl, sg, R.update_motifs(data, H0, L, tol=1e-12), R.bar(R.rel(Wl, W), 1e-8))
        out["W"] = (W, sg["near"], floor)
    out["Win"] = np.asfortranarray(W)
    for v in variants:
        sl, sg = {}, {}
        Hl, ll = R.update_feature_maps(data, W, H0, variant=v, mode="literal", stats=sl)
        Hg, lg = R.update_feature_maps(data, W, H0, variant=v, stats=sg)
        H12, _ = R.update_feature_maps(data, W, H0, variant=v, tol=1e-12)
        floor = R.check_step(f"{name} H {v}", Hl, Hg, sl, sg, H12, R.bar(R.rel(Hl, Hg), 1e-8))
        out[v] = (Hg, sg["near"], floor, lg, abs(ll - lg))
    return out


def run_shape(cmf, name, N, T, K, L, steps, variants, seed, backup_only):
    ref = reference(name, N, T, K, L, steps, variants, seed)
    data, W0, H0 = ref["data"], ref["W0"], ref["H0"]
    rule = cmf.ANLSUpdate(data, W0, H0)
    try:
        if backup_only:
            rule.set_option("anls_backup_only", 1)
        if "w" in steps:
            Wr, near, floor = ref["W"]
            W = W0.copy(order="F")
            rule.update_motifs(data, W, H0)
            same(f"{name} W", W, Wr, near, R.bar(floor, 1e-8))
            assert rule.counter("anls_capped") == 0 and rule.last_W_exchanges > 0
            if backup_only:
                assert rule.counter("anls_backup") > 0
        for v in variants:
            Hr, near, floor, lr, lfloor = ref[v]
            H = H0.copy(order="F")
            loss = rule.update_feature_maps(data, ref["Win"], H, variant=":" + v)
            same(f"{name} H {v}", H, Hr, near, R.bar(floor, 1e-8))
            print(f"{name} H {v}: loss {loss!r} vs {lr!r}")
            assert abs(loss - lr) <= R.bar(lfloor, 1e-10), (loss, lr)
            assert rule.counter("anls_capped") == 0 and rule.last_H_exchanges > 0
            if backup_only:
                assert rule.counter("anls_backup") > 0
    finally:
        rule.close()


@pytest.mark.parametrize("backup_only", [0, 1])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_single_calls_match_the_restatement(cmf, case, backup_only):
    run_shape(cmf, case, *R.CASES[case], seed=sorted(R.CASES).index(case), backup_only=backup_only)


@pytest.mark.parametrize("backup_only", [0, 1])
@pytest.mark.parametrize("variant", ["basic", "block"])
def test_figure_shape(cmf, variant, backup_only):
    """N = 250, T = 50 000, K = 5, L = 20 (figures/fast_bcd/synthetic_comparison.jl:58-67), once per variant; the W call rides
    with the basic variant."""
    run_shape(cmf, "fig_" + variant, *R.FIG, "wh" if variant == "basic" else "h", (variant,), seed=100, backup_only=backup_only)


@pytest.mark.parametrize("variant", ["basic", "block"])
def test_fit_matches_the_golden_fixture(cmf, variant):
    g = np.load(os.path.join(HERE, "golden", "fit_anls_n40_t600_10.npz"))
    r = cmf.fit_cnmf(g["data"], L=int(g["L"]), K=int(g["K"]), alg=cmf.ANLSUpdate, max_itr=10, check_convergence=False,
                     W_init=g["W_init"], H_init=g["H_init"], variant=":" + variant)
    assert len(r.loss_hist) == 11 and (np.diff(r.loss_hist) <= 1e-12).all(), r.loss_hist
    tol = R.bar(float(g[f"floor_{variant}"]), 1e-6)
    same(f"fit {variant} W", r.W, g[f"W_{variant}"], g[f"nearW_{variant}"], tol)
    same(f"fit {variant} H", r.H, g[f"H_{variant}"], g[f"nearH_{variant}"], tol)
    np.testing.assert_allclose(r.loss_hist[1:], g[f"loss_hist_{variant}"][1:], rtol=0, atol=max(tol, 1e-10))


def test_call_by_call_use_sees_the_callers_edits(cmf):
    """Nothing of the factors is cached on the device: a caller who zeroes a row of H and rescales a component of W between
    calls gets what the restatement gives for the edited factors."""
    N, T, K, L = 20, 260, 4, 6
    data, W0, H0 = R.problem(N, T, K, L, seed=11)
    r = cmf.fit_cnmf(data, L=L, K=K, alg=cmf.ANLSUpdate, max_itr=3, check_convergence=False, W_init=W0, H_init=H0)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    rule = cmf.ANLSUpdate(data, W, H)
    try:
        losses = []
        for _ in range(3):
            rule.update_motifs(data, W, H)
            losses.append(rule.update_feature_maps(data, W, H))
        assert np.array_equal(W, r.W) and np.array_equal(H, r.H) and np.array_equal(np.asarray(losses), r.loss_hist[1:])
        H[1] = 0.0  # a dead stacked row block: its unknowns stay zero, no special case
        H[:, ::3] *= 0.5
        Hed = H.copy()
        rule.update_motifs(data, W, H)
        sg = {}
        Wr = R.update_motifs(data, Hed, L, stats=sg)
        same("edited H -> W", W, Wr, sg["near"], 1e-8)
        assert (W[1] == 0).all() and np.array_equal(H, Hed)
        W[2] *= 3.0
        Wed = W.copy()
        loss = rule.update_feature_maps(data, W, H, variant="block")
        Hr, lr = R.update_feature_maps(data, Wed, Hed, variant="block", stats=sg)
        same("edited W -> H", H, Hr, sg["near"], 1e-8)
        assert abs(loss - lr) <= 1e-10 and np.array_equal(W, Wed)
    finally:
        rule.close()


def test_what_cannot_run_is_refused(cmf):
    lib = cmf.load_library()
    data, W0, H0 = R.problem(8, 5, 2, 6, seed=3)  # T < L
    rule = cmf.ANLSUpdate(data, W0, H0)
    try:
        H = H0.copy(order="F")
        with pytest.raises(cmf.CMFError) as ei:
            rule.update_feature_maps(data, W0, H, variant=":block")
        assert ei.value.code == 1 and np.array_equal(H, H0)
        with pytest.raises(ValueError):
            rule.update_feature_maps(data, W0, H, variant=":comb")
        with pytest.raises(NotImplementedError, match="anls_backup_only"):
            rule.set_option("gram", 1)
        with pytest.raises(cmf.CMFError):
            rule.set_option("anls_backup_only", 2)
        # the C entries: NULL pointers and a bad variant are CMF_ERR_ARG
        pd = ctypes.POINTER(ctypes.c_double)
        Wp, Hp = W0.ctypes.data_as(pd), H.ctypes.data_as(pd)
        assert lib.cmf_anls_update_motifs(rule._h, None, Wp) == 1 and lib.cmf_anls_update_motifs(rule._h, Hp, None) == 1
        assert lib.cmf_anls_update_feature_maps(rule._h, None, Hp, 0, None) == 1
        assert lib.cmf_anls_update_feature_maps(rule._h, Wp, Hp, 2, None) == 1
        assert lib.cmf_anls_prepare(rule._h, None) == 1
    finally:
        rule.close()
    # an unprepared handle is CMF_ERR_STATE
    mu = cmf.MultUpdate(data, W0, H0)
    try:
        pd = ctypes.POINTER(ctypes.c_double)
        assert lib.cmf_anls_update_motifs(mu._h, H0.ctypes.data_as(pd), W0.ctypes.data_as(pd)) == 3
        assert lib.cmf_anls_update_feature_maps(mu._h, W0.ctypes.data_as(pd), H0.ctypes.data_as(pd), 0, None) == 3
    finally:
        mu.close()
    for (N, T, K, L), call in (((8, 300, 3, 43), "W"), ((8, 40, 65, 1), "H")):  # K*L = 129; K = 65
        data, W0, H0 = R.problem(N, T, K, L, seed=3)
        rule = cmf.ANLSUpdate(data, W0, H0)
        try:
            with pytest.raises(cmf.CMFError) as ei:
                if call == "W":
                    rule.update_motifs(data, W0.copy(order="F"), H0)
                else:
                    rule.update_feature_maps(data, W0, H0.copy(order="F"))
            assert ei.value.code == 4
        finally:
            rule.close()
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.fit_cnmf(data, L=2, K=3, alg=cmf.ANLSUpdate, max_itr=1, devices=[0, 0])
    with pytest.raises(NotImplementedError, match="anls_backup_only"):
        cmf.fit_cnmf(data, L=2, K=3, alg=cmf.ANLSUpdate, max_itr=1, options={"no_such_option": 1})
    with pytest.raises(NotImplementedError):
        cmf.fit_cnmf(data, L=2, K=3, alg=":anls", max_itr=1)


def test_a_rank_deficient_problem_ends_with_an_error_and_leaves_the_factor(cmf):
    """Two identical rows of H make G singular on any passive set that holds both: the call reports it (no spin, no NaN
    factor) and W is untouched.  A dead row (all zero) is not such a case."""
    N, T, K, L = 6, 80, 3, 2
    data, W0, H0 = R.problem(N, T, K, L, seed=9)
    H = H0.copy(order="F")
    H[1] = H[0]
    rule = cmf.ANLSUpdate(data, W0, H0)
    try:
        W = W0.copy(order="F")
        with pytest.raises(cmf.CMFError) as ei:
            rule.update_motifs(data, W, H)
        assert ei.value.code == 4 and np.array_equal(W, W0)
        H[1] = 0.0
        rule.update_motifs(data, W, H)
        assert np.isfinite(W).all() and (W[1] == 0).all() and rule.counter("anls_capped") == 0
    finally:
        rule.close()
