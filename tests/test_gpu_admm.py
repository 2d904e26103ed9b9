"""The ADMM rule on the GPU (cmf_admm_*; ADMMUpdate; fit_cnmf(alg=":admm")) against the fp64 restatement
tests/admm_restatement.py (src/algs/admm.jl).  Bars for single calls: the same inner iteration counts and reverts, factors within
1e-8 (Frobenius-relative), the loss within 1e-10."""
import os

import numpy as np
import pytest

import admm_restatement as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build(quiet=True)
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def problem(N, T, K, L, seed, row_scale=False):
    rng = np.random.default_rng(seed)
    W = rng.random((K, N, L))
    H = rng.random((K, T)) * (rng.random((K, T)) < 0.3)
    data = R.conv(W, H) + 0.1 * rng.random((N, T))
    if row_scale:  # rows from 0.05x to 20x: the w[n] >= 1 rule rescales some stacked columns and leaves the others
        data *= np.geomspace(0.05, 20, N)[:, None]
    W0 = np.asfortranarray(rng.random((K, N, L)))
    H0 = np.asfortranarray(rng.random((K, T)))
    return np.asfortranarray(data), W0, H0


# (N, T, K, L, motif keywords, feature-map keywords, row_scale)
CASES = {
    "k5": (20, 300, 5, 7, {}, {}, False),
    "k1": (16, 200, 1, 6, {}, {}, False),
    "k33": (24, 150, 33, 3, {}, {}, False),
    "l1": (18, 250, 4, 1, {}, {}, False),
    "t_lt_2l": (12, 9, 3, 6, {}, {}, False),
    "t_prime": (14, 211, 3, 5, {}, {}, False),
    "t50000": (6, 50000, 3, 4, {}, {}, False),
    "signed": (15, 180, 4, 5, {"nonnegW": False}, {"nonnegH": False}, False),
    "l1h": (15, 180, 4, 5, {}, {"l1H": 0.3}, False),
    "norm_mix": (30, 240, 3, 4, {}, {}, True),
    "long_loop": (10, 120, 3, 4, {"admm_W_maxiter": 80, "admm_tol": -np.inf}, {"admm_H_maxiter": 80, "admm_tol": -np.inf}, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_single_calls_match_the_restatement(cmf, case):
    N, T, K, L, wkw, hkw, scale = CASES[case]
    data, W0, H0 = problem(N, T, K, L, seed=sorted(CASES).index(case), row_scale=scale)
    rule = cmf.ADMMUpdate(data, W0, H0)
    try:
        W = W0.copy(order="F")
        rule.update_motifs(data, W, H0, **wkw)
        stats = {}
        Wr, _, wi, wr = R.update_motifs(data, H0, L, rhow=wkw.get("rhow", 10), maxiter=wkw.get("admm_W_maxiter", 30),
                                        tol=wkw.get("admm_tol", 1e-4), nonneg=wkw.get("nonnegW", True), stats=stats)
        assert (rule.last_W_iters, rule.last_W_reverts) == (wi, wr)
        assert rel(W, Wr) < 1e-8, rel(W, Wr)
        if case == "norm_mix":
            assert any(0 < c < N for c in stats["scaled_cols"]), stats["scaled_cols"]
        H = H0.copy(order="F")
        loss = rule.update_feature_maps(data, W, H, **hkw)
        Hr, lr, hi, hr = R.update_feature_maps(data, W, rhoh=hkw.get("rhoh", 10), maxiter=hkw.get("admm_H_maxiter", 30),
                                               l1H=hkw.get("l1H", 0.0), tol=hkw.get("admm_tol", 1e-4), nonneg=hkw.get("nonnegH", True))
        assert (rule.last_H_iters, rule.last_H_reverts) == (hi, hr)
        assert rel(H, Hr) < 1e-8, rel(H, Hr)
        assert abs(loss - lr) < 1e-10, (loss, lr)
    finally:
        rule.close()


def test_shape_limits_are_refused(cmf):
    data, W0, H0 = problem(8, 5, 2, 6, seed=3)  # T < L
    rule = cmf.ADMMUpdate(data, W0, H0)
    try:
        with pytest.raises(cmf.CMFError) as ei:
            rule.update_feature_maps(data, W0, H0.copy(order="F"))
        assert ei.value.code == 1
    finally:
        rule.close()
    data, W0, H0 = problem(8, 40, 65, 2, seed=3)
    rule = cmf.ADMMUpdate(data, W0, H0)
    try:
        with pytest.raises(cmf.CMFError) as ei:
            rule.update_feature_maps(data, W0, H0.copy(order="F"))
        assert ei.value.code == 4
    finally:
        rule.close()
    with pytest.raises(NotImplementedError):
        cmf.fit_cnmf(data, L=2, K=3, alg=":admm", max_itr=1, devices=[0, 0])
    with pytest.raises(NotImplementedError, match="no library options"):
        cmf.fit_cnmf(data, L=2, K=3, alg=":admm", max_itr=1, options={"gram": 1})


def test_fit_matches_the_golden_fixture(cmf):
    g = np.load(os.path.join(HERE, "golden", "fit_admm_n40_t600_10.npz"))
    assert g["margin_tol"] >= 1e-7 and g["margin_zero"] >= 1e-7  # no decision of the recorded fit is a tie
    rule_counts = []
    orig = cmf.ADMMUpdate.update_feature_maps

    def counting(self, *a, **kw):
        loss = orig(self, *a, **kw)
        rule_counts.append((self.last_W_iters, self.last_W_reverts, self.last_H_iters, self.last_H_reverts))
        return loss

    cmf.ADMMUpdate.update_feature_maps = counting
    try:
        r = cmf.fit_cnmf(g["data"], L=int(g["L"]), K=int(g["K"]), alg=":admm", max_itr=10, check_convergence=False,
                         W_init=g["W_init"], H_init=g["H_init"])
    finally:
        cmf.ADMMUpdate.update_feature_maps = orig
    assert rel(r.W, g["W"]) < 1e-6 and rel(r.H, g["H"]) < 1e-6
    np.testing.assert_allclose(r.loss_hist[1:], g["loss_hist"][1:], rtol=0, atol=1e-9)
    assert [tuple(c) for c in g["counts"]] == rule_counts


def test_call_by_call_loop_gives_the_bits_of_fit(cmf):
    data, W0, H0 = problem(20, 260, 4, 6, seed=11)
    r = cmf.fit_cnmf(data, L=6, K=4, alg=cmf.ADMMUpdate, max_itr=3, check_convergence=False, W_init=W0, H_init=H0)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    rule = cmf.ADMMUpdate(data, W, H)
    try:
        losses = []
        for _ in range(3):
            rule.update_motifs(data, W, H)
            losses.append(rule.update_feature_maps(data, W, H))
    finally:
        rule.close()
    assert np.array_equal(W, r.W) and np.array_equal(H, r.H)
    assert np.array_equal(np.asarray(losses), r.loss_hist[1:])


def test_a_caller_who_edits_H_between_calls_gets_the_reference_answer(cmf):
    data, W0, H0 = problem(16, 220, 3, 5, seed=5)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    rule = cmf.ADMMUpdate(data, W, H)
    try:
        rule.update_motifs(data, W, H)
        rule.update_feature_maps(data, W, H)
        H[:, ::3] *= 0.5  # the caller edits H in place
        H[1] = 0.0
        Hed = H.copy()
        rule.update_motifs(data, W, H)
        Wr, _, wi, wr = R.update_motifs(data, Hed, 5)
        assert rel(W, Wr) < 1e-8 and (rule.last_W_iters, rule.last_W_reverts) == (wi, wr)
    finally:
        rule.close()


def test_one_outer_iteration_at_config_2(cmf):
    """Config 2 (N=2000, T=50000, K=32, L=20), the shape the fp64 argument is about: the 640 x 640 Cholesky of G, the solve over
    2000 columns, K=32 factorisations over 25001 frequencies.  One update_motifs! and one update_feature_maps! from init_rand's
    start against the restatement computed here: factors within 1e-6, the same inner counts and reverts."""
    N, T, K, L = 2000, 50000, 32, 20
    data = np.asarray(cmf.gen_synthetic(N=N, T=T, seed=1234))
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
    W, H = np.array(W0, order="F"), np.array(H0, order="F")
    rule = cmf.ADMMUpdate(data, W, H)
    try:
        rule.update_motifs(data, W, H)
        loss = rule.update_feature_maps(data, W, H)
        counts = (rule.last_W_iters, rule.last_W_reverts, rule.last_H_iters, rule.last_H_reverts)
    finally:
        rule.close()
    tw, th = [], []
    Wr, _, wi, wr = R.update_motifs(data, np.asarray(H0), L, loss_trace=tw)
    Hr, lr, hi, hr = R.update_feature_maps(data, Wr, loss_trace=th)
    margins = [R.decision_margins(tr, 1e-4) for tr in (tw, th)]
    assert counts == (wi, wr, hi, hr), (counts, (wi, wr, hi, hr), margins)
    assert rel(W, Wr) < 1e-6, rel(W, Wr)
    assert rel(H, Hr) < 1e-6, rel(H, Hr)
    assert abs(loss - lr) < 1e-9, (loss, lr)
