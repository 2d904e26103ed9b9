"""CPU half of tests/test_exact_parity.py and tests/test_gpu_divergence_paths.py: the integer problems' preconditions over the whole
shape table, the ulp comparator's power to see one missing term, the launch-path names kept equal to the library's table, and for
the divergence forms the problems, the restated halves, the sensitivity condition and the element-wise check's power to see
corruptions a Frobenius-relative 1e-4 passes; and for the masked MU rule and the PGD rule (tests/test_gpu_exact_masked_mu.py,
tests/test_gpu_exact_pgd.py) the preconditions on the whole table, a float32 model of the PGD half-step and the same kind of mutations;
and for the HALS sweeps (tests/test_gpu_exact_hals.py) the launch names, the plan mirror, the preconditions and the float32 model on every row
of HALS_SHAPES, the bars made from them, and the local errors of a sweep kernel as mutations of the restatement."""
import os
import re

import numpy as np
import pytest

import exact_problems as ep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_table():
    """(N, T, K, L) of the table the two GPU files share."""
    return [s[:4] for s in ep.SHAPES]


def test_preconditions_hold_for_every_shape_in_the_table():
    shapes = _gpu_table() + [(2000, 50000, 32, 20)]  # (+ config 2, run once)
    assert len(shapes) > 30
    for shape in shapes:
        for family in ("W", "H"):
            b = ep.preconditions(*shape, family)
            assert b["exact"] and b["sensitive"], (shape, family, b)
            if shape[3] <= 32:
                assert b["loss_exact"], (shape, family, b)


def test_preconditions_bound_the_actual_sums():
    """The closed-form bounds are bounds: on small problems the contractions formed in fp64 stay below them."""
    from oracle import cmf_oracle as oracle

    for shape in [(30, 200, 5, 7), (20, 90, 32, 20), (7, 40, 3, 64)]:
        N, T, K, L = shape
        for family in ("W", "H"):
            W, H, X = ep.make_problem(N, T, K, L, family)
            b = ep.preconditions(N, T, K, L, family)
            est = oracle.tensor_conv(W, H)
            assert est.max() <= b["est"]
            if family == "W":
                for lag in range(min(L, T)):
                    assert (H[:, : T - lag] @ X[:, lag:].T).max() <= b["num"]
                    assert (H[:, : T - lag] @ est[:, lag:].T).max() <= b["den"]
            else:
                assert oracle.tensor_transconv(W, X).max() <= b["num"]
                assert oracle.tensor_transconv(W, est).max() <= b["den"]
            assert np.all(X == np.round(X)) and X.min() >= 0 and X.max() <= ep.XMAX
            # every column / (n, l) contributes: the factor that is NOT updated has exactly one nonzero per column / (n, l)
            if family == "W":
                assert np.array_equal((H != 0).sum(axis=0), np.ones(T))
            else:
                assert np.array_equal((W != 0).sum(axis=0), np.ones((N, L)))


def _w_half(W, H, X, drop_t=None, drop_den_lag=None):
    from oracle import cmf_oracle as oracle

    K, N, L = W.shape
    T = H.shape[1]
    est = oracle.tensor_conv(W, H)
    num, den = np.zeros(W.shape), np.zeros(W.shape)
    Hn = H.copy()
    if drop_t is not None:
        Hn[:, drop_t] = 0.0  # one t row of num missing
    for lag in range(min(L, T)):
        num[:, :, lag] = Hn[:, : T - lag] @ X[:, lag:].T
        if lag != drop_den_lag:
            den[:, :, lag] = H[:, : T - lag] @ est[:, lag:].T
    eps = float(np.finfo(np.float64).eps)
    return np.maximum(W * (num / (((den + ep.L1) + 2 * ep.L2 * W) + eps)), eps)


def test_ulp_comparator_sees_one_missing_term():
    N, T, K, L = 40, 300, 5, 8
    W, H, X = ep.make_problem(N, T, K, L, "W")
    ref = _w_half(W, H, X)
    true32 = ref.astype(np.float32)
    assert ep.ulps(true32, ref).max() <= 1  # the correctly rounded result passes the 2 ulp bar
    for got in (_w_half(W, H, X, drop_t=T // 2), _w_half(W, H, X, drop_den_lag=L - 1)):
        u = ep.ulps(got.astype(np.float32), ref)
        assert u.max() > 2, "a single dropped term must fail the bar"
        assert ep.first_bad(u > 2, "knl") is not None


def test_launch_path_names_match_the_library():
    src = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_internal.h")).read()
    m = re.search(r"kLaunchNames\[\] = \{(.*?)\};", src, re.S)
    assert m, "kLaunchNames table not found"
    assert re.findall(r'"([^"]+)"', m.group(1)) == ep.LAUNCH_PATHS
    assert len(set(ep.LAUNCH_PATHS)) == len(ep.LAUNCH_PATHS)


def test_plan_mirror_covers_the_instances():
    """The table reaches every hxt_kernel<LP>, transconv_kernel<LT> and few-component instance by the plan rules (the GPU test
    confirms with the counters)."""
    shapes = _gpu_table()
    general = [s for s in shapes if s[2] > 16]
    assert {ep.hxt_lp(s[3]) for s in general} == set(ep.HXT_LP)
    assert {ep.transconv_lt(s[3]) for s in general} == {4, 8, 12, 16, 20, 24, 28, 32}
    small = [ep.small_k_plan(*s) for s in shapes if s[2] <= 16]
    assert {p[0] for p in small if not p[1]} == set(range(1, 11))
    assert {p[0] for p in small if p[1]} == {1, 2, 3}
    assert {p[2] for p in small if not p[3]} == set(range(1, 7))
    assert {p[2] for p in small if p[3]} == {1, 2, 3}
    assert any(p[4] > 1 for p in small)
    assert {min(8, {5: 6, 7: 8}.get(p[5], p[5])) for p in small} == {1, 2, 3, 4, 6, 8}
    k32 = [s for s in shapes if s[2] % 32 == 0 and s[3] == 20]
    assert {ep.conv3_form(s[0], s[1]) for s in k32} >= {"whole", "whole+4", "whole+16", "pieces4", "pieces16"}


# ---- the divergence forms (tests/test_gpu_divergence_paths.py) ----------------------------------------------------------------
BARS_FILE = os.path.join(ROOT, "profiles", "mu_divergence_elementwise.txt")
MUTATION_SHAPES = [(130, 700, 32, 20), (70, 600, 20, 10), (90, 610, 5, 7)]


def test_whole_few_component_tiles_are_in_the_table():
    """launch_conv's few-component grid: every older row is quarter pieces only; the added row runs 1024 whole tiles and 16 cut."""
    small = [s for s in _gpu_table() if s[2] <= 16]
    whole = [s for s in small if ep.conv_small_form(s[0], s[1])[0] > 0]
    assert whole == [(1000, 4100, 8, 10)]
    assert ep.conv_small_form(1000, 4100) == (1024, 16) and ep.conv_small_form(1000, 4100, conv_split=0) == (1040, 0)
    assert (8 + 1) // 2 <= 4 and 1040 <= 4 * 4 * ep.N_CU  # (the preloaded data tile: at most 4 k pairs, at most 4 rounds)


def oracle_conv(W, H):
    from oracle import cmf_oracle as oracle

    return oracle.tensor_conv(W, H)


def test_divergence_problem():
    N, T, K, L = 90, 610, 5, 7
    for family in ("W", "H"):
        W0, H0, _ = ep.make_problem(N, T, K, L, family)
        W, H, X, mask = ep.make_divergence_problem(N, T, K, L, family)
        _, _, Xz, maskz = ep.make_divergence_problem(N, T, K, L, family, zeros=True)
        assert np.array_equal(W, W0) and np.array_equal(H, H0)
        assert X.min() == ep.DIV_XMIN and X.max() == ep.DIV_XMAX and np.all(X == np.round(X))
        assert len(np.unique(X)) == ep.DIV_XMAX - ep.DIV_XMIN + 1
        zero = Xz == 0
        assert 0.10 < zero.mean() < 0.15 and np.array_equal(Xz[~zero], X[~zero])
        assert np.array_equal(mask, maskz) and set(np.unique(mask)) == {0.0, 1.0} and 0.2 < (mask == 0).mean() < 0.3
        Xr = ep.make_divergence_problem(N, T, K, L, family, relative=True)[2]
        est = oracle_conv(W, H)
        assert np.array_equal(Xr * 16, X * est) and np.array_equal(Xr.astype(np.float32), Xr) and (Xr / est).min() >= 1 and (Xr / est).max() < 2
        assert np.array_equal(mask[:, :608].reshape(N, -1, 8).min(axis=2), mask[:, :608].reshape(N, -1, 8).max(axis=2))  # blocks of 8


@pytest.mark.parametrize("shape", MUTATION_SHAPES[1:], ids=str)
def test_divergence_half_is_the_restatements(shape):
    """divergence_half (the restatement's operations with the intermediate arrays kept) gives the bits of the restatements' own
    update_motifs / update_feature_maps, in fp64 and in the float32 model."""
    import beta_mu_restatement as br
    import is_mu_restatement as ir
    import kl_mu_restatement as kr
    import masked_kl_mu_restatement as mk
    import masked_pq_mu_restatement as pm

    N, T, K, L = shape
    for family in ("W", "H"):
        W, H, X, mask = ep.make_divergence_problem(N, T, K, L, family, zeros=True)
        Xp = ep.make_divergence_problem(N, T, K, L, family)[2]
        for form, (kind, beta, masked, zeros_ok, relative) in ep.FORMS.items():
            for dt in (np.float64, np.float32):
                data = ep.make_divergence_problem(N, T, K, L, family, zeros=zeros_ok, relative=True)[2] if relative else X if zeros_ok else Xp
                a = ep.divergence_half(form, family, data, mask, W, H, cdtype=dt, edtype=dt)
                Wr, Hr = W.copy(order="K"), H.copy(order="K")  # (the layout decides the order of the BLAS sums)
                if kind == ":kl" and masked:
                    args, kw, mod = (mk.MaskedKL(data, mask), Wr, Hr), dict(cdtype=dt), mk
                elif kind == ":kl":
                    args, kw, mod = (data, Wr, Hr), dict(cdtype=dt), kr
                elif masked:  # (update_feature_maps takes the observed count between the mask and the factors)
                    xs, count = pm.check_data(data, mask, ep.pq_beta(form))
                    args = (xs, mask, Wr, Hr, ep.pq_beta(form)) if family == "W" else (xs, mask, count, Wr, Hr, ep.pq_beta(form))
                    kw, mod = dict(cdtype=dt, edtype=dt), pm
                elif kind == ":itakura_saito":
                    args, kw, mod = (data, Wr, Hr), dict(cdtype=dt, edtype=dt), ir
                else:
                    args, kw, mod = (data, Wr, Hr, beta), dict(cdtype=dt, edtype=dt), br
                if family == "W":
                    mod.update_motifs(*args, l1W=ep.L1, l2W=ep.L2, **kw)
                    assert np.array_equal(a["new"], Wr), (form, family, dt)
                else:
                    loss = mod.update_feature_maps(*args, l1H=ep.L1, l2H=ep.L2, **kw)
                    assert np.array_equal(a["new"], Hr), (form, family, dt)
                    if dt is np.float64 or kind != ":kl":  # (the KL restatements' own loss has no float32 epilogue)
                        assert loss == a["loss"], (form, dt)
                    else:
                        assert abs(loss - a["loss"]) <= 1e-5 * loss


def test_bars_file_states_the_condition():
    """One bar and one loss bar per form, of the expected size, and every row's sensitivity at least 4 bars."""
    bars = ep.read_bars(BARS_FILE)
    assert set(bars["bar"]) == set(bars["lossbar"]) == set(ep.FORMS)
    for form in ep.FORMS:
        # (8 x a model error between one fp32 rounding and a few tens of them: sums of some hundred to a thousand terms)
        assert 4e-7 <= bars["bar"][form] <= 2e-5 and 1e-7 <= bars["lossbar"][form] <= 2e-5, (form, bars)
    rows = [ln.split() for ln in open(BARS_FILE) if ln.startswith("row ")]
    variants = sum(2 if f[3] else 1 for f in ep.FORMS.values())
    assert len(rows) == variants * 2 * len(ep.SHAPES)
    for r in rows:
        sens = float(r[-1].split("=")[-1])
        assert sens >= 4 * bars["bar"][r[1].split("+")[0]], r


@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=str)
def test_sensitivity_from_the_arrays(shape):
    """The condition again from arrays generated here; the closed-form bound is a lower bound of the exact value; and the definition
    itself: removing the one smallest term of the most fragile element moves it by the value returned."""
    bars = ep.read_bars(BARS_FILE)["bar"]
    N, T, K, L = shape
    for family in ("W", "H"):
        for zeros in (False, True):
            for form, f in ep.FORMS.items():
                if zeros and not f[3]:
                    continue
                W, H, X, mask = ep.make_divergence_problem(N, T, K, L, family, zeros=zeros, relative=f[4])
                a = ep.divergence_half(form, family, X, mask, W, H)
                s, lo = ep.sensitivity(form, a), ep.sensitivity(form, a, exact=False)
                assert lo <= s * (1 + 1e-12) and s >= 4 * bars[form], (form, family, zeros, s, lo)
    # the definition, on the W half of the Itakura-Saito form: brute force over every element's numerator terms
    W, H, X, mask = ep.make_divergence_problem(N, T, K, L, "W", relative=True)
    a = ep.divergence_half("is", "W", X, mask, W, H)
    comp = np.argmax(H, axis=0)
    k, n, lag = 1, N // 2, min(L, T) - 1
    cols = np.flatnonzero(comp == k)
    terms = a["P"][n, cols[cols + lag < T] + lag]
    assert np.isclose(terms.sum(), a["num"][k, n, lag], rtol=1e-12)
    moved = 1.0 - np.sqrt((a["num"][k, n, lag] - terms.min()) / a["num"][k, n, lag])
    assert moved >= ep.sensitivity("is", a) * (1 - 1e-9)
    assert np.isclose(ep._min_positive_terms("W", a["P"], W, H)[k, n, lag], terms.min(), rtol=0)


SENTINEL = -1.0  # cmf_kernels.h CMF_PQ_HELD_OUT


def _corruptions(family, has_q, pq_masked=False):
    """name -> corrupt(stage, arrays) for divergence_half: the damage a seam error in an epilogue or a contraction would do."""
    big = 1.0 / ep.EPS

    def strip(which):
        def f(stage, a):  # one 4-row strip of a 64 x 64 block zeroed (a piece of a cut tile that stored P but not Q, or neither)
            if stage == "sources":
                a[which] = a[which].copy()
                a[which][8:12, 192:256] = 0.0
        return f

    def lag(stage, a):  # C2 loses its last lag over one time chunk
        if stage == "sums":
            l = a["num"].shape[2] - 1
            a["num"][:, :, l] -= a["H"][:, 128:384] @ a["P"][:, 128 + l:384 + l].T

    def kpair(stage, a):  # C3 loses one k pair of one 32-unit block over one 64-column tile
        if stage == "sums":
            W, P = a["W"], a["P"]
            for l in range(W.shape[2]):
                a["num"][2:4, 64:128] -= W[2:4, :32, l] @ P[:32, 64 + l:128 + l]

    def pad(stage, a):  # the contraction runs one column past T, where Q holds 1 / eps instead of the selected 0
        if stage == "sums":
            T = a["H"].shape[1]
            for l in range(1, a["W"].shape[2]):
                if family == "W":
                    a["den"][:, :, l] += a["H"][:, T - l][:, None] * big
                else:
                    a["den"][:, T - l] += a["W"][:, :, l].sum(axis=1) * big

    def double(stage, a):  # one time row of P counted twice
        if stage == "sums":
            t0 = 300
            for l in range(a["W"].shape[2]):
                if family == "W":
                    a["num"][:, :, l] += a["H"][:, t0 - l][:, None] * a["P"][:, t0][None, :]
                else:
                    a["num"][:, t0 - l] += a["W"][:, :, l] @ a["P"][:, t0]

    def term(stage, a):  # ONE term missing from the numerator of ONE element (the unit of exact_problems.sensitivity)
        if stage == "sums":
            if family == "W":
                k, n, l = 1, 5, 2
                t = [t for t in np.flatnonzero(a["H"][k] != 0)[3:] if a["P"][n, t + l] > 0][0]  # (a held-out entry is no term)
                a["num"][k, n, l] -= a["P"][n, t + l]
            else:
                k, t = 1, 100
                n, l = [(n, l) for l in range(a["W"].shape[2]) for n in np.flatnonzero(a["W"][k, :, l] != 0) if a["P"][n, t + l] > 0][0]
                a["num"][k, t] -= a["P"][n, t + l]

    # What only a sentinel family (Itakura-Saito or beta under the mask) can suffer, inside the strip of strip() above:
    def unselected(a):
        """(P, Q) of the form before the select, from the data with the sentinel under the mask (cmf_kernels.h CMF_PQ_HELD_OUT): Q of a
        held-out entry is 1 / e (e^(beta - 1)), P is the form's product taken on the sentinel, (x q) q or x e^(beta - 2).  (The device's
        beta P has a select x > 0 of its own, which happens to give 0 for the sentinel; the damage modelled is the product.)"""
        import kl_mu_restatement as kr

        beta, xs = ep.pq_beta(a["form"]), np.where(a["mask"] != 0, a["X"], SENTINEL)
        e = kr.tensor_conv(a["W"], a["H"]) + ep.EPS
        return ((xs / e) / e, 1.0 / e) if beta == 0 else (xs * e ** (beta - 2.0), e ** (beta - 1.0))

    def leak(which):
        def f(stage, a):  # a select missing in one piece of a cut tile: the held-out entries of the strip keep the unselected value
            if stage == "sources":
                held = np.zeros(a["mask"].shape, bool)
                held[8:12, 192:256] = a["mask"][8:12, 192:256] == 0
                assert held.any()
                a[which] = np.where(held, unselected(a)[0 if which == "P" else 1], a[which])
        return f

    def xst_off(stage, a):  # the [n][t] sentinel copy disagrees with the [t][n] one: its mask lies four columns off inside one 64-column block
        if stage == "sources":
            import masked_pq_mu_restatement as pm

            m = a["mask"].copy()
            m[:, 192:256] = a["mask"][:, 196:260]
            assert (m != a["mask"]).any()
            # (make_divergence_problem's data is clean under the mask too: the entries the shifted mask lets through are ordinary terms)
            a["P"], a["Q"] = pm.pq(a["X"], m, a["W"], a["H"], ep.pq_beta(a["form"]))

    out = {"strip_P": strip("P"), "double": double, "term": term, "lag" if family == "W" else "kpair": lag if family == "W" else kpair}
    if has_q:
        out.update(strip_Q=strip("Q"), pad=pad)
    if pq_masked:
        out.update(leak_Q=leak("Q"), leak_P=leak("P"))
        if family == "W":
            out.update(xst_off=xst_off)
    return out


# Which of the corruptions a Frobenius-relative 1e-4 on the updated factor -- the bar of every other divergence test -- passes on at
# least one (shape, form) here, measured by the test below (it asserts this very set).  On these three small shapes a strip, a lag
# over a chunk, a k pair over a tile, a doubled time row and the padding read all move the norm by more than 1e-4 as well (a strip is
# 4 of 70 ... 130 units); what the norm passes is the single term -- and, at the sizes the GPU test adds, everything confined to one
# tile: a 4 x 64 strip changes 4 of 2000 units by 2 of 210 terms (4e-4 of the norm at T = 6720, 5e-5 at config 2's T = 50000).  The
# element-wise check flags every one, at every size, because its bar is per element.
# The three damages of the sentinel families (leak_Q, leak_P, xst_off) touch a quarter of one strip's entries or of one block's columns.
# The norm passes leak_P even on these small shapes: the sentinel is -1 where observed data is 16 and more, so a P taken on it is a
# surplus term well below an ordinary term's size, in the sums of four units.  A leaked Q is a whole term and moves the norm by more
# than 1e-4 here, as xst_off does.
FROBENIUS_PASSES = {"term", "leak_P"}


def test_elementwise_check_flags_what_frobenius_passes():
    bars = ep.read_bars(BARS_FILE)["bar"]
    blind = set()
    for N, T, K, L in MUTATION_SHAPES:
        for family, names in (("W", "knl"), ("H", "kt")):
            for form in ep.FORMS:
                W, H, X, mask = ep.make_divergence_problem(N, T, K, L, family, relative=ep.FORMS[form][4])
                ref = ep.divergence_half(form, family, X, mask, W, H)
                assert ep.check_elementwise(ref["new"].astype(np.float32), ref["new"], bars[form], names) is None
                if ep.pq_masked(form):  # every 4 x 64 strip holds held-out entries, so leak_P and leak_Q damage something wherever the strip lies
                    strips = (mask[:N // 4 * 4, :T // 64 * 64] == 0).reshape(N // 4, 4, T // 64, 64)
                    assert strips.any(axis=(1, 3)).all()
                for name, corrupt in _corruptions(family, ref["Q"] is not None, ep.pq_masked(form)).items():
                    got = ep.divergence_half(form, family, X, mask, W, H, corrupt=corrupt)["new"].astype(np.float32)
                    msg = ep.check_elementwise(got, ref["new"], bars[form], names)
                    assert msg is not None and " at k=" in msg, (name, form, family, (N, T, K, L))
                    if np.linalg.norm(got - ref["new"]) / np.linalg.norm(ref["new"]) < 1e-4:
                        blind.add(name)
    print("a Frobenius-relative 1e-4 passes:", sorted(blind))
    assert blind == FROBENIUS_PASSES


def test_check_elementwise_reports_the_worst_element():
    ref = np.full((3, 4, 5), 2.0)
    got = ref.astype(np.float32)
    assert ep.check_elementwise(got, ref, 1e-6, "knl") is None
    got[1, 2, 3] *= 1.001
    got[2, 0, 0] *= 1.1
    msg = ep.check_elementwise(got, ref, 1e-6, "knl")
    assert "k=2, n=0, l=0" in msg and "2 elements" in msg and msg.startswith("rel 1.00e-01")
    got[0, 0, 0] = np.nan
    assert "k=0, n=0, l=0" in ep.check_elementwise(got, ref, 1e-6, "knl")


# ---- the masked MU rule and the PGD rule (tests/test_gpu_exact_masked_mu.py, tests/test_gpu_exact_pgd.py) ------------------------
PROFILE = os.path.join(ROOT, "profiles", "exact_masked_pgd.txt")
ULP_BAR = 2
SMALL_ROW, LARGEST_ROW = (70, 600, 20, 10), (2000, 6720, 32, 20)
TABLE_IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in ep.SHAPES]


def test_pgd_problem():
    N, T, K, L = 90, 610, 5, 7
    for family in ("W", "H"):
        W0, H0, _ = ep.make_problem(N, T, K, L, family)
        W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
        dense, dense0, other, other0 = (W, W0, H, H0) if family == "W" else (H, H0, W, W0)
        assert np.array_equal(dense, ep.PGD_SCALE * dense0) and np.array_equal(other, other0)
        r = X - oracle_conv(W, H)
        assert np.all(X == np.round(X)) and X.min() >= 0 and set(np.unique(r)) == set(range(-ep.PGD_R, ep.PGD_R + 1))
        assert 0.17 < (r == 0).mean() < 0.23  # sign(0) = 0 of the AbsoluteLoss store is exercised
        assert set(np.unique(mask)) == {0.0, 1.0, 2.0} and 0.2 < (mask == 0).mean() < 0.3 and 0.3 < (mask == 2).mean() < 0.45
        assert np.array_equal(mask[:, :608].reshape(N, -1, 8).min(axis=2), mask[:, :608].reshape(N, -1, 8).max(axis=2))  # blocks of 8
        m01 = ep.mu_mask(N, T)
        assert np.array_equal(m01, ep.make_divergence_problem(N, T, K, L, family)[3])
        holes = ep.holes_mask(N, T)
        assert not holes[N // 2].any() and not holes[:, T // 3].any() and holes.mean() > 0.7


@pytest.mark.parametrize("shape", [(70, 600, 20, 10), (90, 610, 5, 7), (30, 24, 32, 12)], ids=str)
def test_halves_are_the_references(shape):
    """pgd_half and masked_mu_half (the operations with the intermediate arrays kept) give the bits of the references the GPU tests
    compare with: the oracle's PGD rule and the masked restatement."""
    from oracle import cmf_oracle as oracle

    import masked_mu_restatement as mr

    N, T, K, L = shape
    for family in ("W", "H"):
        W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
        for variant in ep.PGD_VARIANTS:
            a = ep.pgd_half(variant, family, W, H, X, mask)
            ref, steps, loss = ep.pgd_oracle_half(oracle, variant, family, W, H, X, mask)
            assert np.array_equal(a["new"], ref), (variant, family)
            assert (steps[0] if family == "H" else steps[1]) == ep.STEP0 and (steps[1] if family == "H" else steps[0]) in (ep.STEP0 * 1.05, ep.STEP0 * 0.70)
            assert (loss is None) == (family == "W")
        W, H, X = ep.make_problem(N, T, K, L, family)
        for m in (ep.mu_mask(N, T), ep.holes_mask(N, T)):
            a = ep.masked_mu_half(family, W, H, X, m)
            Wr, Hr = W.copy(order="K"), H.copy(order="K")
            rule = mr.MaskedMult(X, m)
            if family == "W":
                mr.update_motifs(rule, Wr, Hr, l1W=ep.L1, l2W=ep.L2)
                assert np.array_equal(a["new"], Wr)
            else:
                mr.update_feature_maps(rule, Wr, Hr, l1H=ep.L1, l2H=ep.L2)
                assert np.array_equal(a["new"], Hr)


def _profile_rows():
    """{(rule, shape, family, variant): {key: value}} of the `row` lines of profiles/exact_masked_pgd.txt."""
    out = {}
    for line in open(PROFILE):
        f = line.split()
        if f and f[0] == "row":
            out[(f[1], f[2], f[3], f[4])] = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in f[5:]}
    return out


@pytest.mark.parametrize("N,T,K,L", [s[:4] for s in ep.SHAPES], ids=TABLE_IDS)
def test_pgd_preconditions_and_float32_model(N, T, K, L):
    """Every row, family and variant: the preconditions from the arrays generated (none is met by skipping a row), and the float32
    model of the half-step -- the exact integer gradient, alpha rounded to float32, product and difference in float32, fused and not --
    within 2 ulp of the fp64 half-step per element: the derivation of exact_problems' PGD section, confirmed.  The values are those
    profiles/exact_masked_pgd.txt records."""
    rows = _profile_rows()
    for family in ("W", "H"):
        W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
        r2 = (ep._conv(W, H) - X) ** 2
        assert ep.max_tile_sum(r2) <= ep.EXACT  # compute_loss() of the integer factors is exact
        for variant in ep.pgd_variants(N):
            what = f"{(N, T, K, L)} {family} {variant}"
            a = ep.pgd_half(variant, family, W, H, X, mask)
            b = ep.assert_pgd_preconditions(a, X, mask, what)
            assert b["loss_exact"], what
            worst = max(float(ep.ulps(ep.pgd_f32_model(a, fused), a["new"]).max()) for fused in (False, True))
            assert worst <= ULP_BAR, f"{what}: the float32 model is {worst:.2f} ulp from the fp64 half-step"
            rec = rows[("pgd", f"{N}x{T}x{K}x{L}", family, variant)]
            assert abs(rec["model_ulp"] - worst) <= 0.006 and abs(rec["units"] - b["units"]) <= 0.006 * b["units"], (what, rec, worst, b["units"])


def test_pgd_step_decisions_are_not_close_calls():
    """rule.steps is compared exactly: the loss after the half-step is far from the rule's first cur_loss (norm(data), pgd.jl:151), so
    a float32 loss takes the 1.05 / 0.70 decision the oracle takes.  (The five rows with N >= 1000: in the GPU test's own run.)"""
    from oracle import cmf_oracle as oracle

    for N, T, K, L in [s[:4] for s in ep.SHAPES if s[0] < 1000]:
        for family in ("W", "H"):
            W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
            for variant in ep.pgd_variants(N):
                Wc, Hc = W.copy(order="F"), H.copy(order="F")
                rule = oracle.PGDUpdate(X, Wc, Hc)
                loss, masked, penW, penH, nonneg = ep.PGD_VARIANTS[variant]
                kw = dict(nonneg=nonneg, mask=mask if masked else None, loss=loss)
                if family == "W":
                    oracle.pgd_update_motifs(rule, X, Wc, Hc, penaltiesW_sq=penW[0], penaltiesW_abs=penW[1], **kw)
                else:
                    oracle.pgd_update_feature_maps(rule, X, Wc, Hc, penaltiesH_sq=penH[0], penaltiesH_abs=penH[1], **kw)
                assert abs(rule.cur_loss - rule.datanorm) > 1e-3 * rule.datanorm, (N, T, K, L, family, variant, rule.cur_loss, rule.datanorm)


@pytest.mark.parametrize("N,T,K,L", [s[:4] for s in ep.SHAPES], ids=TABLE_IDS)
def test_masked_mu_preconditions(N, T, K, L):
    """assert_preconditions of tests/test_exact_parity.py on the MASKED sums, and every element keeps an observed term."""
    rows = _profile_rows()
    for family in ("W", "H"):
        W, H, X = ep.make_problem(N, T, K, L, family)
        a = ep.masked_mu_half(family, W, H, X, ep.mu_mask(N, T))
        seen = ep.assert_masked_mu_preconditions(a, f"{(N, T, K, L)} {family}")
        worst = float(ep.ulps(a["new"].astype(np.float32), a["new"]).max())
        assert worst <= 0.5
        rec = rows[("masked_mu", f"{N}x{T}x{K}x{L}", family, "mask")]
        assert rec["max_sum"] == max(a["num"].max(), a["den"].max()) and rec["min_observed"] == seen[seen > 0].min()
    if (N, T, K, L) == (130, 700, 32, 20):  # the holes: the unit's row of W and the sample's ... have no observed term
        W, H, X = ep.make_problem(N, T, K, L, "W")
        a = ep.masked_mu_half("W", W, H, X, ep.holes_mask(N, T))
        seen = ep.assert_masked_mu_preconditions(a, "holes", holes=True)
        assert np.all(a["new"][:, N // 2, :] == ep.EPS) and (a["new"] == ep.EPS).sum() == K * L == (seen == 0).sum()


def _pgd_mutations(a, X, mask):
    """name -> the change of G a seam error of the residual conv or of the contraction would make (pgd_half's arrays a)."""
    family, W, H, E = a["family"], a["W"], a["H"], a["E"]
    K, N, L = W.shape
    T = H.shape[1]
    masked = ep.PGD_VARIANTS[a["variant"]][1]
    out = {}
    dE = np.zeros((N, 64))
    dE[8:12] = -E[8:12, 192:256]  # a 4-row strip of one 64-column block of the residual never stored
    out["strip"] = ep.contract_cols(family, W, H, dE, 192)
    lag = min(L, T) - 1
    if family == "W":  # C2 loses its last lag over one time chunk
        d = np.zeros(W.shape)
        d[:, :, lag] = -(H[:, 128:384] @ E[:, 128 + lag:384 + lag].T)
        out["lag"] = d
    else:  # C3 loses one k pair of one 32-unit block over one 64-column tile
        d = np.zeros(H.shape)
        for l in range(min(L, T)):
            d[2:4, 64:128] -= W[2:4, :32, l] @ E[:32, 64 + l:128 + l]
        out["kpair"] = d
    out["double"] = ep.contract_cols(family, W, H, E[:, 300:301], 300)  # one time row counted twice
    if masked:
        raw = ep.pgd_sources(a["variant"].replace("_masked", "").replace("_free", ""), W, H, X, mask)[0][:64, 256:320]
        dE = np.zeros((N, 64))
        dE[:64] = raw * mask[:64, 264:328] - E[:64, 256:320]  # the mask tile read one 8-block off
        out["mask_shift"] = ep.contract_cols(family, W, H, dE, 256)
        dE = np.zeros((N, 64))
        dE[:64] = raw * (mask[:64, 256:320] != 0) - E[:64, 256:320]  # the weight read as a 0/1 flag
        out["mask_flag"] = ep.contract_cols(family, W, H, dE, 256)
    d = np.zeros(W.shape if family == "W" else H.shape)
    if family == "W":  # ONE term missing from ONE element
        k, n, l = 1, 5, 2
        t = [t for t in np.flatnonzero(H[k] != 0)[3:40] if E[n, t + l] != 0][0]
        d[k, n, l] = -H[k, t] * E[n, t + l]
    else:
        k, t = 1, 100
        n, l = [(n, l) for l in range(L) for n in np.flatnonzero(W[k, :, l] != 0) if E[n, t + l] != 0][0]
        d[k, t] = -W[k, n, l] * E[n, t + l]
    out["term"] = d
    return out


def _mu_mutations(a, X):
    """name -> (change of num, change of den) for masked_mu_half's arrays a."""
    family, W, H, M, Xm, est = a["family"], a["W"], a["H"], a["M"], a["Xm"], a["est"]
    K, N, L = W.shape
    T = H.shape[1]
    zero = np.zeros(W.shape if family == "W" else H.shape)
    out = {}
    dE = np.zeros((N, 64))
    dE[8:12] = -est[8:12, 192:256]
    out["strip"] = (zero, ep.contract_cols(family, W, H, dE, 192))
    lag = min(L, T) - 1
    if family == "W":
        d = np.zeros(W.shape)
        d[:, :, lag] = -(H[:, 128:384] @ Xm[:, 128 + lag:384 + lag].T)
        out["lag"] = (d, zero)
    else:
        d = np.zeros(H.shape)
        for l in range(min(L, T)):
            d[2:4, 64:128] -= W[2:4, :32, l] @ Xm[:32, 64 + l:128 + l]
        out["kpair"] = (d, zero)
    out["double"] = (ep.contract_cols(family, W, H, Xm[:, 300:301], 300), zero)
    conv = ep._conv(W, H)[:64, 256:320]
    shifted = M[:64, 264:328] != 0  # the mask tile read one 8-block off, for data and est alike
    dX, dEst = np.zeros((N, 64)), np.zeros((N, 64))
    dX[:64] = np.where(shifted, X[:64, 256:320], 0.0) - Xm[:64, 256:320]
    dEst[:64] = np.where(shifted, conv, 0.0) - est[:64, 256:320]
    out["mask_shift"] = (ep.contract_cols(family, W, H, dX, 256), ep.contract_cols(family, W, H, dEst, 256))
    dEst = np.zeros((N, 64))
    dEst[:64] = conv - est[:64, 256:320]  # the mask not read in one tile: est stored unmasked
    out["mask_unread"] = (zero, ep.contract_cols(family, W, H, dEst, 256))
    d = zero.copy()
    if family == "W":
        k, n, l = 1, 5, 2
        t = [t for t in np.flatnonzero(H[k] != 0)[3:40] if Xm[n, t + l] != 0][0]
        d[k, n, l] = -H[k, t] * Xm[n, t + l]
    else:
        k, t = 1, 100
        n, l = [(n, l) for l in range(L) for n in np.flatnonzero(W[k, :, l] != 0) if Xm[n, t + l] != 0][0]
        d[k, t] = -W[k, n, l] * Xm[n, t + l]
    out["term"] = (d, zero)
    return out


def _frob(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


# What a Frobenius-relative 1e-4 on the updated factor -- the bar of tests/test_gpu_masked_mu.py and of the PGD tests of
# tests/test_gpu_parity.py -- passes on the LARGEST row of the table, measured by the test below, which asserts these very sets.  PGD:
# every corruption confined to a tile, a chunk or a time row (a unit of G moves an element by alpha, 1e-4 of an entry).  Masked MU: the
# single term; a strip, a chunk, a tile or a time row still moves the norm by a few 1e-4 at T = 6720 and falls below the bar at config
# 2's T = 50000 (the comment at FROBENIUS_PASSES above).  The 2 ulp check flags every one on both rows.
NORMWISE_PASSES_ON_THE_LARGEST_ROW = {
    ("pgd", "W"): {"strip", "lag", "double", "mask_shift", "mask_flag", "term"},
    ("pgd", "H"): {"strip", "kpair", "double", "mask_shift", "mask_flag", "term"},
    ("masked_mu", "W"): {"term"},
    ("masked_mu", "H"): {"term"},
}


@pytest.mark.parametrize("shape", [SMALL_ROW, LARGEST_ROW], ids=str)
def test_two_ulp_check_flags_what_a_normwise_check_passes(shape):
    N, T, K, L = shape
    blind = {k: set() for k in NORMWISE_PASSES_ON_THE_LARGEST_ROW}
    for family, names in (("W", "knl"), ("H", "kt")):
        W, H, X, mask = ep.make_pgd_problem(N, T, K, L, family)
        for variant in ("square", "abs_masked"):
            a = ep.pgd_half(variant, family, W, H, X, mask)
            assert ep.ulps(ep.pgd_f32_model(a, False), a["new"]).max() <= ULP_BAR
            for name, dG in _pgd_mutations(a, X, mask).items():
                assert np.any(dG != 0), (name, variant, family)
                bad = ep.pgd_finish(dict(a, G=a["G"] + dG))
                got = ep.pgd_f32_model(bad, False)
                u = ep.ulps(got, a["new"])
                assert u.max() > ULP_BAR and ep.first_bad(u > ULP_BAR, names), (name, variant, family, shape, u.max())
                if _frob(got, a["new"]) < 1e-4:
                    blind[("pgd", family)].add(name)
        W, H, X = ep.make_problem(N, T, K, L, family)
        a = ep.masked_mu_half(family, W, H, X, ep.mu_mask(N, T))
        x = W if family == "W" else H
        for name, (dnum, dden) in _mu_mutations(a, X).items():
            assert np.any(dnum != 0) or np.any(dden != 0), (name, family)
            got = np.maximum(x * ((a["num"] + dnum) / ((((a["den"] + dden) + ep.L1) + (2.0 * ep.L2) * x) + ep.EPS)), ep.EPS).astype(np.float32)
            u = ep.ulps(got, a["new"])
            assert u.max() > ULP_BAR and ep.first_bad(u > ULP_BAR, names), (name, family, shape, u.max())
            if _frob(got, a["new"]) < 1e-4:
                blind[("masked_mu", family)].add(name)
    print("a Frobenius-relative 1e-4 passes:", {k: sorted(v) for k, v in blind.items()})
    if shape == LARGEST_ROW:
        assert blind == NORMWISE_PASSES_ON_THE_LARGEST_ROW


# ---- the HALS sweeps (tests/test_gpu_exact_hals.py) -----------------------------------------------------------------------------
HALS_PROFILE = os.path.join(ROOT, "profiles", "exact_hals.txt")
HALS_IDS = [f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in ep.HALS_SHAPES]
_hals_halves = {}


def _hals_half(shape, family, r):
    """(W, H, X, the fp64 half) of a row under the regulariser pair r, formed once per session."""
    key = (shape, family, r)
    if key not in _hals_halves:
        W, H, X = ep.make_hals_problem(*shape, family)
        _hals_halves[key] = (W, H, X, ep.hals_half(family, W, H, X, ep.HALS_REGS[r]))
    return _hals_halves[key]


def test_hals_launch_path_names_match_the_library():
    src = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_internal.h")).read()
    m = re.search(r"kHalsLaunchNames\[\] = \{(.*?)\};", src, re.S)
    assert m, "kHalsLaunchNames table not found"
    assert re.findall(r'"([^"]+)"', m.group(1)) == ep.HALS_LAUNCH_PATHS
    assert len(set(ep.HALS_LAUNCH_PATHS)) == len(ep.HALS_LAUNCH_PATHS) and not set(ep.HALS_LAUNCH_PATHS) & set(ep.LAUNCH_PATHS)
    m = re.search(r"kHalsNQ\[10\] = \{(.*?)\};", src)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == ep.HALS_NQ


def test_hals_plan_mirror_assigns_every_instance_to_a_row():
    """By the plan rules the table reaches every register instance of the W sweep (three of them with padding slots), the general W
    sweep by the plan and forced, one to four pullers per row, the stage pipeline at both lags over more than one segment, the general H
    sweep by the plan and forced, the chased form, and the T and L edges the sweeps treat separately; the GPU test confirms the plans
    with the launch counters."""
    plans = [(s[:4], cfg, ep.hals_plan(*s[:4], cfg)) for s in ep.HALS_SHAPES for cfg in s[4]]
    default = {shape: p for shape, cfg, p in plans if not cfg or set(cfg) == {"hals_chase"}}
    assert set(default) == {s[:4] for s in ep.HALS_SHAPES}
    assert {p["NQ"] for p in default.values() if p["NQ"]} == set(ep.HALS_NQ)
    padded = {(s[2], s[3]): (p["nq"], p["NQ"]) for s, p in default.items() if p["pad_slots"]}
    assert padded[(33, 3)] == (3, 4) and padded[(33, 31)] == (31, 32) and padded[(64, 18)] == (18, 20)
    assert default[(37, 1300, 64, 40)]["w_general"] and default[(9, 200, 3, 70)]["w_general"] and default[(9, 200, 3, 70)]["h_general"]
    forced_w = [s for s, cfg, p in plans if cfg.get("hals_general", 0) & 1 and not default[s]["w_general"]]
    forced_h = [s for s, cfg, p in plans if cfg.get("hals_general", 0) & 2 and not default[s]["h_general"]]
    assert len(set(forced_w)) >= 2 and len(set(forced_h)) >= 2
    assert {p["P"] for _, _, p in plans} == {0, 1, 2, 3, 4}
    assert {s[2] for s, _, p in plans if p["P"] > 0} >= {1, 2, 18, 64}
    assert any(p["P"] > p["nblk"] for _, _, p in plans), "no row with fewer blocks than pullers"
    stage = [(s, cfg) for s, cfg, p in plans if p["P"] == 0 and not p["h_general"]]
    assert {cfg.get("hals_lag", 2) for s, cfg in stage if s[1] > 256 and cfg.get("hals_seg") == 256} == {2, 3}
    chased = [(s, cfg, p) for s, cfg, p in plans if p["chase"]]
    assert [(s, cfg.get("hals_chase"), p["P"], p["chase"]) for s, cfg, p in chased] == [((130, 9000, 32, 20), 65, 3, 91)]
    past = {s for s, _, p in plans if not p["gram_window"]}  # the Gram form of P past its LDS window: from the residual under every hals_gram
    assert past == {(29, 1200, 129, 46)} and ep.rup(129, 32) * (64 + 2 * 45) * 4 > 96 * 1024 >= ep.rup(129, 32) * (64 + 2 * 44) * 4
    shapes = list(default)
    assert any(T < L for _, T, _, L in shapes) and any(L < T < 2 * L for _, T, _, L in shapes) and any(2 * L <= T <= 64 + L for _, T, _, L in shapes)
    assert any(T % 64 == 0 for _, T, _, _ in shapes) and any(T < 64 for _, T, _, _ in shapes) and {1, 64} <= {L for _, _, _, L in shapes}
    assert any(L >= 10 and p["P"] > 0 for (_, _, _, L), p in default.items())
    assert all(N % 2 == 1 for N, _, _, _ in shapes if N < 100)


@pytest.mark.parametrize("shape", [(12, 40, 3, 6), (9, 5, 2, 8), (9, 70, 5, 1), (20, 150, 7, 9)])
def test_hals_halves_are_the_sweeps(shape):
    """w_half / h_half in fp64 give w_sweep / h_sweep bit for bit on the integer problems (where the taps are exact), and on real-valued
    factors W bit for bit and H to the rounding of the taps' matrix product."""
    import hals_gram_form as hg
    from oracle import cmf_oracle as o

    for family in ("W", "H"):
        W, H, X = ep.make_problem(*shape, family)
        for reg in ep.HALS_REGS:
            np.testing.assert_array_equal(hg.w_half(o, W, H, X, *reg)["new"], hg.w_sweep(o, W, H, X, *reg))
            np.testing.assert_array_equal(hg.h_half(o, W, H, X, *reg)["new"], hg.h_sweep(o, W, H, X, *reg))
    N, T, K, L = shape
    rng = np.random.default_rng(3)
    W, H, X = rng.random((K, N, L)), rng.random((K, T)), rng.random((N, T))
    np.testing.assert_array_equal(hg.w_half(o, W, H, X, 0.1, 0.2)["new"], hg.w_sweep(o, W, H, X, 0.1, 0.2))
    b = hg.h_half(o, W, H, X, 0.1, 0.2)
    np.testing.assert_allclose(b["new"], hg.h_sweep(o, W, H, X, 0.1, 0.2), rtol=0, atol=1e-12)
    assert abs(b["loss"] - o.compute_loss(X, W, b["new"])) <= 1e-14


@pytest.mark.parametrize("N,T,K,L", [s[:4] for s in ep.HALS_SHAPES], ids=HALS_IDS)
def test_hals_preconditions_and_float32_model(N, T, K, L):
    """Every row, half and regulariser pair, from the arrays generated: every contraction below 2^24 in absolute sums, the shares of
    positive and clamped elements (also among the last L - 1 columns of H), the clamp decided away from the bar, and the float32
    model's distance from the fp64 half -- the values profiles/exact_hals.txt records, from which the bars are made."""
    prof = ep.read_hals_profile(HALS_PROFILE)["row"]
    bars = dict(zip("WH", ep.hals_bars(HALS_PROFILE)[:2]))
    for family in ("W", "H"):
        for r, reg in enumerate(ep.HALS_REGS):
            W, H, X, a = _hals_half((N, T, K, L), family, r)
            what = f"{(N, T, K, L)} {family} reg{r}"
            b = ep.hals_preconditions(family, a, bars[family])
            ep.assert_hals_preconditions(b, a["new"].size, L, what)
            m = ep.hals_half(family, W, H, X, reg, np.float32)
            model = float(ep.hals_units(m["new"], a).max())
            assert model <= bars[family] / ep.HALS_BAR_FACTOR * (1 + 1e-5), f"{what}: the model is {model:.2f} units from fp64: above a quarter of the bar"
            assert not (((m["new"] > 0) != (a["new"] > 0)) & ~ep.hals_excused(a, bars[family])).any(), f"{what}: the model's zero pattern differs outside the excused elements"
            rec = prof[(f"{N}x{T}x{K}x{L}", family, f"reg{r}")]
            assert abs(rec["model"] - model) <= 0.006 * max(model, 1.0), (what, rec["model"], model)
            b["zero_mismatch"] = int(((m["new"] > 0) != (a["new"] > 0)).sum())
            assert rec["abs_sum"] == b["abs_sum"] and rec["close"] == b["close"] and rec["zero_mismatch"] == b["zero_mismatch"], (what, rec, b)
            for key in ("pos", "clamp", "edge_pos", "edge_clamp"):
                assert (key in rec) == (key in b) and abs(rec.get(key, 0.0) - b.get(key, 0.0)) < 1e-5, (what, key, rec, b)
            assert abs(rec["min_pre"] - b["min_pre"]) <= 1e-4 * b["min_pre"], (what, rec["min_pre"], b["min_pre"])
            if family == "H":
                rel = abs(m["loss"] - a["loss"]) / a["loss"]
                assert rel <= ep.hals_bars(HALS_PROFILE)[2] / ep.HALS_BAR_FACTOR * (1 + 1e-6)
                assert abs(rec["loss_model"] - rel) <= 0.05 * rel + 1e-12, (what, rec["loss_model"], rel)


def test_hals_bars_are_made_from_the_profile_rows():
    """One bar per half: 4 times the worst float32-model error over the table, at least 8; the loss bar 4 times the worst relative error
    of the float32 conv model's loss (no floor).  The `bar` lines
    of the profile are these numbers, and there is a `row` line for every row, half and regulariser pair (and no other)."""
    prof = ep.read_hals_profile(HALS_PROFILE)
    want = {(f"{s[0]}x{s[1]}x{s[2]}x{s[3]}", f, f"reg{r}") for s in ep.HALS_SHAPES for f in "WH" for r in range(len(ep.HALS_REGS))}
    assert set(prof["row"]) == want
    bw, bh, bl = ep.hals_bars(HALS_PROFILE)
    for f, bar in (("W", bw), ("H", bh)):
        worst = max(v["model"] for k, v in prof["row"].items() if k[1] == f)
        assert bar == max(8.0, 4.0 * worst) and abs(prof["bar"][f] - bar) <= 1e-4 * bar
    assert bl == 4.0 * max(v["loss_model"] for k, v in prof["row"].items() if k[1] == "H")
    assert abs(prof["bar"]["loss"] - bl) <= 1e-4 * bl
    # no bar comes from a GPU result: the `gpu` lines are below the bars, and changing them changes nothing above
    for name, v in prof["gpu"].items():
        assert v <= (bl if name == "loss" else bw if name.startswith("W") else bh), (name, v)


# The local errors a sweep kernel would make, applied to the restatement through its corrupt hook; `None`: every row must have a site.
HALS_W_MUTATIONS = {"term": "L > 1", "stale_row": "K > 1, L > 1", "slot": "padding slots, L > 1"}
HALS_H_MUTATIONS = {"window": "L > 1", "push": "L > 1", "cross_interior": "K > 1, L > 1, more than two blocks", "cross_edge": "K > 1, L > 1"}


@pytest.mark.parametrize("N,T,K,L", [s[:4] for s in ep.HALS_SHAPES], ids=HALS_IDS)
def test_hals_check_flags_the_local_errors_of_a_sweep(N, T, K, L):
    """Each mutation moves the worst element by at least 4 bars on every row it applies to (under the regularisers (0.5, 0.25)): one
    G-update term of one step dropped, the HH row of step s used at step s + 1 for one unit, the last live slot's update dropped at one
    step where the instance has padding slots (W); one truncated window taken at full length, norm and taps, one cross-row term of one
    source row lost in an interior and in an edge block, one same-row push lost (H); l1 or l2 left out (both).  Where a mutation does
    not apply there is no such term: at L = 1 HH and the taps are diagonal (no step feeds a later one); with one component the HH rows of
    two consecutive steps agree on every column still to be swept; K = 1 has no cross-row term.

    NOT covered by any mutation here, said plainly: (1) the update of a PADDING slot of hals_w_sweep_reg_kernel.  A slot past L * K32
    has no column in the restatement: the kernel holds zeros there and multiplies them by the zeros its bounded loads return, so
    dropping that update changes no result and no CPU mutation can stand for it.  The `slot` mutation is a different error -- the last
    LIVE slot taken for padding at one step -- and what holds the padding slots themselves is the GPU file's element-wise check on the
    three rows that have them.  (2) eps left out moves NOTHING on any row, which is asserted: the squared norms are integers; where one
    is >= 1, eps = 2^-52 vanishes in the fp32 sum and moves the fp64 reference by 1e-16; where it is 0 the projection is exactly 0, the
    quotient is 0/0 or -l1/0 and fmaxf(., 0) makes both 0, as the reference does.  A kernel without eps passes the GPU file."""
    shape = (N, T, K, L)
    bw, bh, _ = ep.hals_bars(HALS_PROFILE)
    plan = ep.hals_plan(N, T, K, L)
    nblk = (T + 63) // 64
    applies = {"term": L > 1, "stale_row": L > 1 and K > 1, "slot": plan["pad_slots"] > 0 and L > 1, "window": L > 1, "push": L > 1,
               "cross_interior": K > 1 and L > 1 and nblk >= 3, "cross_edge": K > 1 and L > 1}
    for family, bar in (("W", bw), ("H", bh)):
        W, H, X, a = _hals_half(shape, family, 1)
        muts = ep.hals_w_mutations(a, plan) if family == "W" else ep.hals_h_mutations(a)
        for name in (HALS_W_MUTATIONS if family == "W" else HALS_H_MUTATIONS):
            if not applies[name]:
                continue
            assert name in muts, f"{shape} {family}: no site for the mutation {name!r}"
            moved = float(ep.hals_units(ep.hals_half(family, W, H, X, ep.HALS_REGS[1], corrupt=muts[name])["new"], a).max())
            assert moved >= 4 * bar, f"{shape} {family} {name}: moves the worst element by {moved:.0f} units only ({4 * bar:.0f} asked)"
        for name, reg in (("l1", (0.0, ep.L2)), ("l2", (ep.L1, 0.0))):
            moved = float(ep.hals_units(ep.hals_half(family, W, H, X, reg)["new"], a).max())
            assert moved >= 4 * bar, f"{shape} {family} {name} left out: moves the worst element by {moved:.0f} units only ({4 * bar:.0f} asked)"
        W, H, X, a = _hals_half(shape, family, 0)  # (l2 = 0: eps is all there is beside the norm)
        moved = float(ep.hals_units(ep.hals_half(family, W, H, X, ep.HALS_REGS[0], eps=0.0)["new"], a).max())
        assert moved < 1.0, f"{shape} {family}: eps left out moves an element by {moved:.2f} units"


def test_hals_check_reports_the_worst_element():
    W, H, X, a = _hals_half((9, 30, 2, 20), "H", 1)
    got = a["new"].astype(np.float32).astype(np.float64)
    assert ep.check_hals(got, a, 8.0, "kt")[1] is None
    i = tuple(np.argwhere(a["new"] > 0)[3])
    got[i] *= 1.0 + 1e-3
    worst, msg = ep.check_hals(got, a, 8.0, "kt", ["x"])
    assert worst > 1000 and msg.startswith(f"{worst:.1f} units (bar 8) at k={i[0]}, t={i[1]}: got ") and msg.endswith("; 1 elements over the bar); launches ['x']")
    got = a["new"].copy()
    j = tuple(np.argwhere((a["new"] == 0) & (a["diag"] != 0))[0])
    got[j] = 1e-30  # within any bar of 0, but not ON the clamp
    worst, msg = ep.check_hals(got, a, 8.0, "kt")
    assert worst < 1 and msg.startswith(f"zero pattern differs at k={j[0]}, t={j[1]}")


# ---- the plans for fewer compute units (tests/test_gpu_exact_cu_plans.py) ----------------------------------------------------------
def _claims(row, n_cu):
    """[(launch path, reached or not)] a row of CU_SHAPES is there for at its count, and what the mirrors say about each."""
    N, T, K, L, configs, why = row
    plan = ep.cu_plan(N, T, K, L, {}, n_cu)
    return [(w.lstrip("!"), not w.startswith("!"), plan.get(w.lstrip("!"))) for w in why]


def test_cu_plan_rows_take_the_branches_they_are_there_for():
    """From the mirrors alone: every row of CU_SHAPES reaches, at its count, the form its last entry claims; each of 128, 64 and 32 CUs
    reaches every count-dependent path; the candidate rows of the 32-CU table are the forms they were chosen for; and the same shapes
    take OTHER branches on the whole chip (which is why the whole-chip table cannot stand in for them)."""
    assert set(ep.CU_COUNTS) == {128, 64, 32, 1, 38} and all(n % 4 for n in ep.CU_COUNTS if n not in ep.CU_FULL)
    for n_cu in ep.CU_COUNTS:
        assert dict() in [c for row in ep.CU_SHAPES[n_cu] for c in row[4]]
        for row in ep.CU_SHAPES[n_cu]:
            assert row[4][0] == dict() and row[5], row  # (the claims are about the configuration without options)
            for path, want, got in _claims(row, n_cu):
                assert got is want, f"{row[:4]} at {n_cu} CUs: the row is there for {path} = {want}, the mirror says {got}"
            for family in ("W", "H"):
                b = ep.preconditions(*row[:4], family)
                assert b["exact"] and b["sensitive"] and b["loss_exact"], (row[:4], family, b)
        if n_cu not in ep.CU_FULL:
            assert max(r[0] * r[1] for r in ep.CU_SHAPES[n_cu]) <= 250 * 1500  # (1 and the odd count: the small rows only)
    assert max(r[0] * r[1] for n in ep.CU_COUNTS for r in ep.CU_SHAPES[n]) <= 1.15 * 500 * 12800
    for n_cu in ep.CU_FULL:
        reached = set()
        for N, T, K, L, configs, why in ep.CU_SHAPES[n_cu]:
            for cfg in configs:
                if "devices" in cfg:
                    if cfg.get("halo_in_allreduce") == 1 and K % 32 == 0 and T // len(cfg["devices"]) >= 2 * L:
                        reached.add("transconv_kernel:front_block")
                    continue
                reached |= {p for p, v in ep.cu_plan(N, T, K, L, cfg, n_cu).items() if v}
                if cfg.get("gram"):
                    reached |= {"gram_w_kernel", "gram_h_mfma_kernel"}
            if K > 16:
                reached.add("slab_sum_kernel:carry")  # (iterate(2) of the general kernels: the deferred loss rides on the slab sum)
        assert reached >= set(ep.CU_PATHS), (n_cu, sorted(set(ep.CU_PATHS) - reached))
        assert {r[:4] for r in ep.CU_SHAPES[n_cu] if r[2] == 32} >= {(130, 448, 32, 20), (130, 700, 32, 20)}
        plans = [ep.cu_plan(*r[:4], {}, n_cu) for r in ep.CU_SHAPES[n_cu] if r[2] > 16]
        assert {p["transconv_kernel:xcd"] for p in plans} == {True, False} and {p["hxt_kernel:tail"] for p in plans} == {True, False}
        small = [ep.cu_plan(*r[:4], {}, n_cu) for r in ep.CU_SHAPES[n_cu] if r[2] <= 16]
        assert {(p["g_gemm_fold_small_kernel<*>"], p["g_gemm_fold_small_kernel:split"]) for p in small} >= {(True, True), (True, False)}
    forms32 = {(130, 448): "pieces16", (130, 700): "pieces4", (250, 3200): "whole", (250, 6400): "whole+16", (250, 7040): "whole+4", (500, 12800): "whole+4"}
    for (N, T), form in forms32.items():
        assert ep.conv3_form(N, T, n_cu=32) == form and (N, T, 32, 20) in [r[:4] for r in ep.CU_SHAPES[32]]
    assert ep.conv3_cut(500, 12800, n_cu=32) == (1440, 160, 4) and 1600 // (12 * 32) >= 4  # four whole rounds and the extra cut
    assert ep.conv3_form(130, 700) == "pieces16" and ep.conv3_form(500, 12800) == "whole" and ep.conv3_form(250, 3200) == "pieces16"  # (256 CUs)
    assert ep.hxt_chunks(130, 700, 32, 20, n_cu=1) == (1, 690, 690) and ep.tc_plan(130, 700, 32, n_cu=1)[0] == 8  # the degenerate plan
    assert not ep.tc_plan(250, 1500, 32, n_cu=38)[2] and ep.tc_plan(250, 1500, 32, n_cu=38)[0] == 8 * 38 and ep.tc_plan(250, 1500, 32, n_cu=32)[2]
    assert {r[:4] for r in ep.CU_EPILOGUE_ROWS if r[2] == 32} == {(N, T, 32, 20) for (N, T) in forms32 if N < 500} and len(ep.CU_EPILOGUE_ROWS) == 7


def test_cu_plan_mirrors_restate_the_library_rules():
    """The constants the new mirrors share with cmf_api.hip plan(): a change there must be made here."""
    src = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_api.hip")).read()
    for text in ("const int wave_slots = 4 * n_cu * (best <= 5 ? 2 : 1);", "const int unit = 6 * best;", "(wave_slots + waves_per_chunk / 2) / waves_per_chunk",
                 "const long long W = std::min<long long>(8LL * n_cu, U);", "if (W >= 64 && W % 32 == 0) {", "h->sk_tc_ok = waves * h->sk3_NS >= 2LL * n_cu;"):
        assert text in src, text
    rules = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_rules.hip")).read()
    assert "if (h->n_cu % 8 != 0 || h->n_cu > 256) return 0;" in rules
    # the whole-chip values the library's comments state: T = 6250 over 8 chunks is 26 rotations + 10 rows (config 2's T / 8 shard)
    assert ep.hxt_chunks(2000, 6250, 32, 20) == (8, 780, 6240)
    assert ep.hxt_chunks(2000, 50000, 32, 20)[0] == 8 and ep.tc_plan(2000, 6250, 32)[0] == 2048


def test_cu_hals_rows_take_the_pipelines_they_are_there_for():
    rows = {s[:4] for s in ep.HALS_SHAPES}
    got = {}
    for n_cu, table in ep.CU_HALS_SHAPES.items():
        for N, T, K, L, configs in table:
            assert (N, T, K, L) in rows  # (the bars of profiles/exact_hals.txt are made from the rows of HALS_SHAPES)
            for cfg, P, chased in configs:
                plan = ep.hals_plan(N, T, K, L, cfg, n_cu=n_cu)
                assert (plan["P"], plan["chase"] > 0) == (P, chased), (n_cu, (N, T, K, L), cfg, plan)
                got.setdefault(n_cu, set()).add((P, chased))
    assert {p for n in (128, 64, 32) for p, _ in got[n]} >= {0, 2, 3, 4}
    assert (0, False) in got[64] and ep.hals_plan(37, 700, 32, 20, {}, n_cu=64)["P"] == 0 and ep.hals_plan(37, 700, 32, 20, {})["P"] == 4
    assert {p for p, _ in got[32]} >= {2, 3, 4}
    # the chased form with fewer CUs beside the pipeline than on the whole chip: 8 (16 - 12) = 32 at 128 CUs, 8 (32 - 16) = 128 at 256
    assert (2, True) in got[128] and 128 // 8 - (32 + 31 * 2 + 7) // 8 == 4 and 256 // 8 - (32 + 31 * 3 + 7) // 8 == 16
    # ... and off where the count is no multiple of 8, although every other condition holds as at 128
    assert got[134] == {(2, False)} and 134 // 8 - (32 + 31 * 2 + 7) // 8 >= 4 and got[38] == {(4, False)}


def test_two_ulp_check_sees_the_errors_a_replanned_chunking_could_make():
    """What a seam error of a plan for fewer CUs does to the W half of the row chosen for the tail rows at 32 CUs, (130, 481, 32, 20):
    8 chunks of 60 rows cover 480 rows and row 480 is left to the slab sum.  That one row lost, or every chunk one ring rotation (30
    rows) short, fails the 2 ulp bar by orders of magnitude -- and so does the bit-identity with the whole-chip plan."""
    N, T, K, L = 130, 481, 32, 20
    nch, clen, main = ep.hxt_chunks(N, T, K, L, n_cu=32)
    assert (nch, clen, main) == (8, 60, 480) and ep.hxt_chunks(N, T, K, L) != (nch, clen, main)
    W, H, X = ep.make_problem(N, T, K, L, "W")
    ref = _w_half(W, H, X)
    assert ep.ulps(ref.astype(np.float32), ref).max() <= 1
    tail = _w_half(W, H, X, drop_t=np.arange(main, T))
    short = _w_half(W, H, X, drop_t=np.concatenate([np.arange(c * clen + clen - 30, c * clen + clen) for c in range(nch)]))
    u_tail, u_short = ep.ulps(tail.astype(np.float32), ref), ep.ulps(short.astype(np.float32), ref)
    print(f"tail row lost: {u_tail.max():.0f} ulp on {(u_tail > 2).sum()} elements; chunks one rotation short: {u_short.max():.0f} ulp on {(u_short > 2).sum()} elements")
    assert u_tail.max() > 1000 and (u_tail > 2).sum() >= 0.9 * N  # (row 480's component: its lag-0 entry of every unit whose X there is not 0)
    assert u_short.max() > 1000 and (u_short > 2).mean() > 0.9


# ---- seqNMF's cross-orthogonality penalties (tests/test_gpu_exact_xortho.py) ---------------------------------------------------------
XO_SMALL_ROWS = [(70, 600, 20, 10), (90, 610, 5, 7), (30, 24, 32, 12), (37, 150, 33, 7), (17, 150, 16, 64)]
XO_ROWS = [s[:4] for s in ep.SHAPES] + [ep.XO_FOLD_ROW]
# the weakest terms of the table under XO_WEIGHTS, as the arrays give them (a unit of G; a unit of xW; an entry of numH in a window)
XO_WEAKEST = {((2000, 3000, 32, 20), "H"): ("G", 13), ((2000, 6720, 32, 20), "W"): ("xW", 19), ((70, 600, 20, 40), "H"): ("numH entry", 21),
              (ep.XO_FOLD_ROW, "H"): ("G", 17)}


@pytest.mark.parametrize("shape", XO_SMALL_ROWS, ids=str)
def test_xortho_half_is_the_restatements(shape):
    """xortho_half (the operations with the intermediate arrays kept) gives the bits of xortho_mu_restatement's update functions under
    all three weights and under each alone; the vectorised window sum is the restatement's loop bit for bit, on any input."""
    import xortho_mu_restatement as xr

    L = shape[3]
    noise = np.random.default_rng(7).random((shape[2], shape[1]))
    assert np.array_equal(ep.xo_smooth(noise, L), xr.smooth(noise, L))
    for family in ("W", "H"):
        W, H, X = ep.make_xortho_problem(*shape, family)
        assert set(np.unique(X)) == {0.0, 1.0, 2.0, 3.0}
        assert np.array_equal(ep.xo_smooth(H, L), xr.smooth(H, L))
        base = ep.xortho_half(family, X, W, H)
        for weights in ep.xo_weight_sets():
            a = ep.xortho_half(family, X, W, H, weights)
            b = ep.xortho_finish(base, weights)
            Wr, Hr = W.copy(order="F"), H.copy(order="F")
            if family == "W":
                xr.update_motifs(X, Wr, Hr, *weights, l1W=ep.L1, l2W=ep.L2)
                assert np.array_equal(a["new"], Wr) and np.array_equal(b["new"], Wr), (family, weights)
            else:
                loss = xr.update_feature_maps(X, Wr, Hr, *weights, l1H=ep.L1, l2H=ep.L2)
                assert np.array_equal(a["new"], Hr) and np.array_equal(b["new"], Hr) and a["loss"] == loss == b["loss"], (family, weights)
        xW, xH, G, oW = xr.terms(X, W, H)
        if family == "W":
            assert np.array_equal(base["xW"], xW) and np.array_equal(base["oW"], oW) and np.array_equal(base["G"], G)
        else:
            assert np.array_equal(base["xH"], xH) and np.array_equal(base["G"], G)


@pytest.mark.parametrize("N,T,K,L", XO_ROWS, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in XO_ROWS])
def test_xortho_preconditions(N, T, K, L):
    """Every row of the table and XO_FOLD_ROW, both families, all three weights and each alone, from the arrays generated: every table
    an integer table below 2^24, every stage of the denominator exact in float32, one unit of every sum at least 8 ulp."""
    shape = (N, T, K, L)
    for family in ("W", "H"):
        W, H, X = ep.make_xortho_problem(N, T, K, L, family)
        base = ep.xortho_half(family, X, W, H)
        for weights in ep.xo_weight_sets():
            a = ep.xortho_finish(base, weights, loss=False)
            p = ep.xortho_preconditions(a, f"{shape} {family} {weights}")
            if weights == ep.XO_WEIGHTS:
                assert float(ep.ulps(a["new"].astype(np.float32), a["new"]).max()) <= 0.5
                print(f"{shape} {family}: weakest {p['weakest'][0]} {p['weakest'][1]:.1f} ulp; " + ", ".join(f"{k} {v:.0f}" for k, v in p["ulp"].items()))
                if (shape, family) in XO_WEAKEST:
                    name, ulp = XO_WEAKEST[(shape, family)]
                    assert p["weakest"][0] == name and round(p["weakest"][1]) == ulp, (shape, family, p["weakest"])


def test_xortho_rows_and_configs():
    """XO_FOLD_ROW is the only row whose fold launch comes round twice (config 2 itself does not); xortho_configs drops exactly the
    refused configurations; at every CU count the penalised rows hold a tail the penalty contraction leaves and a C3 launch of more
    than one slab, and the count's own tail row."""
    passes = {s[:4]: ep.xo_fold_passes(ep.rup(s[2], 32), ep.rup(s[0], 128), s[3]) for s in ep.SHAPES}
    assert set(passes.values()) == {1} and ep.xo_fold_passes(32, 2048, 20) == 1
    N, T, K, L = ep.XO_FOLD_ROW
    assert ep.xo_fold_passes(ep.rup(K, 32), ep.rup(N, 128), L) == 2 and L * ep.rup(K, 32) * ep.rup(N, 128) // 4 == 532480 > ep.XO_FOLD_GRID == 524288
    for row in ep.SHAPES:
        kept = ep.xortho_configs(row[4])
        assert kept and kept[0] == row[4][0] and all("gram" not in c and "devices" not in c for c in kept)
        assert [c for c in row[4] if c not in kept] == [c for c in row[4] if "gram" in c or "devices" in c]
    for n in ep.CU_COUNTS:
        rows = ep.xo_cu_rows(n)
        ps = [ep.xo_cu_predicates(*row, n) for row in rows]
        assert any(p["left_tail"] for p in ps) and any(p["slabs"] > 1 for p in ps) and any(p["tail"] for p in ps), (n, ps)
        assert [r[:4] for r in ep.CU_SHAPES[n] if "hxt_kernel:tail" in r[5]][0] in rows
        assert all(K > 16 for _, _, K, _ in rows)


XO_MUTATIONS = {"W": {"window_short_lo", "window_short_hi", "window_seam", "S_first_column", "S_last_column", "off_one_component", "off_with_itself",
                      "G_of_the_previous_H", "tail_reads_H", "oW_first_lag_only"},
                "H": {"window_short_lo", "window_short_hi", "window_seam", "S_first_column", "S_last_column", "off_one_component", "off_with_itself",
                      "G_of_the_previous_H", "slab_lost_before_the_window", "lambda_and_lambda_H_exchanged"}}


@pytest.mark.parametrize("shape", [(70, 600, 20, 10), (90, 610, 5, 7), (37, 150, 33, 7), (1001, 2500, 32, 20)], ids=str)
def test_two_ulp_check_flags_the_local_errors_of_the_penalties(shape):
    """Every mutation of xortho_half -- a window one row short at either end, a lost first or last column of S, a window cut at a
    64-column seam, a component or a 32-block of components missing from off, off with the component itself, G of the previous H, a C3
    slab that never reached the window's table, a chunk tail contracted with H in G's place, lambda and lambda_H exchanged, oW at the
    first lag only -- fails the 2 ulp check at some element by at least four bars.  The Frobenius-relative error beside it is printed
    and not asserted: what a norm-wise 1e-4 would have made of the same fault."""
    for family, names in (("W", "knl"), ("H", "kt")):
        W, H, X = ep.make_xortho_problem(*shape, family)
        a = ep.xortho_half(family, X, W, H)
        assert ep.ulps(a["new"].astype(np.float32), a["new"]).max() <= 0.5
        muts = ep.xortho_mutations(family, a)
        assert set(muts) == XO_MUTATIONS[family] | ({"off_one_k_block"} if shape[2] > 32 else set()), (family, sorted(muts))
        for name, corrupt in muts.items():
            bad = ep.xortho_half(family, X, W, H, corrupt=corrupt)
            got = bad["new"].astype(np.float32)
            u = ep.ulps(got, a["new"])
            print(f"{shape} {family} {name}: {u.max():.0f} ulp at {ep.first_bad(u == u.max(), names)}, {int((u > ULP_BAR).sum())} of {u.size} elements over the bar; "
                  f"Frobenius-relative {_frob(got, a['new']):.2e}")
            assert u.max() >= 4 * ULP_BAR, (shape, family, name, u.max())
