"""seqNMF's significance test of components on the GPU (cmf_null_moments, evaluate_significance) against tests/significance_restatement.py.

EXACT PROBLEMS.  X holds hashed integers in {0..3} and W hashed integers in {0, 1, 2}: every overlap is an integer below 2^24, so the fp32
contraction is exact in any order, and T' vmax^3 < 2^53 (asserted from the arrays) makes the fp64 power sums exact in any order as well.
cmf_null_moments must then equal the restatement BIT FOR BIT on every draw 0 .. 12: a wrong shift, a shift per component instead of per
unit, a zero fill instead of the wrap, a lost t block or a column read from the neighbouring draw moves a sum by at least 1
(tests/test_significance_cpu.py shows it for each on these very problems).  Shapes (N, T', K, L):
    (6, 5, 3, 8)        T' < L
    (7, 130, 1, 1)      K = 1 and L = 1
    (13, 300, 5, 7)     N no multiple of 8, six draws per column block, three t blocks with a tail
    (40, 257, 33, 20)   a draw straddling column blocks, a t tail of one column
    (24, 200, 32, 33)   the second lag block
    (130, 700, 16, 20)  a mid-sized shape
On two of them the result is bitwise the same under signif_batch 1, 3 and the default, as one call of 13 draws and as calls of 5 + 8, and
on handles planned for 1, 38 and 256 CUs.  A second W uploaded with cmf_set_factors is what the next call reads, and a fit continued
after a call gives the bits it gives without it (the plain rule, and under lambda_xortho).

REAL-VALUED DATA.  The planted-sequence problem of the CPU test and a gen_synthetic split with W from a 30-iteration fit on the device:
skew and skewnull within the bar of profiles/significance_precision.txt of the restatement, pvals, is_significant and excluded exactly
equal (every null lies at least 4 x bar from the component's own skewness: asserted here from the arrays), the moments bitwise the same
under two batch sizes.
"""
import ctypes
import os

import numpy as np
import pytest

import significance_restatement as sr
from test_significance_cpu import read_bar

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 4
DRAWS = sr.EXACT_DRAWS
SEED = sr.EXACT_SEED
_refs = {}


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def reference(shape, which=0):
    """(W, X, the restatement's sums of draws 0 .. 12), once per problem; the exactness precondition asserted from the arrays."""
    if (shape, which) not in _refs:
        W, X = sr.exact_problem(shape, which)
        sums = sr.null_moments(W, X, SEED, range(DRAWS))
        sr.assert_exact_precondition(W, X, sums)
        _refs[(shape, which)] = (W, X, sums)
    return _refs[(shape, which)]


def make_rule(cmf, W, X, n_cu=None):
    H = np.zeros((W.shape[0], X.shape[1]), order="F")
    if n_cu is None:
        return cmf.MultUpdate(X, W, H)
    old = {k: os.environ.get(k) for k in ("CMF_TEST_HOOKS", "CMF_TEST_N_CU")}
    os.environ["CMF_TEST_HOOKS"] = "1"
    os.environ["CMF_TEST_N_CU"] = str(n_cu)
    try:
        rule = cmf.MultUpdate(X, W, H)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        assert rule.counter("plan:n_cu") == n_cu
    except BaseException:
        rule.close()
        raise
    return rule


def same_bits(a, b, what):
    bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} of {a.size} sums differ, first (moment, component, draw) {tuple(bad[0])}: {a[tuple(bad[0])]!r} against {b[tuple(bad[0])]!r}"


IDS = ["x".join(map(str, s)) for s in sr.EXACT_SHAPES]


@pytest.mark.parametrize("shape", sr.EXACT_SHAPES, ids=IDS)
def test_exact_moments_equal_the_restatement_bit_for_bit(cmf, shape):
    W, X, want = reference(shape)
    rule = make_rule(cmf, W, X)
    try:
        before = rule.counter("signif_launches")
        got = rule.null_moments(SEED, 0, DRAWS)
        assert rule.counter("signif_launches") > before
    finally:
        rule.close()
    assert got.shape == (3, shape[2], DRAWS)
    same_bits(got, want, f"{shape}")


CUT_SHAPES = [(13, 300, 5, 7), (40, 257, 33, 20)]


@pytest.mark.parametrize("shape", CUT_SHAPES, ids=["x".join(map(str, s)) for s in CUT_SHAPES])
def test_result_is_independent_of_batch_calls_and_cu_plan(cmf, shape):
    W, X, want = reference(shape)
    rule = make_rule(cmf, W, X)
    try:
        for batch in (1, 3, 0):
            rule.set_option("signif_batch", batch)
            same_bits(rule.null_moments(SEED, 0, DRAWS), want, f"{shape} signif_batch {batch}")
        for batch in (0, 3):
            rule.set_option("signif_batch", batch)
            two = np.concatenate([rule.null_moments(SEED, 0, 5), rule.null_moments(SEED, 5, DRAWS - 5)], axis=2)
            same_bits(two, want, f"{shape} as calls of 5 + 8 draws, signif_batch {batch}")
    finally:
        rule.close()
    for n_cu in (1, 38, 256):
        rule = make_rule(cmf, W, X, n_cu)
        try:
            same_bits(rule.null_moments(SEED, 0, DRAWS), want, f"{shape} planned for {n_cu} CUs")
        finally:
            rule.close()


def test_a_second_W_is_what_the_next_call_reads(cmf):
    shape = (13, 300, 5, 7)
    W, X, want = reference(shape)
    W2, _, want2 = reference(shape, 1)
    assert not np.array_equal(W, W2) and not np.array_equal(want, want2)
    rule = make_rule(cmf, W, X)
    try:
        same_bits(rule.null_moments(SEED, 0, DRAWS), want, "first W")
        rule.upload(W2, np.zeros((shape[2], shape[1]), order="F"))
        same_bits(rule.null_moments(SEED, 0, DRAWS), want2, "second W")
    finally:
        rule.close()


@pytest.mark.parametrize("xortho", [0.0, 0.01], ids=["plain", "lambda_xortho"])
def test_a_fit_continued_after_the_call_gives_the_same_bits(cmf, xortho):
    N, T, K, L = 40, 600, 5, 10
    X = np.asfortranarray(sr.hashed_ints(3, 1, (N, T), 1000) / 1000.0)
    W0 = np.asfortranarray(0.1 + sr.hashed_ints(3, 2, (K, N, L), 1000) / 1000.0)
    H0 = np.asfortranarray(0.1 + sr.hashed_ints(3, 3, (K, T), 1000) / 1000.0)

    def run(with_calls):
        rule = cmf.MultUpdate(X, W0, H0)
        try:
            if xortho:
                rule.set_xortho(xortho)
            out = []
            if with_calls:
                rule.null_moments(SEED, 0, 3)
            out.append(rule.iterate(3).copy())
            if with_calls:
                rule.null_moments(SEED, 2, 70)  # (more than one batch)
            out.append(rule.iterate(3).copy())
            return out, rule.download()
        finally:
            rule.close()

    (la, (Wa, Ha)), (lb, (Wb, Hb)) = run(True), run(False)
    for a, b, what in ((la[0], lb[0], "losses of the first three iterations"), (la[1], lb[1], "losses of the next three"), (Wa, Wb, "W"), (Ha, Hb, "H")):
        assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), what
    assert np.all(np.isfinite(la[0])) and np.all(np.isfinite(la[1])) and not np.array_equal(la[0], la[1])


def test_refusals(cmf):
    lib = cmf.load_library()
    shape = (13, 300, 5, 7)
    N, T, K, L = shape
    W, X, want = reference(shape)

    def refused(rule, code):
        with pytest.raises(cmf.CMFError) as ei:
            rule.null_moments(SEED, 0, 2)
        assert ei.value.code == code, ei.value

    rule = make_rule(cmf, W, X)
    try:
        for bad in ((0, 0), (-1, 1)):  # (first_draw, n_draws)
            with pytest.raises(cmf.CMFError) as ei:
                rule.null_moments(SEED, *bad)
            assert ei.value.code == ERR_ARG
        assert lib.cmf_null_moments(rule._h, SEED, 0, 1, None) == ERR_ARG
        mask = np.asfortranarray((sr.hashed_ints(5, 1, (N, T), 4) > 0).astype(np.float64))
        rule.set_mask(mask)
        refused(rule, ERR_STATE)
        rule.set_mask(None)
        same_bits(rule.null_moments(SEED, 0, DRAWS), want, "after the mask was taken away")
        assert lib.cmf_set_mask(rule._h, cmf.host.ptr(mask)) == 0  # the PGD entries' mask
        refused(rule, ERR_STATE)
        assert lib.cmf_set_mask(rule._h, None) == 0
        same_bits(rule.null_moments(SEED, 0, DRAWS), want, "after the PGD mask was taken away")
        with pytest.raises(cmf.CMFError) as ei:
            rule.set_option("signif_batch", -1)
        assert ei.value.code == ERR_ARG
    finally:
        rule.close()
    group = cmf.MultUpdate(X, W, np.zeros((K, T), order="F"), devices=[0, 0])
    try:
        refused(group, ERR_UNSUPPORTED)
    finally:
        group.close()
    h = ctypes.c_void_p()
    assert lib.cmf_create(ctypes.byref(h), 0, N, T, K, L, cmf.host.ptr(X)) == 0
    try:
        sums = np.zeros((3, K, 2), order="F")
        assert lib.cmf_null_moments(h, SEED, 0, 2, cmf.host.ptr(sums)) == ERR_STATE
        assert "factors" in lib.cmf_last_error().decode()
    finally:
        lib.cmf_destroy(h)


# ---- real-valued data ----------------------------------------------------------------------------------------------------------------
def check_real(cmf, name, W, X, seed, nnull):
    bar = read_bar()
    T = X.shape[1]
    want = sr.decide(W, sr.null_moments(W, X, seed, range(1 + nnull)), T)
    gap = float(np.nanmin(np.abs(want["skewnull"] - want["skew"][:, None])))
    assert gap >= 4 * bar, f"{name}: a null lies {gap} from the component's own skewness, the bar is {bar}"
    got = cmf.evaluate_significance(W, X, p=0.05, nnull=nnull, seed=seed)
    err = max(float(np.abs(got.skew - want["skew"]).max()), float(np.abs(got.skewnull - want["skewnull"]).max()))
    print(f"{name}: largest skewness error {err:.3g} (bar {bar:g}), closest null {gap:.3g}, pvals {got.pvals}, significant {got.is_significant}")
    assert err <= bar
    assert np.array_equal(got.pvals, want["pvals"])
    assert np.array_equal(got.is_significant, want["is_significant"])
    assert np.array_equal(got.excluded, want["excluded"])
    rule = make_rule(cmf, W, X)
    try:
        a = rule.null_moments(seed, 0, 1 + nnull)
        rule.set_option("signif_batch", 7)
        b = rule.null_moments(seed, 0, 1 + nnull)
    finally:
        rule.close()
    same_bits(a, b, f"{name}: default batch against signif_batch 7")
    return got


def test_planted_sequences_on_the_device(cmf):
    W, X = sr.planted_problem()
    got = check_real(cmf, "planted", W, X, sr.PLANTED_SEED, sr.PLANTED_NNULL)
    assert list(got.is_significant) == [True, True, False]


def test_synthetic_split_fitted_on_the_device(cmf):
    N, Tt, K, L = sr.SPLIT_SHAPE
    data = cmf.gen_synthetic(N=N, T=sr.SPLIT_T, K=3, L=L, seed=sr.SPLIT_SEED)
    train, test = np.asfortranarray(data[:, : sr.SPLIT_T - Tt]), np.asfortranarray(data[:, sr.SPLIT_T - Tt :])
    r = cmf.fit_cnmf(train, L=L, K=K, alg=":mult", max_itr=sr.SPLIT_ITERS, seed=sr.SPLIT_SEED, check_convergence=False)
    W = np.asfortranarray(r.W)
    assert W.shape == (K, N, L) and np.all(np.isfinite(W))
    got = check_real(cmf, "split", W, test, sr.SPLIT_SEED, sr.default_nnull(K, 0.05))
    res = cmf.evaluate_significance(r, test, seed=sr.SPLIT_SEED)  # a CNMF_results and the default nnull = 2 ceil(K / p)
    assert res.nnull == 200 and np.array_equal(res.pvals, got.pvals)
