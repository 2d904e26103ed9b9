"""seqNMF's significance test of components, the parts that need no GPU: the shift table of the library (cmf_null_shifts) against the
restatement (tests/significance_restatement.py), the refusals that come before any device work, the restatement's own arithmetic
(raw-sum skewness against the two-pass form, the exclusion rules, the planted-sequence decision), the condition the real-valued GPU test
relies on, and five mutations of the restatement, each of which moves a power sum on the exact problems of tests/test_gpu_significance.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import significance_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 4


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    return m


def read_bar():
    text = open(os.path.join(ROOT, "profiles", "significance_precision.txt")).read()
    return float(re.search(r"^bar skew (\S+)\s*$", text, re.M).group(1))


# ---- the shift table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,L", [(5, 13, 7), (33, 40, 20), (1, 7, 1), (3, 6, 8), (7, 11, 4096), (32, 24, 33)])
def test_null_shifts_equal_the_restatement(cmf, K, N, L):
    seed = 0x1234_5678_9ABC_DEF0 + K
    got = cmf.null_shifts(seed, 9, K, N, L)
    want = sr.null_shifts(seed, range(9), K, N, L)
    assert got.shape == (N, K, 9) and got.dtype == np.int32
    assert np.array_equal(got, want)
    assert not got[:, :, 0].any(), "draw 0 is the identity"
    assert got.min() >= 0 and got.max() < L
    if L == 1:
        assert not got.any()
    if L == 4096:  # (bits >> 32) * L needs 44 bits: a 32-bit product would wrap
        assert got.max() > 2048
    if L > 1:
        assert got[:, :, 1:].any()
    # a range of draws cut differently, and far-away draws (the counter is a 64-bit product)
    later = cmf.null_shifts(seed, [4, 5, 6], K, N, L)
    assert np.array_equal(later, got[:, :, 4:7])
    far = cmf.null_shifts(seed, [3, 2**40], K, N, L)
    assert np.array_equal(far, sr.null_shifts(seed, [3, 2**40], K, N, L))


def test_null_shifts_differ_per_unit_and_per_component(cmf):
    s = cmf.null_shifts(11, 40, 5, 13, 7)[:, :, 1:]
    assert any(len(set(s[:, k, d])) > 1 for k in range(5) for d in range(39)), "one shift per component"
    assert any(len(set(s[n, :, d])) > 1 for n in range(13) for d in range(39))
    counts = np.bincount(s.ravel(), minlength=7)
    assert counts.min() > 0.7 * s.size / 7 and counts.max() < 1.3 * s.size / 7, counts


def test_refusals_without_a_device(cmf):
    lib = cmf.load_library()
    buf = (ctypes.c_int32 * 64)()
    ok = lambda **kw: dict(dict(seed=1, first=0, n=1, K=2, N=3, L=4, out=buf), **kw)
    call = lambda a: lib.cmf_null_shifts(a["seed"], a["first"], a["n"], a["K"], a["N"], a["L"], a["out"])
    assert call(ok()) == 0
    for bad in (dict(out=None), dict(n=0), dict(first=-1), dict(K=0), dict(N=0), dict(L=0), dict(L=4097)):
        assert call(ok(**bad)) == ERR_ARG, bad
        assert "cmf_null_shifts" in lib.cmf_last_error().decode()
    sums = (ctypes.c_double * 8)()
    assert lib.cmf_null_moments(None, 1, 0, 1, sums) == ERR_ARG
    assert {"cmf_null_shifts", "cmf_null_moments"} <= set(cmf.SYMBOLS)
    names = ctypes.create_string_buffer(4096)
    assert lib.cmf_option_names(names, 4096) == 0 and b"signif_batch" not in names.value


# ---- the restatement's own arithmetic -------------------------------------------------------------------------------------------------
def test_raw_sum_skewness_equals_the_two_pass_form():
    W, X = sr.planted_problem()
    K, N, L = W.shape
    worst = 0.0
    for d in range(6):
        Wd = sr.null_motif(W, sr.null_shifts(sr.PLANTED_SEED, [d], K, N, L)[:, :, 0])
        v = sr.transconv(Wd, X)
        raw, _ = sr.skew_from_sums(sr.power_sums(v), X.shape[1])
        worst = max(worst, float(np.abs(raw - sr.skew_two_pass(v)).max()))
    print("raw-sum against two-pass skewness:", worst)
    assert worst <= 1e-12
    for shape in sr.EXACT_SHAPES[2:]:
        W, X = sr.exact_problem(shape)
        v = sr.transconv(W, X)
        raw, _ = sr.skew_from_sums(sr.power_sums(v), X.shape[1])
        assert np.abs(raw - sr.skew_two_pass(v)).max() <= 1e-12, shape


def test_transconv_drops_terms_beyond_the_last_column(oracle):
    W, X = sr.exact_problem((13, 300, 5, 7))
    assert np.array_equal(sr.transconv(W, X), oracle.tensor_transconv(W, X))
    W, X = sr.exact_problem((6, 5, 3, 8))  # T' < L
    assert np.array_equal(sr.transconv(W, X), oracle.brute_transconv(W, X))
    # seqNMF's helper wraps circularly: the same on data followed by L zero columns
    K, N, L = W.shape
    Xz = np.concatenate([X, np.zeros((N, L))], axis=1)
    T = Xz.shape[1]
    wrap = np.zeros((K, T))
    for l in range(L):
        wrap += W[:, :, l] @ np.roll(Xz, -l, axis=1)
    assert np.array_equal(wrap[:, : X.shape[1]], sr.transconv(W, X))


def planted_sums():
    W, X = sr.planted_problem()
    return W, X, sr.null_moments(W, X, sr.PLANTED_SEED, range(1 + sr.PLANTED_NNULL))


@pytest.fixture(scope="module")
def planted():
    return planted_sums()


def test_exclusion_rules_each_alone(planted):
    W, X, sums = planted
    T = X.shape[1]
    base = sr.decide(W, sums, T)
    assert not base["excluded"].any()
    # every entry at or below the MU floor
    W1 = W.copy()
    W1[2] = sr.EPS
    s1 = sums.copy()
    s1[:, 2, :] = sr.null_moments(W1, X, sr.PLANTED_SEED, [0])[:, 2, :]
    r = sr.decide(W1, s1, T)
    assert list(r["excluded"]) == [False, False, True] and np.isinf(r["pvals"][2]) and not r["is_significant"][2]
    W1[2, 3, 1] = 2 * sr.EPS  # one entry above the floor: the rule no longer applies (the one-unit rule does: tested below)
    assert not (W1.reshape(3, -1).max(axis=1) <= sr.EPS)[2]
    # one unit carrying the motif
    W2 = W.copy()
    W2[1] = 1e-6
    W2[1, 20, :] = 1.0
    r = sr.decide(W2, sums, T)
    assert list(r["excluded"]) == [False, True, False] and np.isinf(r["pvals"][1])
    W2[1, 21, :] = 0.1  # 0.01 / 1.01 of the squared mass elsewhere: kept
    assert not sr.decide(W2, sums, T)["excluded"][1]
    # the component's own overlap has no variance (MATLAB: NaN, then "significant")
    s3 = sums.copy()
    s3[:, 0, 0] = (T * 2.0, T * 4.0, T * 8.0)
    r = sr.decide(W, s3, T)
    assert list(r["excluded"]) == [True, False, False] and np.isnan(r["skew"][0]) and not r["is_significant"][0]
    # the decision divides p by the components KEPT
    assert r["is_significant"][1] == (r["pvals"][1] <= 0.05 / 2)
    # a NaN null compares false
    s4 = sums.copy()
    s4[:, 1, 5] = (T * 2.0, T * 4.0, T * 8.0)
    assert sr.decide(W, s4, T)["pvals"][1] <= base["pvals"][1]


def test_planted_sequences_are_significant_and_the_unstructured_component_is_not(planted, cmf):
    W, X, sums = planted
    r = sr.decide(W, sums, X.shape[1], p=0.05)
    print("planted pvals", r["pvals"], "skew", r["skew"])
    assert r["pvals"][0] == 1 / sr.PLANTED_NNULL and r["pvals"][1] == 1 / sr.PLANTED_NNULL
    assert list(r["is_significant"]) == [True, True, False]
    assert r["pvals"][2] > 0.05
    assert sr.default_nnull(3, 0.05) == 120 and sr.default_nnull(32, 0.05) == 1280
    # the host half of the package on the same sums: the same decision, value for value
    h = cmf.significance_from_sums(W, sums, X.shape[1], p=0.05)
    assert np.array_equal(h.pvals, r["pvals"]) and np.array_equal(h.is_significant, r["is_significant"])
    assert np.array_equal(h.excluded, r["excluded"]) and np.array_equal(h.skew, r["skew"]) and np.array_equal(h.skewnull, r["skewnull"])


def test_real_valued_inputs_keep_every_null_away_from_the_own_skewness(planted, oracle):
    """What the real-valued GPU test relies on: a device error of at most the bar cannot flip a comparison skewnull > skew.  (The GPU
    test fits the split on the device and asserts the same from its own arrays.)"""
    bar = read_bar()
    W, X, sums = planted
    Ws, Xs = sr.split_problem(oracle)
    assert Ws.shape == (5, 40, 10) and Xs.shape == (40, 600)
    for name, (W, X, sums) in (("planted", planted), ("split", (Ws, Xs, sr.null_moments(Ws, Xs, sr.SPLIT_SEED, range(1 + sr.default_nnull(5, 0.05)))))):
        r = sr.decide(W, sums, X.shape[1])
        gap = float(np.nanmin(np.abs(r["skewnull"] - r["skew"][:, None])))
        print(name, "closest null:", gap, "bar", bar, "pvals", r["pvals"], "significant", r["is_significant"])
        assert gap >= 4 * bar, name


def test_fp32_contraction_stays_within_the_bar(planted):
    W, X, sums = planted
    bar = read_bar()
    s32 = sr.null_moments(W, X, sr.PLANTED_SEED, range(1 + sr.PLANTED_NNULL), contraction=np.float32)
    a, _ = sr.skew_from_sums(s32, X.shape[1])
    b, _ = sr.skew_from_sums(sums, X.shape[1])
    assert np.abs(a - b).max() <= bar / 8 * 1.0000001


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
def mutation_is_identity_by_construction(shape, mutation, draws):
    """L = 1 has no shift to get wrong (every draw is the identity), and a mutation of the shifts or of which draw a column reads changes
    nothing there; K = 1 packs one column per draw, so no draw of draws 0 .. 12 lies behind a 32-column seam."""
    N, T, K, L = shape
    if L == 1 and mutation != "last_block_lost":
        return True
    if mutation == "seam_next_draw" and not any(d * K + k >= 32 and (d * K + k) % 32 <= k for d in draws for k in range(K)):
        return True
    return False


@pytest.mark.parametrize("mutation", sr.MUTATIONS)
@pytest.mark.parametrize("shape", sr.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_each_mutation_moves_a_power_sum_on_the_exact_problems(shape, mutation):
    W, X = sr.exact_problem(shape)
    draws = range(sr.EXACT_DRAWS)
    want = sr.null_moments(W, X, sr.EXACT_SEED, draws)
    sr.assert_exact_precondition(W, X, want)
    got = sr.null_moments(W, X, sr.EXACT_SEED, draws, mutation=mutation)
    if mutation_is_identity_by_construction(shape, mutation, draws):
        assert np.array_equal(got, want)
        return
    assert not np.array_equal(got, want), f"{mutation} is invisible on {shape}"
    assert np.array_equal(got[:, :, 0], want[:, :, 0]) or mutation in ("last_block_lost", "seam_next_draw")


def test_shift_table_header_is_free_of_hip_and_clean_under_sanitizers(tmp_path):
    """cmf.jl_amd/csrc/cmf_signif.h's first part needs no HIP: tests/signif_shifts_driver.cpp (its own main) drives it under ASan and UBSan."""
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "signif_shifts_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "cmf.jl_amd", "csrc"), os.path.join(ROOT, "tests", "signif_shifts_driver.cpp"), "-o", exe])
    for seed, first, n, K, N, L in ((5, 0, 9, 5, 13, 7), (2**63 + 11, 3, 4, 33, 40, 4096), (1, 0, 2, 1, 7, 1), (9, 2**40, 2, 3, 6, 8)):
        p = subprocess.run([exe] + [str(v) for v in (seed, first, n, K, N, L)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-500:] + p.stderr
        assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
        lines = p.stdout.split()
        got = np.array(lines[:-2], dtype=np.int64).reshape(n, K, N).transpose(2, 1, 0)
        assert np.array_equal(got, sr.null_shifts(seed, range(first, first + n), K, N, L))
        m = 32 // np.gcd(K, 32)
        assert lines[-2:] == ["batch", str(m * -(-256 // (K * m)))]
    for bad in ((1, -1, 1, 2, 3, 4), (1, 0, 0, 2, 3, 4), (1, 0, 1, 0, 3, 4), (1, 0, 1, 2, 0, 4), (1, 0, 1, 2, 3, 0), (1, 0, 1, 2, 3, 4097)):
        p = subprocess.run([exe] + [str(v) for v in bad], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.strip() == "refused", (bad, p.stdout, p.stderr)
