"""seqNMF's re-centring of motifs, the parts that need no GPU: the library's shift decision (cmf_recentre_shifts, and the HIP-free
csrc/cmf_recentre.h under sanitizers) against the restatement (tests/recentre_restatement.py) on the stated cases, properties of the
definition, five mutations of the restatement, each of which fails the exact comparison on a stated case, the numpy recentre(W, H), and the
refusals that come before any device work.
"""
import ctypes
import os

import numpy as np
import pytest

import recentre_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
CASES = rr.shift_cases()


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    return m


def lib_shifts(cmf, W):
    lib = cmf.load_library()
    Wf = np.asfortranarray(W, dtype=np.float64)
    K, N, L = Wf.shape
    s = np.full(K, -99, dtype=np.int32)
    rc = lib.cmf_recentre_shifts(Wf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), K, N, L, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0, lib.cmf_last_error()
    return s


def some_H(K, T, L, seed=3):
    """Integer-valued H whose outer L columns are at the floor."""
    H = np.random.default_rng(seed).integers(1, 9, size=(K, T)).astype(np.float64)
    H[:, :L] = H[:, T - L:] = rr.EPS
    return H


# ---- the decision --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_library_shifts_equal_the_restatement(cmf, name):
    W, expect = CASES[name]
    want = rr.shifts(W)
    if expect is not None:
        assert np.array_equal(want, expect), "the restatement against the case's closed form"
    assert np.array_equal(lib_shifts(cmf, W), want)
    L = W.shape[2]
    assert np.abs(want).max() <= max(L - 1, 0)
    if name == "K33":
        assert len(set(want.tolist())) > 2, "components decide for themselves"


def test_shift_arguments_are_checked(cmf):
    lib = cmf.load_library()
    W = np.ones((2, 3, 4), order="F")
    s = np.zeros(2, dtype=np.int32)
    pw, ps = W.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for args in ((None, 2, 3, 4, ps), (pw, 2, 3, 4, None), (pw, 0, 3, 4, ps), (pw, 2, 0, 4, ps), (pw, 2, 3, 0, ps)):
        assert lib.cmf_recentre_shifts(*args) == ERR_ARG
        assert b"cmf_recentre_shifts" in lib.cmf_last_error()
    assert lib.cmf_abi_version() == 6
    for sym in ("cmf_recentre_shifts", "cmf_recentre", "cmf_mu_set_recentre", "cmf_mu_recentre_info"):
        assert sym in cmf.SYMBOLS and hasattr(lib, sym)


def test_non_finite_and_huge_ratios_are_safe(cmf):
    W = np.zeros((3, 2, 6))
    W[0, 0, 2] = np.inf
    W[1, 0, 0], W[1, 1, 5] = -1.0, 1.0 + 2.0**-20  # m0 tiny, m1 / m0 beyond 2^20
    W[2, 0, 3] = np.nan
    got = lib_shifts(cmf, W)
    assert np.array_equal(got, rr.shifts(W))
    assert got[0] == 0 and got[2] == 0 and got[1] < -6


# ---- properties of the definition ----------------------------------------------------------------------------------------------------
def middle_problem(K=3, N=4, L=9, T=60):
    """Motifs whose support lies in the middle lags with room to move, H whose outer L columns are at the floor."""
    rng = np.random.default_rng(8)
    W = np.full((K, N, L), rr.EPS)
    for k, lag in enumerate((2, 5, 6)[:K]):
        W[k, :, lag] = rng.integers(1, 9, size=N)
        W[k, :, lag - 1] = rng.integers(1, 5, size=N)
    return W, some_H(K, T, L)


def test_est_is_unchanged_when_nothing_leaves_the_window_or_the_recording():
    W, H = middle_problem()
    W2, H2, s = rr.recentre(W, H)
    assert s.any()
    est, est2 = rr.orc.tensor_conv(W, H), rr.orc.tensor_conv(W2, H2)
    # the two differ only in products with a floor-valued factor: at most K L of them per entry, each below eps max(W, H)
    K, N, L = W.shape
    assert np.abs(est2 - est).max() <= 4 * rr.EPS * K * L * (W.max() + H.max())
    assert est.max() > 1.0


def test_a_second_step_is_a_no_op_when_no_mass_was_lost():
    W, H = middle_problem()
    W2, H2, s = rr.recentre(W, H)
    W3, H3, s3 = rr.recentre(W2, H2)
    assert s.any() and not s3.any()
    assert np.array_equal(W3, W2) and np.array_equal(H3, H2)


def test_fill_and_circular_forms_agree_when_the_ends_of_H_are_at_the_floor():
    W, H = middle_problem()
    a = rr.recentre(W, H)
    b = rr.recentre(W, H, circular_H=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    H[:, 0] = 7.0  # ... and not otherwise: what leaves the recording comes back at the other end
    assert not np.array_equal(rr.recentre(W, H)[1], rr.recentre(W, H, circular_H=True)[1])


def test_vacated_entries_take_the_clamp_floor():
    W, _ = CASES["ends_L8"]
    H = some_H(2, 6, 1)  # T < L: a shift can empty a row of H
    H[:] = 3.0
    W2, H2, s = rr.recentre(W, H)
    assert list(s) == [3, -4]
    assert np.array_equal(W2[0, :, :3], np.full((3, 3), rr.EPS)) and np.array_equal(W2[0, :, 3], W[0, :, 0])
    assert np.array_equal(H2[0, 3:], np.full(3, rr.EPS)) and np.array_equal(H2[0, :3], H[0, 3:])
    assert np.array_equal(H2[1, :4], np.full(4, rr.EPS)) and np.array_equal(H2[1, 4:], H[1, :2])
    assert H2.min() == rr.EPS


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
MUTATION_CASE = {"h_same_way": "ends_L8", "w_wrapped": "ends_L7", "zero_based_m1": "ends_L8", "rounded": "integer_ratio", "no_dead_rule": "dead_L7"}


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_each_mutation_fails_the_exact_comparison(mutation):
    W, _ = CASES[MUTATION_CASE[mutation]]
    K, N, L = W.shape
    H = some_H(K, 40, L)
    want = rr.recentre(W, H)
    got = rr.recentre(W, H, mutation=mutation)
    assert not all(np.array_equal(a, b) for a, b in zip(got, want)), f"{mutation} is invisible on {MUTATION_CASE[mutation]}"
    if mutation == "no_dead_rule":  # ... and at even L the uniform dead motif stays where it is either way
        We, _ = CASES["dead_L8"]
        assert not rr.shifts(We, mutation=mutation).any()
        assert list(rr.shifts(W, mutation=mutation)) == [-1, -1], "a uniform dead motif at odd L walks one lag per step"


# ---- the host side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K33", "ends_L7", "integer_ratio", "m0_zero", "L1"])
def test_numpy_recentre_equals_the_restatement(cmf, name):
    W, _ = CASES[name]
    K, N, L = W.shape
    H = some_H(K, 30, min(L, 5), seed=5)
    W2, H2, s = cmf.recentre(W, H)
    want = rr.recentre(W, H)
    assert s.dtype == np.int32 and np.array_equal(s, want[2])
    assert np.array_equal(W2, want[0]) and np.array_equal(H2, want[1])


def test_host_refusals_name_their_reason(cmf):
    data = np.abs(np.random.default_rng(0).normal(size=(6, 40)))
    for kw, word in ((dict(alg=":hals"), "alg=:mult"), (dict(alg=":pgd"), "alg=:mult"), (dict(alg=":admm"), "alg=:mult"), (dict(alg=cmf.ANLSUpdate), "alg=:mult"),
                     (dict(alg=":sep"), "alg=:mult"), (dict(alg=":mult", devices=[0, 0]), "shards"), (dict(alg=":mult", options={"gram": 1}), "Gram")):
        with pytest.raises(NotImplementedError, match=word):
            cmf.fit_cnmf(data, L=4, K=2, max_itr=2, shift=True, **kw)
    events = cmf.EventData.from_dense(np.round(data)) if hasattr(cmf.EventData, "from_dense") else None
    if events is not None:
        with pytest.raises(NotImplementedError, match="event data"):
            cmf.fit_cnmf(events, L=4, K=2, max_itr=2, alg=":mult", divergence=":kl", shift=True)
    assert "shift" in cmf.host._KNOWN_KW


def test_the_sources_are_in_the_build_list_and_the_digest():
    import importlib.util

    spec = importlib.util.spec_from_file_location("cmf_build", os.path.join(ROOT, "cmf.jl_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    base = {os.path.basename(p) for p in build.DEPS}
    assert {"cmf_recentre.hip", "cmf_recentre.h"} <= base and any(p.endswith("cmf_recentre.hip") for p in build.SOURCES)


def test_decision_header_is_free_of_hip_and_clean_under_sanitizers(tmp_path):
    """cmf.jl_amd/csrc/cmf_recentre.h needs no HIP: tests/recentre_shift_driver.cpp (its own main) drives it under ASan and UBSan."""
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "recentre_shift_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "cmf.jl_amd", "csrc"), os.path.join(ROOT, "tests", "recentre_shift_driver.cpp"), "-o", exe])
    extra = np.zeros((2, 2, 6))
    extra[0, 0, 0], extra[0, 1, 5] = -1.0, 1.0 + 2.0**-40  # c beyond the cap: no overflow of the int32
    extra[1, 0, 2] = np.inf
    for name, W in [(n, c[0]) for n, c in sorted(CASES.items())] + [("huge", extra)]:
        K, N, L = W.shape
        path = tmp_path / f"{name}.txt"
        path.write_text(f"{K} {N} {L}\n" + "\n".join(float(v).hex() for v in np.asfortranarray(W).ravel(order="F")) + "\n")
        p = subprocess.run([exe, str(path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-500:] + p.stderr
        assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
        assert np.array_equal(np.array(p.stdout.split(), dtype=np.int64), rr.shifts(W)), name
    bad = tmp_path / "bad.txt"
    bad.write_text("0 3 4\n")
    p = subprocess.run([exe, str(bad)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "refused", (p.stdout, p.stderr)
