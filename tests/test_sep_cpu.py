"""CPU checks of the separable fit (src/algs/separable.jl): the restatement tests/sep_restatement.py against itself (its two modes,
the parallel form of findsetmax, planted data), the conditions every GPU test input must meet (check_problem), the host-side
decisions of cmf.jl_amd/host.py against the restatement's, and the surface (alg=":sep", the C entries, the Julia binding)."""
import ctypes
import os
import re

import numpy as np
import pytest

import anls_restatement as A
import sep_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cmf_sep_prepare", "cmf_sep_gram", "cmf_sep_spa", "cmf_sep_nnls", "cmf_sep_shift_table", "cmf_sep_construct")


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build(quiet=True)
    import cmf_jl_amd as m

    return m


def adversarial(th):
    n = 200
    yield "ascending by 0.6 thresh", 1.0 + 0.6 * th * np.arange(n)
    yield "descending by 0.6 thresh", 1.0 - 0.6 * th * np.arange(n)
    yield "all equal", np.full(n, 0.25)
    yield "a record at every element", 1.0 + 3.0 * th * np.arange(n)
    yield "records just under the band", 1.0 + 0.999 * th * np.arange(n)
    yield "one element", np.array([0.5])
    yield "saw", 1.0 + th * np.tile([0.0, 0.7, 1.4, -0.9], 50)


def test_findsetmax_parallel_form_is_the_sequential_scan():
    th = S.SQRT_EPS
    for name, x in adversarial(th):
        assert S.findsetmax_records(x) == S.findsetmax(x), name
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(1, 400))
        x = rng.random(n) if trial % 3 else 1.0 + th * rng.integers(-4, 5, n) * 0.6  # (many elements near the band's edges)
        assert S.findsetmax_records(x) == S.findsetmax(x), trial
        big = 0.05  # a wide band: sets of many members
        assert S.findsetmax_records(x, big) == S.findsetmax(x, big), trial


@pytest.mark.parametrize("pre", [None, ":svd", ":svdcond"])
def test_noise_free_data_gives_back_the_planted_factors(pre):
    data, tW, tH, K, L, thresh = S.case_data("ref_clean")
    assert S.is_separable(tH, L)
    out = {}
    W, H = S.fit(data, K, L, thresh=thresh, pre=pre, out=out)
    Gtrue = A.shift_and_stack(tH, L)  # row l*K + k
    for v in out["vertices"]:  # every vertex is a pure column: exactly one (k, l) is active in it
        assert (Gtrue[:, v] != 0).sum() == 1, v
    active = [int(np.flatnonzero(Gtrue[:, v])[0]) for v in out["vertices"]]
    assert sorted(active) == list(range(K * L))  # and every (k, l) is found
    for g in out["groups"]:  # every group is one component, its rows in the order of the lags
        assert len({active[r] % K for r in g}) == 1 and [active[r] // K for r in g] == list(range(L)), g
    perm = S.permute_factors(tH, H)
    assert S.cos_score(tH, H[perm]) > 0.99
    assert np.allclose(S.row_normalize(H).sum(axis=1), 1.0)


CHECKED = [("ref_clean", None, False), ("ref_clean", ":svd", False), ("ref_clean", ":svdcond", False), ("ref_noisy", None, False),
           ("ref_noisy", ":svd", False), ("ref_noisy", ":svdcond", False), ("ref_noisy", None, True), ("k1", None, False), ("l1", None, False),
           ("r128", None, False), ("t_prime", None, False), (S.FIG + (0.1, None, 1), None, False)]


@pytest.mark.parametrize("case,pre,spectral", CHECKED, ids=lambda v: "fig" if isinstance(v, tuple) else str(v))
def test_every_gpu_input_meets_the_conditions(case, pre, spectral):
    """check_problem: the modes agree (decisions identical, values within 1e-10), every decision margin is >= 1e-6 in both,
    tol = 1e-8 and 1e-12 end on the same passive sets."""
    data, tW, tH, K, L, thresh = S.case_data(case)
    noise = (S.CASES[case] if case in S.CASES else case)[4]
    ol, orw, floors, margins = S.check_problem(str(case), data, K, L, noise_free=(noise == 0), thresh=thresh, pre=pre, spectral=spectral)
    print({k: f"{min(v):.2e}" for k, v in margins["rewritten"].items()}, {k: f"{v:.1e}" for k, v in floors.items()})
    if noise == 0:
        assert "spa_col2" in margins["rewritten"]  # the tie case: the tie-break has decided
    else:
        assert "spa_col2" not in margins["rewritten"]  # the no-tie case


def test_host_decisions_are_the_restatements(cmf):
    """The grouping and sorting that host.py does on the shift table, against the restatement's on the same table."""
    from cmf_jl_amd import host

    for case, spectral in (("ref_noisy", False), ("ref_noisy", True), ("ref_clean", False), ("t_prime", False)):
        data, tW, tH, K, L, thresh = S.case_data(case)
        out = {}
        S.fit(data, K, L, thresh=thresh, spectral=spectral, out=out)
        P, head = out["P"], out["head"]

        class Shape:
            pass

        shape = Shape()
        shape.K, shape.L = K, L
        assert host.Separable.cluster(shape, P, head, spectral=spectral) == out["groups"], case
    assert host.cos_score(tH, out["H0"]) == S.cos_score(tH, out["H0"])
    assert host.permute_factors(tH, out["H0"]) == S.permute_factors(tH, out["H0"])
    assert np.array_equal(host.row_normalize(tH), S.row_normalize(tH))
    assert host.is_separable(tH, L) and not host.is_separable(np.ones((2, 30)), 3)


def test_construct_divisor_is_the_references():
    """separable.jl:77 divides by min(T, t+L) - t + 1: L + 1 away from the end, the number of terms in the last L columns."""
    G = np.ones((3, 10))
    W, H = S.construct_WH(np.eye(4, 3), G, [[0, 1, 2]])
    assert np.allclose(H[0, :7], 3 / 4) and np.allclose(H[0, 7:], [1.0, 1.0, 1.0])


def test_sep_resolves_and_fit_cnmf_takes_its_keywords(cmf):
    import warnings

    from cmf_jl_amd.host import _KNOWN_KW, _resolve_alg

    assert _resolve_alg(":sep") is cmf.Separable and _resolve_alg("sep") is cmf.Separable
    assert {"thresh", "refit_H", "refit_W", "refit_H_itr", "spectral", "pre"} <= _KNOWN_KW
    with pytest.raises(NotImplementedError):
        _resolve_alg(":anls")  # (stays as it was)
    if cmf.load_library().cmf_device_count() > 0:
        pytest.skip("a GPU is present")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(cmf.CMFError) as ei:  # no fallback: without a device the fit fails in the library
            cmf.fit_cnmf(np.ones((6, 40)) + np.eye(6, 40), L=2, K=2, alg=":sep", thresh=0.1, pre=":svdcond")
    assert ei.value.code == 2


def test_library_exports_the_entries_and_refuses_null_handles(cmf):
    lib = ctypes.CDLL(cmf.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in cmf.SYMBOLS
    lib.cmf_last_error.restype = ctypes.c_char_p
    x = (ctypes.c_double * 4)()
    v = (ctypes.c_int64 * 4)()
    assert lib.cmf_sep_prepare(None, x) == 1
    assert lib.cmf_sep_gram(None, ctypes.c_double(0.0), x) == 1
    assert lib.cmf_sep_spa(None, ctypes.c_int64(1), ctypes.c_double(0.0), 0, None, v) == 1
    assert lib.cmf_sep_nnls(None, v, ctypes.c_int64(1), x, x) == 1
    assert lib.cmf_sep_shift_table(None, x, ctypes.c_int64(1), ctypes.c_int64(1), x, x) == 1
    assert lib.cmf_sep_construct(None, x, x, v, x, x) == 1
    assert b"NULL" in lib.cmf_last_error()
    assert lib.cmf_abi_version() == 6  # the entries are additive


def test_header_binding_and_digest_cover_the_new_unit(cmf):
    hdr = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    for name in ENTRIES:
        block = hdr[hdr.rindex("/*", 0, hdr.index(f"int {name}(")):hdr.index(f"int {name}(")]
        assert "separable.jl:" in block, name
    assert '"sep_nnls_exchanges"' in hdr
    jl = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert "module HIPSeparable" in jl and re.search(r"function fit\(data, K, L; thresh=0, verbose=false, refit_H=false, refit_W=false, refit_H_itr=10", jl)
    for name in ENTRIES:
        assert f"(:{name}, LIBCMF)" in jl, name
    build = __import__("importlib").import_module(cmf.__name__ + ".build")
    names = [os.path.basename(p) for p in build.DEPS]
    assert "cmf_sep.hip" in names and "cmf_sep.h" in names
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integ for n in ENTRIES + ("HIPSeparable",))


def test_golden_fixture_is_the_restatements_answer():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fit_sep_n100_t250.npz"))
    case = tuple(int(v) if float(v).is_integer() and i != 4 else float(v) for i, v in enumerate(z["case"]))
    data, tW, tH, K, L, thresh = S.case_data(case[:5] + (None, int(case[6])))
    assert float(z["thresh"]) == thresh
    out = {}
    W, H = S.fit(data, K, L, thresh=thresh, pre=":svdcond", out=out)
    assert out["vertices"] == z["vertices"].tolist() and out["groups"] == z["groups"].tolist()
    assert A.rel(W, z["W"]) <= 1e-12 and A.rel(H, z["H"]) <= 1e-12
    assert abs(float(z["loss"]) - np.linalg.norm(A.conv(W, H) - data) / np.linalg.norm(data)) <= 1e-12
