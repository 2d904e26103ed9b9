"""CPU checks of the ANLS rule (src/algs/anls.jl): the fp64 restatement's two modes agree, its block-pivoting solver agrees
with an independent one and satisfies the KKT conditions, each half step is a descent step, and the rule is wired through every
layer (header, binding, Python, Julia)."""
import ctypes
import os
import re

import numpy as np
import pytest

import anls_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_literal_and_gram_modes_agree_and_tol_cannot_matter(case):
    """Every shape the GPU tests use: literal vs Gram mode <= 1e-10 with identical zero patterns, at most 1 % near-degenerate
    entries, and the same passive sets with tol = 1e-5 and tol = 1e-12 (values within the bar of the shape)."""
    N, T, K, L, steps, variants = R.CASES[case]
    data, W0, H0 = R.problem(N, T, K, L, seed=sorted(R.CASES).index(case))
    W = W0
    if "w" in steps:
        sl, sg = {}, {}
        Wl, W = R.update_motifs(data, H0, L, mode="literal", stats=sl), R.update_motifs(data, H0, L, stats=sg)
        R.check_step(case, Wl, W, sl, sg, R.update_motifs(data, H0, L, tol=1e-12), R.bar(R.rel(Wl, W), 1e-8))
        assert sg["exchanges"] > 0
    for v in variants:
        sl, sg = {}, {}
        Hl, ll = R.update_feature_maps(data, W, H0, variant=v, mode="literal", stats=sl)
        Hg, lg = R.update_feature_maps(data, W, H0, variant=v, stats=sg)
        R.check_step(case, Hl, Hg, sl, sg, R.update_feature_maps(data, W, H0, variant=v, tol=1e-12)[0], R.bar(R.rel(Hl, Hg), 1e-8))
        assert abs(ll - lg) <= 1e-10
        assert np.array_equal(H0, R.problem(N, T, K, L, seed=sorted(R.CASES).index(case))[2])  # the caller's H is not edited


def kkt(G, C, X, Y, tol):
    assert (X >= 0).all()
    Yfull = G @ X - C
    assert (Yfull >= -tol - 1e-9 * np.abs(C).max()).all()
    assert np.abs(X * Yfull).max() <= 1e-9 * max(1.0, np.abs(C).max() * np.abs(X).max())
    assert np.abs((Yfull - Y)[X == 0]).max(initial=0.0) <= 1e-9 * np.abs(C).max()


@pytest.mark.parametrize("backup_only", [False, True])
@pytest.mark.parametrize("n,rows,m,dead", [(5, 30, 40, 0), (28, 200, 12, 0), (100, 400, 6, 0), (12, 60, 20, 3)])
def test_block_pivoting_against_lawson_hanson_and_kkt(n, rows, m, dead, backup_only):
    """Random problems, and problems that are rank-deficient by all-zero columns of A (`dead`: their unknowns stay zero)."""
    nnls = pytest.importorskip("scipy.optimize").nnls
    rng = np.random.default_rng(n + m)
    A = rng.random((rows, n))
    if dead:
        A[:, rng.choice(n, dead, replace=False)] = 0.0
    B = A @ (rng.random((n, m)) * (rng.random((n, m)) < 0.5)) + 0.3 * rng.standard_normal((rows, m))
    G, C = A.T @ A, A.T @ B
    st = {}
    X, Y = R.nnls_bpp(G, C, backup_only=backup_only, stats=st)
    assert st["capped"] == 0 and st["exchanges"] >= m and (st["backup"] > 0) == backup_only
    kkt(G, C, X, Y, R.NNLS_TOL)
    Xs = np.stack([nnls(A, B[:, j])[0] for j in range(m)], axis=1)
    assert R.rel(X, Xs) <= 1e-10, R.rel(X, Xs)
    assert (X[np.abs(G).sum(axis=0) == 0] == 0).all()
    for j in range(min(m, 3)):  # the one-column solver of the sequential sweep is the same solver
        s1 = [0, 0, 0]
        x1, y1 = R._bpp1(G, C[:, j], R.NNLS_TOL, backup_only, s1)
        assert np.array_equal(x1 > 0, X[:, j] > 0) and R.rel(x1, X[:, j]) <= 1e-12 and s1[2] == 0


@pytest.mark.parametrize("variant", ["basic", "block"])
def test_every_half_step_is_a_descent_step(variant):
    N, T, K, L = 20, 260, 4, 6
    data, W, H = R.problem(N, T, K, L, seed=5)
    dn = np.linalg.norm(data)
    loss = np.linalg.norm(R.conv(W, H) - data) / dn
    for _ in range(10):
        W = R.update_motifs(data, H, L)
        lw = np.linalg.norm(R.conv(W, H) - data) / dn
        assert lw <= loss + 1e-12, (lw, loss)
        H, lh = R.update_feature_maps(data, W, H, variant=variant)
        assert lh <= lw + 1e-12, (lh, lw)
        loss = lh
    W2, H2, hist = R.fit(data, *R.problem(N, T, K, L, seed=5)[1:], 10, variant=variant)
    assert len(hist) == 11 and (np.diff(hist) <= 1e-12).all() and hist[-1] == loss


def test_the_fixture_is_what_the_restatement_gives():
    g = np.load(os.path.join(ROOT, "tests", "golden", "fit_anls_n40_t600_10.npz"))
    for v in ("basic", "block"):
        W, H, hist = R.fit(g["data"], g["W_init"], g["H_init"], 10, variant=v)
        assert R.rel(W, g[f"W_{v}"]) <= 1e-12 and R.rel(H, g[f"H_{v}"]) <= 1e-12
        assert np.abs(hist - g[f"loss_hist_{v}"]).max() <= 1e-12
        assert g[f"nearW_{v}"].sum() <= 0.01 * W.size and g[f"nearH_{v}"].sum() <= 0.01 * H.size
        assert 0 < float(g[f"floor_{v}"]) <= 1e-10


def test_block_variant_needs_t_ge_l_and_names_are_checked():
    data, W, H = R.problem(8, 5, 2, 6, seed=3)
    with pytest.raises(ValueError, match="T >= L"):
        R.update_feature_maps(data, W, H, variant="block")
    R.update_feature_maps(data, W, H, variant=":basic")
    with pytest.raises(ValueError):
        R.update_feature_maps(data, W, H, variant="comb")


def test_the_rule_is_selected_by_type_and_the_name_still_raises():
    import cmf_jl_amd as cmf
    from cmf_jl_amd.host import _KNOWN_KW, _resolve_alg

    assert _resolve_alg(cmf.ANLSUpdate) is cmf.ANLSUpdate and cmf.HIPANLSUpdate is cmf.ANLSUpdate
    assert issubclass(cmf.ANLSUpdate, cmf.AbstractCFUpdate)
    assert "variant" in _KNOWN_KW
    with pytest.raises(NotImplementedError, match="alg=ANLSUpdate"):
        _resolve_alg(":anls")
    assert [cmf.ANLSUpdate._variant(v) for v in ("basic", ":basic", "block", ":block")] == [0, 0, 1, 1]
    with pytest.raises(ValueError):
        cmf.ANLSUpdate._variant(":comb")
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.ANLSUpdate(np.zeros((1, 8)), np.zeros((1, 1, 1)), np.zeros((1, 8)), devices=[0, 1])
    with pytest.raises(NotImplementedError, match="at most"):
        T = cmf.ANLSUpdate.MAX_T + 1
        cmf.ANLSUpdate(np.zeros((1, T)), np.zeros((1, 1, 1)), np.zeros((1, T)))


def test_fit_cnmf_takes_the_type_without_a_gpu_only_to_fail_loudly():
    """Without a device fit_cnmf(alg=ANLSUpdate) must raise the library's error, never compute on the CPU; with one, the GPU tests
    cover it.  Either way the keyword `variant` draws no 'unknown keyword' warning."""
    import warnings

    import cmf_jl_amd as cmf

    if cmf.load_library().cmf_device_count() > 0:
        pytest.skip("a GPU is present")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(cmf.CMFError) as ei:
            cmf.fit_cnmf(np.ones((4, 16)), L=2, K=2, alg=cmf.ANLSUpdate, max_itr=1, variant=":block")
    assert ei.value.code == 2


def test_library_exports_the_entries_and_refuses_null_handles():
    """Loaded the way tests/test_library_abi.py loads it.  (An unprepared handle, NULL factors and a bad variant need a handle,
    hence a device: tests/test_gpu_anls.py.)"""
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as cmf

    lib = ctypes.CDLL(cmf.LIB_PATH)
    for name in ("cmf_anls_prepare", "cmf_anls_update_motifs", "cmf_anls_update_feature_maps"):
        assert hasattr(lib, name) and name in cmf.SYMBOLS
    lib.cmf_last_error.restype = ctypes.c_char_p
    x = (ctypes.c_double * 4)()
    assert lib.cmf_anls_prepare(None, x) == 1
    assert lib.cmf_anls_update_motifs(None, x, x) == 1
    assert lib.cmf_anls_update_feature_maps(None, x, x, 0, None) == 1
    assert b"NULL" in lib.cmf_last_error()
    assert lib.cmf_set_option(None, b"anls_backup_only", 1) == 1
    buf = ctypes.create_string_buffer(1024)
    assert lib.cmf_option_names(buf, 1024) == 0 and b"anls_backup_only" not in buf.value  # not a path of the listed rules


def test_header_entries_exist_and_cite_the_reference():
    hdr = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    for name, proto, cite in (
        ("cmf_anls_prepare", r"int cmf_anls_prepare\(cmf_handle h, const double \*data\);", "anls.jl:10-14"),
        ("cmf_anls_update_motifs", r"int cmf_anls_update_motifs\(cmf_handle h, const double \*H, double \*W\);", "anls.jl:22-24"),
        ("cmf_anls_update_feature_maps", r"int cmf_anls_update_feature_maps\(cmf_handle h, const double \*W, double \*H, int variant,\s*"
                                         r"double \*loss\);", "anls.jl:26-36"),
    ):
        assert re.search(proto, hdr), name
        block = hdr[hdr.rindex("/*", 0, hdr.index(f"int {name}(")):hdr.index(f"int {name}(")]
        assert cite in block, (name, cite)
    for word in ('"anls_backup_only"', '"anls_W_exchanges"', '"anls_H_exchanges"', '"anls_backup"', '"anls_capped"', "cmf_anls.hip", "cmf_anls.h,"):
        assert word in hdr, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integ for n in ("cmf_anls_prepare", "cmf_anls_update_motifs", "cmf_anls_update_feature_maps", "HIPANLSUpdate"))


def test_julia_binding_has_the_anls_rule():
    jl = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert re.search(r"mutable struct HIPANLSUpdate <: AbstractCFUpdate", jl)
    for name in ("cmf_anls_prepare", "cmf_anls_update_motifs", "cmf_anls_update_feature_maps"):
        assert f"(:{name}, LIBCMF)" in jl, name
    assert re.search(r"function update_feature_maps!\(rule::HIPANLSUpdate, data, W, H; variant=:basic, kwargs\.\.\.\)", jl)
    assert re.search(r"function update_motifs!\(rule::HIPANLSUpdate, data, W, H; kwargs\.\.\.\)", jl)
    assert re.search(r'function HIPANLSUpdate\(data, W, H; device::Integer=parse\(Int, get\(ENV, "LOCAL_RANK", "0"\)\)\)', jl)


def test_the_source_digest_covers_the_new_translation_unit():
    import cmf_jl_amd as cmf

    build = __import__("importlib").import_module(cmf.__name__ + ".build") if hasattr(cmf, "__path__") else None
    if build is None:
        pytest.skip("the package shim has no build module")
    names = [os.path.basename(p) for p in build.DEPS]
    assert "cmf_anls.hip" in names and "cmf_anls.h" in names
    hdr = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    listed = re.search(r"compiled from \((.*?)in that order", hdr, flags=re.S).group(1)
    listed = [os.path.basename(w.strip(" *\n")) for w in listed.replace("\n", " ").split(",") if w.strip(" *\n")]
    assert listed == names, (listed, names)
