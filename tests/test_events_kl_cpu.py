"""CPU checks of the KL form of the MU rule on event lists (cmf_events_*, EventData, EventKLUpdate, fit_cnmf on event data).

What makes the new rule the old definition: on the densified events the event-form restatement (tests/events_kl_restatement.py) IS
tests/kl_mu_restatement.py's fit_kl, to 1e-12 relative after 20 iterations, on all seven mu_kl_* fixtures and on the sparse problems
the GPU test fits; the closed form of the sum of est over all entries is held against the dense sum on its own.  Then: EventData,
the host refusals, the binding, the HIP-free index code under the sanitizers, the committed precision file.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import events_kl_restatement as er
import kl_mu_restatement as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["mu_kl_small", "mu_kl_small_reg", "mu_kl_k5", "mu_kl_k33", "mu_kl_k32", "mu_kl_short", "mu_kl_l40"]
REL = 1e-12
SMALL_SPARSE = er.PROBLEMS[:3]


@pytest.fixture(scope="module")
def cmf():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as m

    return m


def frob_rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def same_fit(ev, data, W0, H0, iters, reg):
    We, He, le = er.fit_events(ev, W0, H0, max_itr=iters, **reg)
    Wd, Hd, ld = kr.fit_kl(data, W0, H0, max_itr=iters, **reg)
    print("relW", frob_rel(We, Wd), "relH", frob_rel(He, Hd), "max rel loss", float(np.max(np.abs(le - ld) / ld)))
    assert frob_rel(We, Wd) <= REL and frob_rel(He, Hd) <= REL
    np.testing.assert_allclose(le, ld, rtol=REL)


@pytest.mark.parametrize("name", FIXTURES)
def test_event_restatement_is_the_dense_restatement_on_the_fixtures(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    data, W0, H0 = (np.asarray(g[k], dtype=np.float64) for k in ("data", "W0", "H0"))
    ev = er.from_dense(data)
    np.testing.assert_array_equal(er.to_dense(ev), data)
    same_fit(ev, data, W0, H0, 20, {k: float(g[k]) for k in ("l1W", "l2W", "l1H", "l2H")})


@pytest.mark.parametrize("name,gen,kw,iters,reg", SMALL_SPARSE, ids=[p[0] for p in SMALL_SPARSE])
def test_event_restatement_is_the_dense_restatement_on_the_sparse_problems(name, gen, kw, iters, reg):
    ev, W0, H0 = gen(**kw)
    same_fit(ev, er.to_dense(ev), W0, H0, 20, reg)


def test_skewed_problem_has_what_it_promises():
    (unit, time, count, (N, T)), _, _ = er.sparse_problem(N=40, T=4000, K=3, L=12, density=0.02, seed=11, skewed=True)
    per_unit = np.bincount(unit, minlength=N)
    assert per_unit[1] == T and sorted(np.nonzero(per_unit == 0)[0]) == [0, 20, 39]  # one unit in every column, three without events
    others = time[unit != 1]
    assert 0 in others and T - 1 in others
    gaps = np.diff(np.unique(others))
    assert gaps.max() > 12  # an empty stretch longer than L
    assert 0.01 < unit.size / (N * T) < 0.05 and (count > 0).all()


@pytest.mark.parametrize("shape", [(6, 40, 3, 5), (4, 3, 2, 7), (1, 1, 1, 1), (5, 9, 2, 9)])
def test_closed_form_of_the_sum_of_est(shape):
    N, T, K, L = shape
    rng = np.random.default_rng(5)
    W, H = rng.random((K, N, L)), rng.random((K, T))
    dense = float(np.sum(kr.tensor_conv(W, H) + kr.EPS))
    assert abs(er.sum_all_est(W, H, N) - dense) <= 1e-13 * dense


def test_event_data_sorts_sums_duplicates_and_drops_zeros(cmf):
    ev = cmf.EventData(unit=[2, 0, 2, 1, 0, 2], time=[3, 1, 3, 0, 4, 0], count=[1.0, 2.0, 0.5, 0.0, 4.0, 8.0], shape=(3, 5))
    assert ev.nnz == 4 and ev.shape == (3, 5)
    assert ev.unit.tolist() == [0, 0, 2, 2] and ev.time.tolist() == [1, 4, 0, 3] and ev.count.tolist() == [2.0, 4.0, 8.0, 1.5]
    assert ev.unit.dtype == np.int32 and ev.time.dtype == np.int32 and ev.count.dtype == np.float64
    assert ev.sum() == 15.5
    dense = ev.todense()
    assert dense.shape == (3, 5) and dense[2, 3] == 1.5 and dense.sum() == 15.5 and np.count_nonzero(dense) == 4
    # duplicates are summed in fp64 in INPUT order: (1e16 + 1) + 1 loses both ones, (1 + 1) + 1e16 keeps them
    a = cmf.EventData([0, 0, 0], [0, 0, 0], [1e16, 1.0, 1.0], (1, 1)).count[0]
    b = cmf.EventData([0, 0, 0], [0, 0, 0], [1.0, 1.0, 1e16], (1, 1)).count[0]
    assert a == 1e16 and b == 1e16 + 2


def test_event_data_refusals(cmf):
    E = cmf.EventData
    for bad, match in (([-1.0], "negative"), ([np.nan], "finite"), ([np.inf], "finite")):
        with pytest.raises(ValueError, match=match):
            E([0], [0], bad, (2, 2))
    for unit, time in (([2], [0]), ([0], [2]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(ValueError, match="out of range"):
            E(unit, time, [1.0], (2, 2))
    with pytest.raises(ValueError, match="integers"):
        E([0.5], [0], [1.0], (2, 2))
    with pytest.raises(ValueError, match="one length"):
        E([0, 1], [0], [1.0], (2, 2))
    with pytest.raises(ValueError, match="finite"):
        E.from_dense(np.array([[1.0, np.nan]]))


def test_event_data_round_trip_and_duck_typed_sparse(cmf):
    rng = np.random.default_rng(2)
    a = rng.integers(0, 4, (7, 31)) * (rng.random((7, 31)) < 0.2) * 1.0
    ev = cmf.EventData.from_dense(a)
    np.testing.assert_array_equal(ev.todense(), a)
    assert ev.nnz == np.count_nonzero(a)
    ru, rt, rc, _ = er.from_dense(a)
    assert ev.unit.tolist() == ru.tolist() and ev.time.tolist() == rt.tolist() and ev.count.tolist() == rc.tolist()

    class Coo:
        def __init__(self, m):
            self.row, self.col = np.nonzero(m.T)[1], np.nonzero(m.T)[0]  # (column-major order: EventData sorts)
            self.data, self.shape = m[self.row, self.col], m.shape

    class Sparse:
        def tocoo(self):
            return Coo(a)

    ev2 = cmf.EventData.from_sparse(Sparse())
    np.testing.assert_array_equal(ev2.todense(), a)
    assert ev2.unit.tolist() == ev.unit.tolist() and ev2.time.tolist() == ev.time.tolist()
    for f in os.listdir(os.path.join(ROOT, "cmf.jl_amd")):  # the package never imports scipy
        if f.endswith(".py"):
            assert not re.search(r"^\s*(import|from)\s+scipy", open(os.path.join(ROOT, "cmf.jl_amd", f)).read(), flags=re.M), f


def test_init_rand_events_takes_the_librarys_draws_and_the_kl_scale(cmf):
    ev = cmf.EventData.from_dense(np.arange(12.0).reshape(3, 4))
    W, H = cmf.init_rand_events(ev, L=2, K=2, seed=7)
    assert W.shape == (2, 3, 2) and H.shape == (2, 4) and W.flags.f_contiguous and H.flags.f_contiguous
    # alpha = sum(x) / sum_all(est): the scaled model's total is the data's total (the stationary point of the KL divergence in a scalar)
    assert abs(er.sum_all_est(W, H, 3) - ev.sum()) <= 1e-12 * ev.sum()
    # the draws: csrc/cmf_rng.h, counter 0 of stream 0 for seed 7, written out
    m64 = (1 << 64) - 1

    def mix(z):
        z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & m64
        z ^= z >> 27; z = (z * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)

    base = mix((7 + 0x632BE59BD9B4E019) & m64)
    u0 = (mix((base + 0x9E3779B97F4A7C15) & m64) >> 11) * 2.0 ** -53
    u = cmf.host._rng_u01(7, 0, 12)
    assert u[0] == u0 and (u >= 0).all() and (u < 1).all()
    s = W[0, 0, 0] / u0
    np.testing.assert_allclose(W.ravel(order="F"), u * s, rtol=1e-15)
    W2, H2 = cmf.init_rand_events(ev, L=2, K=2, seed=7)
    assert np.array_equal(W, W2) and np.array_equal(H, H2)


def test_fit_cnmf_refusals_name_their_reason(cmf):
    """Raised before anything touches a device: no GPU needed."""
    ev = cmf.EventData.from_dense(np.random.default_rng(0).integers(0, 3, (6, 40)) * 1.0)
    for alg in (":hals", ":pgd", ":admm", cmf.ANLSUpdate, ":sep"):
        with pytest.raises(NotImplementedError, match="alg=:mult"):
            cmf.fit_cnmf(ev, L=3, K=2, alg=alg, divergence=":kl")
    with pytest.raises(NotImplementedError, match="divergence=':kl' only"):
        cmf.fit_cnmf(ev, L=3, K=2, alg=":mult")  # (the default, ":square")
    for div, extra in ((":square", {}), (":itakura_saito", {}), (":beta", dict(beta=0.5))):
        with pytest.raises(NotImplementedError, match="divergence=':kl' only"):
            cmf.fit_cnmf(ev, L=3, K=2, alg=":mult", divergence=div, **extra)
    with pytest.raises(NotImplementedError, match="mask="):
        cmf.fit_cnmf(ev, L=3, K=2, alg=":mult", divergence=":kl", mask=np.ones((6, 40)))
    for k in ("lambda_xortho", "lambda_ortho_H", "lambda_ortho_W"):
        with pytest.raises(NotImplementedError, match="cross-orthogonality"):
            cmf.fit_cnmf(ev, L=3, K=2, alg=":mult", divergence=":kl", **{k: 0.1})
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.fit_cnmf(ev, L=3, K=2, alg=":mult", divergence=":kl", devices=[0, 0])
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.EventKLUpdate(ev, np.ones((2, 6, 3)), np.ones((2, 40)), devices=[0])
    with pytest.raises(TypeError, match="EventData"):
        cmf.EventKLUpdate(np.ones((6, 40)), np.ones((2, 6, 3)), np.ones((2, 40)))
    r = cmf.CNMF_results(ev, np.ones((2, 6, 3)), np.ones((2, 40)), np.arange(2.0), np.ones(2))
    with pytest.raises(NotImplementedError, match="event list"):
        cmf.save_model(r, "never_written.npz")
    with pytest.raises(NotImplementedError, match="kind=':kl' only"):
        cmf.evaluate_divergence(r, kind=":square")


def test_library_refusals_come_before_any_device(cmf):
    """cmf_events_create validates first: CMF_ERR_ARG / CMF_ERR_UNSUPPORTED with a message, with or without a GPU."""
    lib = cmf.load_library()
    i32 = ctypes.POINTER(ctypes.c_int32)
    pd = ctypes.POINTER(ctypes.c_double)

    def create(N, T, K, L, unit, time, count, nnz=None):
        u, t, c = np.asarray(unit, dtype=np.int32), np.asarray(time, dtype=np.int32), np.asarray(count, dtype=np.float64)
        h = ctypes.c_void_p()
        rc = lib.cmf_events_create(ctypes.byref(h), 0, N, T, K, L, len(u) if nnz is None else nnz, u.ctypes.data_as(i32), t.ctypes.data_as(i32),
                                   c.ctypes.data_as(pd))
        assert not h.value or rc == 0
        if rc == 0:
            lib.cmf_events_destroy(h)
        return rc, lib.cmf_last_error().decode()

    ok = ([0, 1], [1, 0], [1.0, 2.0])
    assert create(2, 2, 1, 1, [0, 2], [1, 0], ok[2])[0] == 1
    assert create(2, 2, 1, 1, ok[0], [1, 2], ok[2])[0] == 1
    for bad in (0.0, -1.0, np.nan, np.inf):
        rc, msg = create(2, 2, 1, 1, ok[0], ok[1], [1.0, bad])
        assert rc == 1 and "finite and > 0" in msg
    rc, msg = create(2, 2, 1, 1, [1, 0], [0, 1], ok[2])
    assert rc == 1 and "sorted" in msg
    assert create(2, 2, 1, 1, [0, 0], [1, 1], ok[2])[0] == 1  # a duplicate
    assert create(2, 2, 1, 1, ok[0], ok[1], ok[2], nnz=0)[0] == 1
    for dims in ((0, 2, 1, 1), (2, 0, 1, 1), (2, 2, 0, 1), (2, 2, 1, 0)):
        assert create(*dims, *ok)[0] == 1
    h = ctypes.c_void_p()
    assert lib.cmf_events_create(ctypes.byref(h), 0, 2, 2, 1, 1, 2, None, None, None) == 1 and "NULL" in lib.cmf_last_error().decode()
    rc, msg = create(2, 2, 257, 1, *ok)
    assert rc == 4 and "K <= 256" in msg
    rc, msg = create(2, 2, 33, 65, *ok)
    assert rc == 4 and "4096" in msg
    for fn, args in (("cmf_events_update_motifs", (0.0, 0.0)), ("cmf_events_destroy", ()), ("cmf_events_compute_loss", (None,))):
        rc = getattr(lib, fn)(None, *args)
        assert rc == (0 if fn == "cmf_events_destroy" else 1)


def test_new_entries_are_exported_and_bound(cmf):
    names = ["cmf_events_create", "cmf_events_destroy", "cmf_events_set_factors", "cmf_events_get_factors", "cmf_events_update_motifs",
             "cmf_events_update_feature_maps", "cmf_events_compute_loss", "cmf_events_iterate", "cmf_events_terms", "cmf_events_set_option",
             "cmf_events_get_counter"]
    lib = ctypes.CDLL(cmf.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    bound = cmf.load_library()
    for n in names:
        assert n in cmf.SYMBOLS and hasattr(lib, n) and getattr(bound, n).argtypes is not None
        assert re.search(rf"\bint {n}\(cmf_events ", header), n
    assert lib.cmf_abi_version() == 6  # the entries are additive
    assert re.search(r"typedef struct cmf_events_s \*cmf_events;", header)
    assert "`cmf_events_create`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("EventData", "EventKLUpdate", "init_rand_events"):
        assert hasattr(cmf, name)
    assert issubclass(cmf.EventKLUpdate, cmf.AbstractCFUpdate)


def test_the_source_digest_covers_the_new_translation_unit():
    sys.path.insert(0, os.path.join(ROOT, "cmf.jl_amd"))
    try:
        import build
    finally:
        sys.path.pop(0)
    base = {os.path.basename(p) for p in build.DEPS}
    assert {"cmf_events.hip", "cmf_events.h"} <= base and any(p.endswith("cmf_events.hip") for p in build.SOURCES)


def test_restatement_is_test_infrastructure_only():
    """Nothing under cmf.jl_amd/, include/ or bench.py imports the restatement."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("cmf.jl_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(d, f) for f in files if f.endswith((".py", ".h", ".hip", ".jl"))]
    for p in paths:
        assert "events_kl_restatement" not in open(p, errors="replace").read(), p


def test_index_and_validation_under_the_sanitizers(tmp_path):
    """cmf.jl_amd/csrc/cmf_events.h is free of HIP: tests/events_index_stress.cpp (its own main) drives it under ASan and UBSan."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "events_index_stress")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "cmf.jl_amd", "csrc"), os.path.join(ROOT, "tests", "events_index_stress.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok "), p.stdout + p.stderr
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr


def test_no_preload_anywhere_in_the_new_files():
    word = "LD_" + "PRELOAD"
    for rel in ("tests/test_gpu_events_kl.py", "tests/events_kl_restatement.py", "tests/events_index_stress.cpp", "tools/mu_kl_events_precision.py",
                "tools/time_events_kl.py", "cmf.jl_amd/csrc/cmf_events.h", "cmf.jl_amd/csrc/cmf_events.hip"):
        assert word not in open(os.path.join(ROOT, rel)).read(), rel


def test_committed_precision_file_is_what_the_tool_writes():
    """profiles/mu_kl_events_precision.txt against tools/mu_kl_events_precision.py, on the cases that run in seconds: the fixtures'
    lines at their first three counts and the three small sparse problems in full."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mu_kl_events_precision as tool
    finally:
        sys.path.pop(0)
    text = open(os.path.join(ROOT, "profiles", "mu_kl_events_precision.txt")).read()
    rows = {ln.split(" | ")[0]: ln.split(" | ")[1:] for ln in text.splitlines() if " | " in ln and not ln.startswith("#")}
    admits = {ln.split()[1]: int(ln.split()[2]) for ln in text.splitlines() if ln.startswith("admit ")}
    names = [c[0] for c in tool.SPARSE] + tool.FIXTURES
    assert sorted(rows) == sorted(names) == sorted(admits)
    small = {c[0] for c in tool.SPARSE[:3]}
    for name, ev, W0, H0, reg, top in tool.cases():
        if name in small:
            counts = [c for c in tool.COUNTS if c <= top]
        elif name in ("mu_kl_small", "mu_kl_short", "mu_kl_k5"):
            counts = list(tool.COUNTS[:3])
        else:
            continue
        saved, tool.COUNTS = tool.COUNTS, tuple(counts)
        try:
            a = tool.trajectory(ev, W0, H0, reg, np.float64, max(counts))
            b = tool.trajectory(ev, W0, H0, reg, np.float32, max(counts))
        finally:
            tool.COUNTS = saved
        for i, c in enumerate(counts):
            d = max(tool.frob_rel(b[c][0], a[c][0]), tool.frob_rel(b[c][1], a[c][1]), float(np.max(np.abs(b[c][2] - a[c][2]) / a[c][2])))
            # (a float32 rounding drift: numpy's float32 sums run in an order that depends on the SIMD width of the CPU, so the figure is
            # reproduced to a factor of two, and falls on the same side of the admission line)
            have = float(rows[name][i])
            assert d / 2 <= have <= 2 * d, (name, c, rows[name][i], d)
            assert (have <= tool.BAR / 3) == (d <= tool.BAR / 3), (name, c, have, d)
    for name, count in admits.items():  # the admit lines follow from the rows by the project's rule
        ok = 0
        for i, c in enumerate(tool.COUNTS):
            cell = rows[name][i].split()[0]
            if cell == "-" or float(cell) > tool.BAR / 3:
                break
            ok = c
        assert ok == count, (name, ok, count)
