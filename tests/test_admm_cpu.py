"""CPU checks of the ADMM rule (src/algs/admm.jl): the fp64 restatement's two modes agree, the W call converges to an answer
computed independently, and the rule is wired through every layer (header, binding, Python, Julia)."""
import os
import re

import numpy as np
import pytest

import admm_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def problem(N, T, K, L, seed):
    rng = np.random.default_rng(seed)
    data = R.conv(rng.random((K, N, L)), rng.random((K, T)) * (rng.random((K, T)) < 0.3)) + 0.1 * rng.random((N, T))
    return data, rng.random((K, N, L)), rng.random((K, T))


@pytest.mark.parametrize("N,T,K,L,kw", [
    (6, 40, 3, 4, {}),
    (5, 7, 2, 5, {}),                   # T < 2L-1: the lags alias in the per-frequency Grams
    (4, 31, 3, 3, {}),                  # prime T
    (3, 13, 1, 1, {}),                  # K = 1, L = 1
    (5, 24, 2, 3, {"nonneg": False}),
    (5, 24, 2, 3, {"l1H": 0.2}),
    (5, 24, 2, 3, {"tol": -np.inf, "maxiter": 60}),
])
def test_literal_and_rewritten_forms_agree(N, T, K, L, kw):
    data, W, H = problem(N, T, K, L, seed=N * T + K + L)
    wkw = {k: v for k, v in kw.items() if k in ("nonneg", "tol", "maxiter")}
    hkw = {k: v for k, v in kw.items() if k in ("nonneg", "tol", "maxiter", "l1H")}
    a, b = R.update_motifs(data, H, L, mode="literal", **wkw), R.update_motifs(data, H, L, **wkw)
    assert a[2:] == b[2:] and rel(b[0], a[0]) < 1e-12
    a, b = R.update_feature_maps(data, W, mode="literal", **hkw), R.update_feature_maps(data, W, **hkw)
    assert a[2:] == b[2:] and rel(b[0], a[0]) < 1e-12 and abs(a[1] - b[1]) < 1e-12


def test_lag_gram_identity():
    """(whc_t whc_t')[k, k'] = sum_d A_kk'(d) exp(+2 pi i t d / T), including T < 2L-1."""
    rng = np.random.default_rng(1)
    for T in (5, 7, 19):
        W = rng.random((3, 4, 4))
        wh = np.zeros((3, 4, T), dtype=complex)
        wh[:, :, :4] = W
        whc = np.conj(np.fft.fft(wh, axis=2))
        A = R.lag_grams(W)
        d = np.arange(-3, 4)
        for t in range(T):
            lit = whc[:, :, t] @ whc[:, :, t].conj().T
            rw = np.einsum("d,dij->ij", np.exp(2j * np.pi * ((t * d) % T) / T), A)
            assert np.abs(lit - rw).max() < 1e-12 * np.abs(lit).max()


def test_w_call_converges_to_the_constrained_least_squares_answer():
    """With admm_tol = -inf and many inner iterations, the W call's ADMM iterate approaches the minimiser of |data - conv(W, H)|
    under W >= 0 and |W[:, n, :]| <= 1, which an accelerated projected-gradient solve finds independently.  The data are large
    enough that every column's norm constraint is active.  The primal iterate Wstk is compared: the factor the call returns is
    Z3, which the revert rule (admm.jl:101-105) holds at the lowest-loss iterate -- an infeasible one here, since the iterates
    reach the constraint set from the low-loss side."""
    rng = np.random.default_rng(4)
    N, T, K, L = 3, 24, 2, 3
    H = rng.random((K, T))
    data = 5.0 * (R.conv(rng.random((K, N, L)), H) + 0.2 * rng.random((N, T)))
    st = {}
    W, _, iters, reverts = R.update_motifs(data, H, L, maxiter=6000, tol=-np.inf, stats=st)
    assert iters == 6000 and reverts > 0
    Hs = R.shift_and_stack(H, L)
    step = 1.0 / np.linalg.eigvalsh(Hs @ Hs.T).max()
    X = np.zeros((L * K, N))
    Y, tk = X.copy(), 1.0
    for _ in range(20000):  # accelerated projected gradient on 0.5 |Hs' X - data'|^2
        Xn = np.maximum(0, Y - step * (Hs @ (Hs.T @ Y - data.T)))
        Xn /= np.maximum(1.0, np.linalg.norm(Xn, axis=0))
        tn = (1 + np.sqrt(1 + 4 * tk * tk)) / 2
        Y, X, tk = Xn + ((tk - 1) / tn) * (Xn - X), Xn, tn
    assert np.allclose(np.linalg.norm(X, axis=0), 1.0)  # the constraint is active in every column
    assert rel(st["Wstk"], X) < 1e-2, rel(st["Wstk"], X)
    assert rel(W, R.fold_W(X, K, N, L)) > 0.1  # ... and Z3 is not there (see above)


def test_admm_symbol_resolves_to_the_rule():
    import cmf_jl_amd as cmf
    from cmf_jl_amd.host import _KNOWN_KW, _resolve_alg

    assert _resolve_alg(":admm") is cmf.ADMMUpdate and _resolve_alg("admm") is cmf.ADMMUpdate
    assert cmf.HIPADMMUpdate is cmf.ADMMUpdate
    assert {"rhow", "rhoh", "admm_W_maxiter", "admm_H_maxiter", "admm_tol", "nonnegW", "nonnegH", "l1H"} <= _KNOWN_KW
    with pytest.raises(NotImplementedError):
        _resolve_alg(":anls")


def test_header_entries_exist_and_cite_the_reference():
    hdr = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    from cmf_jl_amd import SYMBOLS

    for name, proto, cite in (
        ("cmf_admm_prepare", r"int cmf_admm_prepare\(cmf_handle h, const double \*data\);", "admm.jl:13-21"),
        ("cmf_admm_update_motifs", r"int cmf_admm_update_motifs\(cmf_handle h, const double \*H, double \*W, double rhow, int64_t maxiter, "
                                   r"double tol, int nonnegW,\s+int64_t \*iters\);", "admm.jl:24-121"),
        ("cmf_admm_update_feature_maps", r"int cmf_admm_update_feature_maps\(cmf_handle h, const double \*W, double \*H, double rhoh, "
                                         r"int64_t maxiter, double l1H, double tol,\s+int nonnegH, double \*loss, int64_t \*iters\);", "admm.jl:124-226"),
    ):
        assert re.search(proto, hdr), name
        block = hdr[hdr.rindex("/*", 0, hdr.index(f"int {name}(")):hdr.index(f"int {name}(")]
        assert cite in block, (name, cite)
        assert name in SYMBOLS
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integ for n in ("cmf_admm_prepare", "cmf_admm_update_motifs", "cmf_admm_update_feature_maps"))


def test_julia_binding_has_the_admm_rule():
    jl = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert re.search(r"mutable struct HIPADMMUpdate <: AbstractCFUpdate", jl)
    for name in ("cmf_admm_prepare", "cmf_admm_update_motifs", "cmf_admm_update_feature_maps"):
        assert f"(:{name}, LIBCMF)" in jl, name
    m = re.search(r"function update_feature_maps!\(rule::HIPADMMUpdate, data, W, H;\s*rhoh=10, admm_H_maxiter=30, l1H=0, admm_tol=1e-4, "
                  r"nonnegH=true", jl)
    assert m
    assert re.search(r"function update_motifs!\(rule::HIPADMMUpdate, data, W, H;\s*rhow=10, admm_W_maxiter=30, admm_tol=1e-4, nonnegW=true", jl)


def test_admm_rule_refuses_what_it_cannot_run_before_touching_a_device():
    """A recording longer than one contraction launch covers would make cmf_create cut it into a T-sharded group: refused up front
    with a clear message (no device needed)."""
    import cmf_jl_amd as cmf

    T = cmf.ADMMUpdate.MAX_T + 1
    with pytest.raises(NotImplementedError, match="at most"):
        cmf.ADMMUpdate(np.zeros((1, T)), np.zeros((1, 1, 1)), np.zeros((1, T)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        cmf.ADMMUpdate(np.zeros((1, 8)), np.zeros((1, 1, 1)), np.zeros((1, 8)), devices=[0, 1])
