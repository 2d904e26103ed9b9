"""CPU half of tests/test_exact_parity.py: the integer problems' preconditions over its whole shape table, the ulp comparator's
power to see one missing term, and the launch-path names kept equal to the library's table."""
import os
import re

import numpy as np

import exact_problems as ep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_table():
    """SHAPES of tests/test_exact_parity.py, read from its source (the module itself is GPU-marked)."""
    import ast

    src = open(os.path.join(ROOT, "tests", "test_exact_parity.py")).read()
    tree = ast.parse(src)
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "SHAPES" for t in node.targets):
            return [tuple(ast.literal_eval(e) for e in elt.elts[:4]) for elt in node.value.elts]
    raise AssertionError("no SHAPES table")


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
