"""Every MU kernel path against the fp64 oracle BIT FOR BIT on integer-valued problems (tests/exact_problems.py).

On these problems est, numW, denomW, numH, denomH, the loss tile sums and the Gram tables are exact in fp32 in any summation
order, so tensor_conv, tensor_transconv and the loss equal the oracle exactly, and the updated factor is the fp64 update up to
the element-wise rounding of cmf_mu (cmf_kernels.h: one division and one multiply, within 2 ulp).  A dropped or doubled time
row, column, lag or component block moves some num or den by at least 1 unit = 8 ulp, so unlike the norm-wise 1e-4 checks of
the full-size fits, a seam error confined to one chunk, tile row or lag block fails here.  Every configuration of a shape must
also give the same bits: num and den are exact, and every path applies the same cmf_mu.

The shape table (exact_problems.SHAPES, shared with tests/test_gpu_divergence_paths.py) is derived from the plan rules (cmf_api.hip plan(), cmf_internal.h launch_conv) on a 256-CU MI355X; the
launch counters (cmf_get_counter "launches:<path>") record which instances each shape reached, and the last test asserts
that the table reaches every named path.  tests/test_gpu_exact_cu_plans.py makes the same assertions (mu_references, run_mu_config
below) on handles planned for 128, 64, 32, 38 and 1 CUs, where the same shapes take other branches."""
import os
import time

import numpy as np
import pytest

from exact_problems import L1, L2, EXACT, SENS, LAUNCH_PATHS, SHAPES, conv3_form, first_bad, make_problem, ulps

pytestmark = pytest.mark.gpu

ULP_BAR = 2
EPS = float(np.finfo(np.float64).eps)

_seen = {}          # launches:<path> summed over every handle of the file
_shapes_done = set()


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


def counters(rule):
    return {p: rule.counter("launches:" + p) for p in LAUNCH_PATHS}


def record(c):
    for p, v in c.items():
        _seen[p] = _seen.get(p, 0) + v


def reached(c):
    return {p: v for p, v in c.items() if v}


def make_rule(cmf, cfg, X, W, H):
    cfg = dict(cfg)
    devices = cfg.pop("devices", None)
    rule = cmf.MultUpdate(X, W, H, devices=devices) if devices else cmf.MultUpdate(X, W, H)
    for name, value in cfg.items():
        rule.set_option(name, value)
    return rule


def mu_ref(x, num, den, l1, l2):
    """mult.jl:37-38 / :51-52 in fp64 (oracle/cmf_oracle.py update_motifs)."""
    return np.maximum(x * (num / (((den + l1) + (2.0 * l2) * x) + EPS)), EPS)


def oracle_w_half(oracle, X, W, H):
    """(est, numW, denomW, W_new) of update_motifs! in fp64 (mult.jl:28-38)."""
    K, N, L = W.shape
    T = H.shape[1]
    est = oracle.tensor_conv(W, H)
    num, den = np.zeros(W.shape), np.zeros(W.shape)
    for lag in range(min(L, T)):
        num[:, :, lag] = H[:, : T - lag] @ X[:, lag:].T
        den[:, :, lag] = H[:, : T - lag] @ est[:, lag:].T
    return est, num, den, mu_ref(W, num, den, L1, L2)


def oracle_h_half(oracle, X, W, H):
    """(est, numH, denomH, H_new, loss after the update) of update_feature_maps! in fp64 (mult.jl:44-57)."""
    est = oracle.tensor_conv(W, H)
    num = oracle.tensor_transconv(W, X)
    den = oracle.tensor_transconv(W, est)
    Hn = mu_ref(H, num, den, L1, L2)
    return est, num, den, Hn, oracle.compute_loss(X, W, Hn)


def max_tile_sumsq(est, X, tile=128):
    """The largest exact sum of (est - X)^2 over a tile x tile block (a bound for the 64 x 64 loss tiles of the conv epilogues)."""
    N, T = X.shape
    r = np.zeros((-(-N // tile) * tile, -(-T // tile) * tile))
    r[:N, :T] = (est - X) ** 2
    return r.reshape(r.shape[0] // tile, tile, r.shape[1] // tile, tile).sum(axis=(1, 3)).max()


def assert_preconditions(num, den, est, shape):
    """(a) every accumulation exact, (b) one unit of num / den is at least 8 ulp -- from the arrays actually generated."""
    assert max(num.max(), den.max(), est.max()) < EXACT, f"{shape}: an fp32 accumulation would round"
    assert max(num.max(), den.max()) <= SENS, f"{shape}: num / den above 2^20: the 2 ulp bar could miss a single term"


def check_factor(got, ref, names, what, cfg, c):
    u = ulps(got, ref)
    if u.max() > ULP_BAR:
        raise AssertionError(f"{what} {cfg}: {u.max():.1f} ulp from the fp64 oracle at {first_bad(u > ULP_BAR, names)} "
                             f"(got {got[tuple(np.argwhere(u > ULP_BAR)[0])]!r}, want {ref[tuple(np.argwhere(u > ULP_BAR)[0])]!r}); "
                             f"launches {reached(c)}")


def check_same(got, base, names, what, cfg, base_cfg, c):
    if not np.array_equal(got, base):
        raise AssertionError(f"{what} {cfg} differs from {base_cfg} at {first_bad(got != base, names)}; launches {reached(c)}")


def mu_references(oracle, shape):
    """The two integer problems of a shape, their fp64 halves and losses, with the preconditions asserted from the arrays: computed once
    per shape (tests/test_gpu_exact_cu_plans.py shares them across the CU counts)."""
    N, T, K, L = shape
    r = dict(shape=shape)
    r["Ww"], r["Hw"], r["X"] = make_problem(N, T, K, L, "W")
    est_w, numW, denW, r["W_ref"] = oracle_w_half(oracle, r["X"], r["Ww"], r["Hw"])
    assert_preconditions(numW, denW, est_w, shape)
    r["Wh"], r["Hh"], _ = make_problem(N, T, K, L, "H")
    est_h, numH, denH, r["H_ref"], r["lossH_ref"] = oracle_h_half(oracle, r["X"], r["Wh"], r["Hh"])
    assert_preconditions(numH, denH, est_h, shape)
    r["loss_w_ref"], r["loss_h_ref"] = oracle.compute_loss(r["X"], r["Ww"], r["Hw"]), oracle.compute_loss(r["X"], r["Wh"], r["Hh"])
    r["loss_exact"] = max(max_tile_sumsq(est_w, r["X"]), max_tile_sumsq(est_h, r["X"])) <= EXACT
    return r


def run_mu_config(cmf, cfg, r, record=lambda c: None):
    """One configuration of a row against the references r: (W after the W half, H after the H half, launch counters), everything
    test_exact_mu_paths asserts per configuration asserted."""
    X, Ww, Hw, Wh, Hh = r["X"], r["Ww"], r["Hw"], r["Wh"], r["Hh"]
    rule = make_rule(cmf, cfg, X, Ww, Hw)
    try:
        lw = rule.compute_loss()
        rule.update_motifs(l1W=L1, l2W=L2)
        Wg, _ = rule.download()
        rule.upload(Ww, Hw)
        rule.iterate(1, l1W=L1, l2W=L2, l1H=L1, l2H=L2)
        Wi, _ = rule.download()
        # pipelined iterations (the loss reduction deferred onto the next launch) are the call-by-call loop, bit for bit
        rule.upload(Ww, Hw)
        li = list(rule.iterate(2, l1W=L1, l2W=L2, l1H=L1, l2H=L2))
        Wi2, Hi2 = rule.download()
        rule.upload(Ww, Hw)
        lc = []
        for _ in range(2):
            rule.update_motifs(l1W=L1, l2W=L2)
            lc.append(rule.update_feature_maps(l1H=L1, l2H=L2))
        Wc2, Hc2 = rule.download()
        c = counters(rule)
    finally:
        rule.close()
    assert li == lc, f"{cfg}: iterate(2) losses {li} != call by call {lc}"
    check_same(Wi2, Wc2, "knl", "W after iterate(2)", cfg, "the call-by-call loop", c)
    check_same(Hi2, Hc2, "kt", "H after iterate(2)", cfg, "the call-by-call loop", c)
    rule = make_rule(cmf, cfg, X, Wh, Hh)
    try:
        lh = rule.compute_loss()
        lh1 = rule.update_feature_maps(l1H=L1, l2H=L2)
        _, Hg = rule.download()
        ch = counters(rule)
    finally:
        rule.close()
    c = {p: c[p] + ch[p] for p in c}
    record(c)
    if r["loss_exact"]:
        assert (lw, lh) == (r["loss_w_ref"], r["loss_h_ref"]), f"loss {cfg}: {(lw, lh)} != {(r['loss_w_ref'], r['loss_h_ref'])}; launches {reached(c)}"
    else:  # (some 64 x 64 tile sum of (est - X)^2 may exceed 2^24: not exact by construction)
        np.testing.assert_allclose([lw, lh], [r["loss_w_ref"], r["loss_h_ref"]], rtol=1e-6)
    np.testing.assert_allclose(lh1, r["lossH_ref"], rtol=1e-5)  # (H is no longer integer: today's bar)
    check_factor(Wg, r["W_ref"], "knl", "W half: W", cfg, c)
    check_factor(Hg, r["H_ref"], "kt", "H half: H", cfg, c)
    check_same(Wi, Wg, "knl", "W after iterate(1)", cfg, "update_motifs!", c)
    return Wg, Hg, c


@pytest.mark.parametrize("N,T,K,L,configs,why", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
def test_exact_mu_paths(cmf, oracle, N, T, K, L, configs, why):
    shape = (N, T, K, L)
    t0 = time.perf_counter()
    r = mu_references(oracle, shape)
    t_oracle = time.perf_counter() - t0
    base = None
    for cfg in configs:
        if T // len(cfg.get("devices", [0])) < 2 * L:
            continue  # (shards shorter than two lag windows: not a shape a group takes)
        Wg, Hg, c = run_mu_config(cmf, cfg, r, record=record)
        if base is None:
            base = (cfg, Wg, Hg)
        else:
            check_same(Wg, base[1], "knl", "W half: W", cfg, base[0], c)
            check_same(Hg, base[2], "kt", "H half: H", cfg, base[0], c)
    _shapes_done.add(shape)
    print(f"{shape} {why}: oracle {t_oracle:.2f} s, total {time.perf_counter() - t0:.2f} s")


def test_exact_config2_once(cmf, oracle):
    """Config 2 itself (N = 2000, T = 50000, K = 32, L = 20): conv launches of 4 and more rounds (whole tiles + the extra cut),
    the hxt chunks of the full recording; W half, the loss and iterate(1)."""
    N, T, K, L = 2000, 50000, 32, 20
    W, H, X = make_problem(N, T, K, L, "W")
    est, num, den, W_ref = oracle_w_half(oracle, X, W, H)
    assert_preconditions(num, den, est, (N, T, K, L))
    assert max_tile_sumsq(est, X) <= EXACT
    assert conv3_form(N, T) == "whole+4"
    rule = cmf.MultUpdate(X, W, H)
    try:
        assert rule.compute_loss() == oracle.compute_loss(X, W, H)
        rule.update_motifs(l1W=L1, l2W=L2)
        Wg, _ = rule.download()
        rule.upload(W, H)
        rule.iterate(1, l1W=L1, l2W=L2, l1H=L1, l2H=L2)
        Wi, _ = rule.download()
        c = counters(rule)
    finally:
        rule.close()
    record(c)
    check_factor(Wg, W_ref, "knl", "config 2: W", {}, c)
    check_same(Wi, Wg, "knl", "config 2: W after iterate(1)", {}, "update_motifs!", c)


@pytest.mark.parametrize("N,T,K,L", [(130, 700, 32, 20), (130, 700, 5, 20), (70, 600, 20, 10)])
def test_exact_primitives_and_long_recordings(cmf, oracle, N, T, K, L):
    """tensor_conv / tensor_transconv equal the oracle exactly, whole and column-blocked; a recording longer than a handle holds
    (CMF_MAX_COLUMNS under CMF_TEST_HOOKS=1: sharded automatically on one device) gives the unsharded handle's bits."""
    W, H, X = make_problem(N, T, K, L, "W")
    est_ref, tc_ref = oracle.tensor_conv(W, H), oracle.tensor_transconv(W, X)
    np.testing.assert_array_equal(cmf.tensor_conv(W, H), est_ref)
    np.testing.assert_array_equal(cmf.tensor_transconv(W, X), tc_ref)
    _, _, _, W_ref = oracle_w_half(oracle, X, W, H)
    Wh, Hh, _ = make_problem(N, T, K, L, "H")
    H_ref = oracle_h_half(oracle, X, Wh, Hh)[3]
    os.environ["CMF_TEST_HOOKS"] = "1"
    os.environ["CMF_MAX_COLUMNS"] = "300"
    try:
        np.testing.assert_array_equal(cmf.tensor_conv(W, H), est_ref)
        np.testing.assert_array_equal(cmf.tensor_transconv(W, X), tc_ref)
        rule = cmf.MultUpdate(X, W, H)
        try:
            assert rule.compute_loss() == oracle.compute_loss(X, W, H)
            rule.update_motifs(l1W=L1, l2W=L2)
            Wg, _ = rule.download()
            record(counters(rule))
        finally:
            rule.close()
        rule = cmf.MultUpdate(X, Wh, Hh)
        try:
            rule.update_feature_maps(l1H=L1, l2H=L2)
            _, Hg = rule.download()
            record(counters(rule))
        finally:
            rule.close()
    finally:
        os.environ.pop("CMF_MAX_COLUMNS", None)
        os.environ.pop("CMF_TEST_HOOKS", None)
    check_factor(Wg, W_ref, "knl", "sharded W half: W", {"CMF_MAX_COLUMNS": 300}, {})
    check_factor(Hg, H_ref, "kt", "sharded H half: H", {"CMF_MAX_COLUMNS": 300}, {})


def test_launch_counters(cmf):
    """The counters are there for every name and only for those; a group handle sums its shards."""
    W, H, X = make_problem(130, 700, 32, 20, "W")
    rule = cmf.MultUpdate(X, W, H, devices=[0, 0])
    try:
        c0 = counters(rule)  # (creating a group already exchanges the halos of H)
        rule.update_motifs()
        c = {p: v - c0[p] for p, v in counters(rule).items()}
        assert c["hxt_kernel<5>"] >= 2 and c["hxt_kernel<5>"] == c["hxt_kernel:nsrc1"] + c["hxt_kernel:nsrc2"]  # (each shard launches C2)
        assert c["transconv_kernel<20>"] == 0 and all(v >= 0 for v in c.values())
        with pytest.raises(Exception):
            rule.counter("launches:no_such_kernel")
    finally:
        rule.close()


def test_every_launch_path_reached():
    """The union of launches:* over the table above reaches every named path (a new instance cannot land untested)."""
    if len(_shapes_done) < len(SHAPES):
        pytest.skip("runs after the whole table (the file as a whole)")
    missing = [p for p in LAUNCH_PATHS if not _seen.get(p)]
    print({p: _seen.get(p, 0) for p in LAUNCH_PATHS})
    assert not missing, f"launch paths no shape reached: {missing}"
