"""The exact kernel-path tests under plans for FEWER COMPUTE UNITS than the chip has.

Every contraction launch is dealt out by plan(), launch_conv / conv_tail_cut, tc_plan, the few-component plan and hals_plan, and all of
them are functions of one number: the CU count cmf_create reads from the device.  An MI355X shows 128, 64 or 32 CUs per device in its
partitioned modes, and under another count the same shapes take other branches: other hxt chunk lengths and tail rows, another number of
waves per transconv pair, the XCD placement on or off, other conv tile forms, another n-split of the few-component kernels, another
puller count of the HALS pipeline, the stage pipeline instead of the persistent one, the chase on or off and behind other CU masks.  The
test hook CMF_TEST_N_CU (with CMF_TEST_HOOKS=1, set here around the creation of a handle and nowhere else) plans a handle for such a
count on the whole chip; cmf_get_counter "plan:n_cu" says what the plan used.

On the integer problems of tests/exact_problems.py every contraction is exact in fp32 IN ANY SUMMATION ORDER, so nothing the other exact
files assert depends on the plan, and their assertions are made here unchanged, by their own code (run_mu_config, run_masked_config,
run_pgd_config, run_divergence_config, run_spotlight, run_hals_row) with every bar theirs.  In addition, per handle:

  * plan:n_cu is the count asked for;
  * where num and den are exact (MU, masked MU, PGD) W and H are BIT-IDENTICAL to the same configuration on a handle made without the
    hook;
  * the launch counters show the branch the plan mirrors of exact_problems (conv3_form, conv_small_form, small_k_plan, hxt_chunks,
    tc_plan, hals_plan, called with that count) predict, and the branch the row was chosen for: a row that does not take it fails.

Counts: 128, 64, 32 (the partition sizes: the whole table exact_problems.CU_SHAPES, which reaches every count-dependent path at each of
them -- the last test); 1 (the degenerate plan: one chunk, whole tiles only, one piece) and 38 (no multiple of 4: no XCD placement, no
chase) on the small rows.  The conv families' epilogues (masked MU, PGD, Itakura-Saito, masked KL, and Itakura-Saito and beta = 0.5
under the mask -- the sentinel families, handed junk under the mask) run at 32 CUs on one row per tile form.
The MU rule under seqNMF's cross-orthogonality penalties (run_xortho_config of tests/test_gpu_exact_xortho.py) runs on those rows too, and
at every count on the rows of exact_problems.xo_cu_rows: the penalty contraction is a one-source C2 launch with G as the left operand,
chunked by its own plan, whose tail rows the slab sum reads out of G, and its H side sums as many C3 slabs as the count's plan makes.
HALS (exact_problems.CU_HALS_SHAPES): 2, 3 and 4 pullers by the count, the fall to the stage pipeline at K = 32 on 64 CUs, the chased
form with 32 CUs beside the pipeline (128 CUs, two pullers; the whole chip leaves 128), and 134 CUs, where every condition of the chase
holds but the count is no multiple of 8 and the chase must be off.

One lost term of a contraction moves num or den by one unit, at least 8 ulp against a bar of 2 (exact_problems' module text): a chunk
seam, a dealing or a cut-tile error of one of these plans fails the oracle check by a factor of four, and the bit-identity with the
whole-chip plan at any size."""
import ctypes
import os
import time

import numpy as np
import pytest

import exact_problems as ep
import test_exact_parity as mu
import test_gpu_divergence_paths as dv
import test_gpu_exact_hals as hals
import test_gpu_exact_masked_mu as mm
import test_gpu_exact_pgd as pgd
import test_gpu_exact_xortho as xo
from exact_problems import CU_COUNTS, CU_EPILOGUE_FORMS, CU_EPILOGUE_N_CU, CU_EPILOGUE_ROWS, CU_FULL, CU_HALS_SHAPES, CU_PATHS, CU_SHAPES, L1, L2, LAUNCH_PATHS

pytestmark = pytest.mark.gpu

_seen = {n: {} for n in CU_COUNTS}   # launches:<path> per count, summed over the MU handles of the table
_done = set()
_refs = {}                           # the fp64 references, once per (kind, shape), shared across the counts
_plain = {}                          # (kind, shape, configuration) -> the factors of the handle made without the hook


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1
    return m


class Planned:
    """The package with every rule constructor run under CMF_TEST_HOOKS=1 and CMF_TEST_N_CU=n_cu -- set around the creation of the
    handle only and restored behind it -- and plan:n_cu of every handle asserted.  Handed to the other files' helpers as `cmf`."""

    RULES = ("MultUpdate", "HALSUpdate", "PGDUpdate")

    def __init__(self, cmf, n_cu):
        self._cmf, self.n_cu, self.handles = cmf, n_cu, 0

    def __getattr__(self, name):
        obj = getattr(self._cmf, name)
        if name not in self.RULES:
            return obj

        def create(*args, **kw):
            old = {k: os.environ.get(k) for k in ("CMF_TEST_HOOKS", "CMF_TEST_N_CU")}
            os.environ["CMF_TEST_HOOKS"] = "1"
            os.environ["CMF_TEST_N_CU"] = str(self.n_cu)
            try:
                rule = obj(*args, **kw)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            try:
                got = rule.counter("plan:n_cu")
                assert got == self.n_cu, f"plan:n_cu is {got}, asked for {self.n_cu}"
            except BaseException:
                rule.close()
                raise
            self.handles += 1
            return rule

        return create


def key(cfg):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()))


def cached(kind, shape, make):
    if (kind, shape) not in _refs:
        _refs[(kind, shape)] = make()
    return _refs[(kind, shape)]


def record(n_cu, c):
    for p, v in c.items():
        _seen[n_cu][p] = _seen[n_cu].get(p, 0) + v


def check_plan(plan, c, what):
    """The launch counters c show every branch outcome the mirrors predict ("name<*>": any instance of the kernel)."""
    for path, want in plan.items():
        got = sum(v for p, v in c.items() if p.startswith(path[:-2])) if path.endswith("*>") else c[path]
        assert (got > 0) == want, f"{what}: the plan mirror says {path} is {'reached' if want else 'not reached'}, the counters say {got}; launches {mu.reached(c)}"


def same_as_plain(got, plain, names, what, cfg, c):
    mu.check_same(got, plain, names, what, cfg, "the handle planned for the whole chip", c)


def short_shards(T, L, cfg):
    return T // len(cfg.get("devices", [0])) < 2 * L  # (shards shorter than two lag windows: not a shape a group takes)


# ---- the MU rule (squared error) --------------------------------------------------------------------------------------------------
def plain_mu_halves(cmf, cfg, r):
    """(W after update_motifs!, H after update_feature_maps!) of the configuration on handles made without the hook."""
    out = []
    for W, H, half in ((r["Ww"], r["Hw"], 0), (r["Wh"], r["Hh"], 1)):
        rule = mu.make_rule(cmf, cfg, r["X"], W, H)
        try:
            rule.update_motifs(l1W=L1, l2W=L2) if half == 0 else rule.update_feature_maps(l1H=L1, l2H=L2)
            out.append(rule.download()[half])
        finally:
            rule.close()
    return out


MU_ROWS = [(n,) + row for n in CU_COUNTS for row in CU_SHAPES[n]]


@pytest.mark.parametrize("n_cu,N,T,K,L,configs,why", MU_ROWS, ids=[f"cu{r[0]}-{r[1]}x{r[2]}x{r[3]}x{r[4]}" for r in MU_ROWS])
def test_exact_mu_paths_under_cu_plans(cmf, oracle, n_cu, N, T, K, L, configs, why):
    shape = (N, T, K, L)
    t0 = time.perf_counter()
    r = cached("mu", shape, lambda: mu.mu_references(oracle, shape))
    t_ref = time.perf_counter() - t0
    planned = Planned(cmf, n_cu)
    for cfg in configs:
        if short_shards(T, L, cfg):
            continue
        Wg, Hg, c = mu.run_mu_config(planned, cfg, r, record=lambda c: record(n_cu, c))
        if ("mu", shape, key(cfg)) not in _plain:
            _plain["mu", shape, key(cfg)] = plain_mu_halves(cmf, cfg, r)
        Wp, Hp = _plain["mu", shape, key(cfg)]
        same_as_plain(Wg, Wp, "knl", f"{n_cu} CUs: W half: W", cfg, c)
        same_as_plain(Hg, Hp, "kt", f"{n_cu} CUs: H half: H", cfg, c)
        what = f"{shape} {cfg} at {n_cu} CUs"
        if "devices" not in cfg:
            check_plan(ep.cu_plan(N, T, K, L, cfg, n_cu), c, what)
        elif cfg.get("halo_in_allreduce") == 1 and K % 32 == 0:
            assert c["transconv_kernel:front_block"] > 0, f"{what}: no shard updated the columns in front of its own; launches {mu.reached(c)}"
        if cfg.get("gram"):
            assert c["gram_w_kernel"] > 0 and c["gram_h_mfma_kernel"] + c["gram_h_kernel"] > 0, f"{what}: not the Gram form; launches {mu.reached(c)}"
        if not cfg:  # what the row is there for at this count, on the configuration without options
            for path in why:
                check_plan({path.lstrip("!"): not path.startswith("!")}, c, f"{what} (the row's purpose)")
    assert planned.handles > 0
    _done.add((n_cu, shape))
    print(f"{n_cu} CUs {shape} {why}: references {t_ref:.2f} s, total {time.perf_counter() - t0:.2f} s, {planned.handles} handles")


# ---- the conv families' epilogues on the replanned conv (32 CUs) ------------------------------------------------------------------
EPI_IDS = [f"{r[0]}x{r[1]}x{r[2]}x{r[3]}" for r in CU_EPILOGUE_ROWS]


def epilogue_configs(configs):
    return [c for c in ep.divergence_configs(configs, "masked") if set(c) <= {"conv_split"}]


@pytest.mark.parametrize("N,T,K,L,configs,why", CU_EPILOGUE_ROWS, ids=EPI_IDS)
def test_masked_mu_under_cu_plan(cmf, N, T, K, L, configs, why):
    shape, n_cu = (N, T, K, L), CU_EPILOGUE_N_CU
    refs = cached("masked", shape, lambda: mm.references(shape))
    mask, X, (Ww, Hw, _), (Wh, Hh, _) = refs
    planned = Planned(cmf, n_cu)
    worst = {"W": 0.0, "H": 0.0}
    for cfg in epilogue_configs(configs):
        Wg, Hg, c = mm.run_masked_config(planned, cfg, refs, record=lambda c: None, worst=worst)
        check_plan({p: v for p, v in ep.cu_plan(N, T, K, L, cfg, n_cu).items() if p.startswith("conv")}, c, f"masked MU {shape} {cfg} at {n_cu} CUs")
        out = []
        for W, H, half in ((Ww, Hw, 0), (Wh, Hh, 1)):
            rule = mm.masked_rule(cmf, cfg, X, W, H, mask)
            try:
                rule.update_motifs(l1W=L1, l2W=L2) if half == 0 else rule.update_feature_maps(l1H=L1, l2H=L2)
                out.append(rule.download()[half])
            finally:
                rule.close()
        same_as_plain(Wg, out[0], "knl", f"{n_cu} CUs: masked W half: W", cfg, c)
        same_as_plain(Hg, out[1], "kt", f"{n_cu} CUs: masked H half: H", cfg, c)
    assert planned.handles > 0
    print(f"masked MU {shape} at {n_cu} CUs: worst W {worst['W']:.2f} ulp, H {worst['H']:.2f} ulp")


@pytest.mark.parametrize("N,T,K,L,configs,why", CU_EPILOGUE_ROWS, ids=EPI_IDS)
def test_pgd_under_cu_plan(cmf, oracle, N, T, K, L, configs, why):
    shape, n_cu = (N, T, K, L), CU_EPILOGUE_N_CU
    ref_w = cached("pgdW", shape, lambda: pgd.references(oracle, shape, "W", True))  # (the step-size precondition asserted from the arrays)
    ref_h = cached("pgdH", shape, lambda: pgd.references(oracle, shape, "H", True))
    variants_w = {v: pgd.Variant(cmf, v, ref_w[3]) for v in ref_w[5]}
    variants_h = {v: pgd.Variant(cmf, v, ref_h[3]) for v in ref_h[5]}
    planned = Planned(cmf, n_cu)
    worst = {"W": 0.0, "H": 0.0}
    for cfg in pgd.pgd_configs(epilogue_configs(configs)):
        got, c = pgd.run_pgd_config(planned, cfg, ref_w, ref_h, variants_w, variants_h, record=lambda c: None, worst=worst)
        plain, _ = pgd.run_pgd_config(cmf, cfg, ref_w, ref_h, variants_w, variants_h, record=lambda c: None, worst=worst)
        for (family, v), x in got.items():
            same_as_plain(x, plain[(family, v)], "knl" if family == "W" else "kt", f"{n_cu} CUs: PGD {family} half, {v}", cfg, c)
    assert planned.handles > 0
    print(f"PGD {shape} at {n_cu} CUs: worst W {worst['W']:.2f} ulp, H {worst['H']:.2f} ulp")


@pytest.mark.parametrize("form", CU_EPILOGUE_FORMS)
@pytest.mark.parametrize("N,T,K,L,configs,why", CU_EPILOGUE_ROWS, ids=EPI_IDS)
def test_divergence_forms_under_cu_plan(cmf, N, T, K, L, configs, why, form):
    """The element-wise bars of profiles/mu_divergence_elementwise.txt, the sensitivity condition from the arrays (dv.reference) and the
    spotlight loss at SPOT_BAR, its spotlights on the tiles around the cut of the grid AT THIS COUNT."""
    shape, n_cu = (N, T, K, L), CU_EPILOGUE_N_CU
    refs = cached("div:" + form, shape, lambda: dv.references(form, shape, False))
    planned = Planned(cmf, n_cu)
    base = None
    for cfg in epilogue_configs(configs):
        Wg, Hg, c = dv.run_divergence_config(planned, form, cfg, K, refs, record=lambda form, c: None)
        check_plan({p: v for p, v in ep.cu_plan(N, T, K, L, cfg, n_cu).items() if p.startswith("conv")}, c, f"{form} {shape} {cfg} at {n_cu} CUs")
        if base is None:  # (options that change the conv form alone: the same bits, as in tests/test_gpu_divergence_paths.py)
            base = (cfg, Wg, Hg)
        else:
            dv.check_same(Wg, base[1], "knl", "W half: W", cfg, base[0], c)
            dv.check_same(Hg, base[2], "kt", "H half: H", cfg, base[0], c)
    dv.run_spotlight(planned, N, T, K, L, dict(), form, n_cu=n_cu, record=lambda form, c: None)
    assert planned.handles > 0
    _done.add(("divergence", form, shape))


# ---- the MU rule under seqNMF's cross-orthogonality penalties -----------------------------------------------------------------------
def xortho_under_plan(cmf, n_cu, shape, configs):
    """run_xortho_config of tests/test_gpu_exact_xortho.py (all three weights; every bar its own) on handles planned for n_cu CUs, the
    factors bit-identical to the same configuration on the whole-chip plan.  Returns the launch counters per configuration."""
    refs = cached("xortho", shape, lambda: xo.xortho_references(shape))
    planned = Planned(cmf, n_cu)
    worst = {"W": 0.0, "H": 0.0}
    out = []
    for cfg in configs:
        Wg, Hg, c = xo.run_xortho_config(planned, cfg, refs, record=lambda c: None, worst=worst)
        if ("xortho", shape, key(cfg)) not in _plain:
            _plain["xortho", shape, key(cfg)] = xo.run_xortho_config(cmf, cfg, refs, record=lambda c: None, worst=worst)[:2]
        Wp, Hp = _plain["xortho", shape, key(cfg)]
        same_as_plain(Wg, Wp, "knl", f"{n_cu} CUs: penalised W half: W", cfg, c)
        same_as_plain(Hg, Hp, "kt", f"{n_cu} CUs: penalised H half: H", cfg, c)
        out.append((cfg, c))
    assert planned.handles > 0
    print(f"penalised MU {shape} at {n_cu} CUs: worst W {worst['W']:.2f} ulp, H {worst['H']:.2f} ulp")
    return out


@pytest.mark.parametrize("N,T,K,L,configs,why", CU_EPILOGUE_ROWS, ids=EPI_IDS)
def test_xortho_under_cu_plan(cmf, N, T, K, L, configs, why):
    """One row per conv tile form and two few-component rows at 32 CUs: the conv forms and the few-component plans the replanned
    handle takes are those the mirrors predict."""
    n_cu = CU_EPILOGUE_N_CU
    for cfg, c in xortho_under_plan(cmf, n_cu, (N, T, K, L), epilogue_configs(configs)):
        plan = {p: v for p, v in ep.cu_plan(N, T, K, L, cfg, n_cu).items() if p.startswith("conv") or p.startswith("g_gemm") or p == "transconv_kernel:xcd"}
        check_plan(plan, c, f"penalised MU {(N, T, K, L)} {cfg} at {n_cu} CUs")


XO_CU_ROWS = [(n,) + row for n in CU_COUNTS for row in ep.xo_cu_rows(n)]


@pytest.mark.parametrize("n_cu,N,T,K,L", XO_CU_ROWS, ids=[f"cu{r[0]}-{r[1]}x{r[2]}x{r[3]}x{r[4]}" for r in XO_CU_ROWS])
def test_xortho_tails_and_slabs_under_cu_plans(cmf, n_cu, N, T, K, L):
    """The chunk tails of the penalty contraction read G where the rule's read H (CmfHxtTail's left operand), and xo_h_tables sums as many
    C3 slabs as the plan of the count makes: at every count the count's own tail row, a row whose ONE-source chunks leave a tail as well,
    and a row of more than one slab -- which row is which is read off the plan mirrors called with that count."""
    p = ep.xo_cu_predicates(N, T, K, L, n_cu)
    for cfg, c in xortho_under_plan(cmf, n_cu, (N, T, K, L), [dict()]):
        what = f"penalised MU {(N, T, K, L)} at {n_cu} CUs"
        # both launches run in every W phase: the rule's two-source one and the penalty contraction's one-source one
        assert c["hxt_kernel:nsrc1"] > 0 and c["hxt_kernel:nsrc2"] > 0, f"{what}: launches {mu.reached(c)}"
        check_plan({"hxt_kernel:tail": p["tail"] or p["left_tail"], "hxt_kernel:no_tail": not (p["tail"] and p["left_tail"])}, c, what)
    _done.add(("xortho", n_cu, (N, T, K, L)))


# ---- HALS -----------------------------------------------------------------------------------------------------------------------------
HALS_ROWS = [(n,) + row for n in CU_HALS_SHAPES for row in CU_HALS_SHAPES[n]]


@pytest.mark.parametrize("n_cu,N,T,K,L,configs", HALS_ROWS, ids=[f"cu{r[0]}-{r[1]}x{r[2]}x{r[3]}x{r[4]}" for r in HALS_ROWS])
def test_exact_hals_paths_under_cu_plans(cmf, n_cu, N, T, K, L, configs):
    """Everything tests/test_gpu_exact_hals.py asserts -- the element-wise bars of profiles/exact_hals.txt, the zero pattern, the loss
    bar, EXACTLY the launch names the plan mirror expects at this count, bit-identity of two runs and across hals_gram = 2, 0 and 1, no
    hals_pipeline_reruns -- on handles planned for n_cu CUs."""
    shape = (N, T, K, L)
    assert shape in [s[:4] for s in ep.HALS_SHAPES]  # (the bars are made from the rows of that table)
    for cfg, P, chased in configs:  # the row is there for this plan (tests/test_exact_problems.py holds the table to the mirror as well)
        plan = ep.hals_plan(N, T, K, L, cfg, n_cu=n_cu)
        assert (plan["P"], plan["chase"] > 0) == (P, chased), (shape, cfg, n_cu, plan)
    refs = cached("hals", shape, lambda: hals.references(shape))
    planned = Planned(cmf, n_cu)
    seen = {}
    failures = hals.run_hals_row(planned, shape, [cfg for cfg, _, _ in configs], refs, n_cu=n_cu, seen=seen, worst={}, worst_loss=[0.0])
    assert not failures, "\n".join(failures)
    assert planned.handles > 0
    _done.add(("hals", n_cu, shape))
    print(f"HALS {shape} at {n_cu} CUs: {sorted(p for p, v in seen.items() if v)}")


# ---- the hook itself ------------------------------------------------------------------------------------------------------------------
def test_cu_counts_the_hook_refuses_and_the_hook_without_test_hooks(cmf):
    """With the hooks on, 0 and one more than the device has are CMF_ERR_ARG, no handle is made and cmf_last_error names the variable --
    for a single handle and for a group; without CMF_TEST_HOOKS the variable does nothing."""
    lib = cmf.load_library()
    N, T, K, L = 30, 200, 5, 7
    W, H, X = ep.make_problem(N, T, K, L, "W")
    rule = cmf.MultUpdate(X, W, H)
    try:
        real = rule.counter("plan:n_cu")
    finally:
        rule.close()
    assert real >= 1
    assert "CMF_TEST_HOOKS" not in os.environ and "CMF_TEST_N_CU" not in os.environ
    devs = (ctypes.c_int * 2)(0, 0)
    try:
        os.environ["CMF_TEST_HOOKS"] = "1"
        for bad in (0, -3, real + 1):
            os.environ["CMF_TEST_N_CU"] = str(bad)
            for create in (lambda h: lib.cmf_create(ctypes.byref(h), 0, N, T, K, L, cmf.host.ptr(X)),
                           lambda h: lib.cmf_create_multi(ctypes.byref(h), 2, devs, 0, N, T, K, L, cmf.host.ptr(X))):
                h = ctypes.c_void_p(12345)
                rc = create(h)
                msg = lib.cmf_last_error().decode()
                if rc == 0:
                    lib.cmf_destroy(h)
                assert rc == 1 and not h.value, f"CMF_TEST_N_CU={bad}: return code {rc}, handle {h.value}"
                assert "CMF_TEST_N_CU" in msg and str(bad) in msg, msg
            with pytest.raises(cmf.CMFError) as ei:
                cmf.MultUpdate(X, W, H)
            assert ei.value.code == 1
        os.environ["CMF_TEST_N_CU"] = str(real)  # (the device's own count is a count like any other)
        rule = cmf.MultUpdate(X, W, H)
        try:
            assert rule.counter("plan:n_cu") == real
        finally:
            rule.close()
        os.environ.pop("CMF_TEST_HOOKS")
        os.environ["CMF_TEST_N_CU"] = "32"
        for devices in (None, [0, 0]):
            rule = cmf.MultUpdate(X, W, H, devices=devices)
            try:
                assert rule.counter("plan:n_cu") == real, "CMF_TEST_N_CU counted without CMF_TEST_HOOKS=1"
            finally:
                rule.close()
    finally:
        os.environ.pop("CMF_TEST_N_CU", None)
        os.environ.pop("CMF_TEST_HOOKS", None)
    planned = Planned(cmf, 32)  # a group: the value of its shards; a long recording sharded automatically: every shard's
    for devices in (None, [0, 0, 0]):
        rule = planned.MultUpdate(X, W, H, devices=devices)
        rule.close()
    os.environ["CMF_MAX_COLUMNS"] = "60"
    try:
        rule = planned.MultUpdate(X, W, H)
        try:
            assert rule.counter("allreduce_calls") >= 0  # (a group's counter: the recording was cut into shards)
        finally:
            rule.close()
    finally:
        os.environ.pop("CMF_MAX_COLUMNS", None)
    assert "CMF_TEST_HOOKS" not in os.environ and "CMF_TEST_N_CU" not in os.environ


def test_every_count_dependent_path_reached_at_every_partition_size():
    """For each of 128, 64 and 32 CUs the union of launches:* over its rows reaches every path whose choice depends on the count."""
    for n in CU_FULL:
        print(n, {p: _seen[n].get(p, 0) for p in LAUNCH_PATHS if _seen[n].get(p)})
    want = {(n, row[:4]) for n in CU_COUNTS for row in CU_SHAPES[n]} | {("hals", n, row[:4]) for n in CU_HALS_SHAPES for row in CU_HALS_SHAPES[n]}
    want |= {("divergence", form, row[:4]) for form in CU_EPILOGUE_FORMS for row in CU_EPILOGUE_ROWS}  # every epilogue form on every epilogue row
    if not want <= _done:
        pytest.skip("runs after the whole table (the file as a whole)")
    for n in CU_FULL:
        missing = [p for p in CU_PATHS if not _seen[n].get(p)]
        assert not missing, f"at {n} CUs no row reached {missing}"
