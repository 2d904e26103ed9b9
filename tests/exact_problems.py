"""Integer-valued MU problems on which every contraction is exact in fp32 (tests/test_exact_parity.py, and its CPU half in
tests/test_exact_problems.py).

The MU rule's contractions (est, numW, denomW, numH, denomH, the loss tile sums, the lagged Gram tables) are sums of
non-negative products.  With W, H and X small integers every product is exact in fp32, and so is every partial sum, in any
order, while the exact total stays below 2^24: the fp64 oracle and every GPU path then agree bit for bit on all of them, and
the only rounding left is the element-wise update (cmf_kernels.h cmf_mu: one division, one multiply).

Two families, so that the factor being updated is dense and each of its entries sees every term:
  "W" (the W half): W dense in {1, 2}; H one nonzero (1) per column t, at a hashed component;
  "H" (the H half): H dense in {1, 2}; W one nonzero (1) per (n, l), at a hashed component;
  both: X in {0 ... 40}.
Dropping or doubling any time row, column, lag or component block then moves some num or den by at least 1, and
preconditions() bounds every num / den by 2^20, so such an error is at least 8 ulp of fp32.

The shape table SHAPES is shared with tests/test_gpu_divergence_paths.py, which holds the divergence forms of the rule to their fp64
restatements element by element on the same factors, the Itakura-Saito and beta forms under a 0/1 mask among them (make_divergence_problem, divergence_half, sensitivity, check_elementwise below),
and with tests/test_gpu_exact_masked_mu.py and tests/test_gpu_exact_pgd.py, which hold the MU rule under a 0/1 mask and the PGD rule to
their references on it (mu_mask, make_pgd_problem, pgd_half, pgd_preconditions).  The last section holds the HALS sweeps' own table
(HALS_SHAPES), the mirror of their plan, their element-wise check and the mutations of their restatement (tests/test_gpu_exact_hals.py),
and behind it the MU rule under seqNMF's cross-orthogonality penalties on the shape table (xortho_half, xortho_preconditions,
xortho_mutations: tests/test_gpu_exact_xortho.py).
"""
import numpy as np

XMAX = 40
L1, L2 = 0.5, 0.25  # dyadic: (den + l1) + 2*l2*x is exact in fp32 as well
EXACT = 2 ** 24     # fp32 integers are exact up to here
SENS = 2 ** 20      # max(num, den) at most this: one unit >= 8 ulp
N_CU = 256          # CUs of an MI355X (the plan rules below)


def _hash(*idx, salt=0):
    """A fixed integer hash of broadcast index arrays (splitmix64 finaliser): the same problem on every machine."""
    with np.errstate(over="ignore"):
        z = np.uint64(0x9E3779B97F4A7C15) * np.uint64(salt + 1)
        for i in idx:
            z = (z ^ np.asarray(i, dtype=np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            z = z ^ (z >> np.uint64(31))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(27))
    return z


def components_of_t(T, K, seed=0):
    """W family: the component of H's one nonzero in column t."""
    return (_hash(np.arange(T), salt=seed * 4 + 1) % np.uint64(K)).astype(np.int64)


def components_of_nl(N, L, K, seed=0):
    """H family: the component of W's one nonzero at (n, l), as an (N, L) array."""
    n, l = np.meshgrid(np.arange(N), np.arange(L), indexing="ij")
    return (_hash(n, l, salt=seed * 4 + 2) % np.uint64(K)).astype(np.int64)


def _data_hash(N, T, seed=0):
    """The hash X is drawn from, as an (N, T) array of uint64."""
    nn, tt = np.meshgrid(np.arange(N), np.arange(T), indexing="ij")
    return _hash(nn, tt, salt=seed * 4)


def make_problem(N, T, K, L, family, seed=0):
    """(W (K, N, L), H (K, T), X (N, T)) in float64, Fortran order, integer-valued (family "W" or "H": see the module doc)."""
    k, n, l = np.meshgrid(np.arange(K), np.arange(N), np.arange(L), indexing="ij")
    if family == "W":
        W = 1.0 + (_hash(k, n, l, salt=seed * 4 + 3) & np.uint64(1)).astype(np.float64)
        H = np.zeros((K, T))
        H[components_of_t(T, K, seed), np.arange(T)] = 1.0
    elif family == "H":
        kk, tt = np.meshgrid(np.arange(K), np.arange(T), indexing="ij")
        H = 1.0 + (_hash(kk, tt, salt=seed * 4 + 3) & np.uint64(1)).astype(np.float64)
        W = (k == components_of_nl(N, L, K, seed)[None]).astype(np.float64)
    else:
        raise ValueError(family)
    X = (_data_hash(N, T, seed) % np.uint64(XMAX + 1)).astype(np.float64)
    return np.asfortranarray(W), np.asfortranarray(H), np.asfortranarray(X)


def preconditions(N, T, K, L, family, seed=0):
    """Closed-form bounds from the construction (no contraction is formed): the exact totals of every fp32 accumulation the
    MU paths make, and max(num, den) of the factor the family updates.  Returns a dict of bounds and flags:
      exact      est, numW/denomW (W family) or numH/denomH (H family), transconv(W, X) and the lagged Gram tables < 2^24
      sensitive  max(num, den) <= 2^20
      loss_exact the 64 x 64 loss tile sums (est - X)^2 of the conv epilogues (cmf_kernels.h conv epilogues) <= 2^24
    """
    est_max = 2 * min(L, T)  # every column of est sums at most min(L, T) products of 1 and an entry <= 2
    b = {}
    if family == "W":
        cnt = np.bincount(components_of_t(T, K, seed), minlength=K).max()  # columns of H owned by one component
        b["num"] = XMAX * cnt            # numW[k, n, l] = sum over those columns of X
        b["den"] = est_max * cnt         # denomW[k, n, l] = ... of est
        b["transconv"] = XMAX * 2 * N * L  # sum_{n, l} W[k, n, l] X[n, t + l]
        b["gram"] = cnt                  # HH[k, k', d] = sum_t H[k, t] H[k', t + d]
    else:
        cnt = np.bincount(components_of_nl(N, L, K, seed).ravel(), minlength=K).max()  # (n, l) pairs owned by one component
        b["num"] = XMAX * cnt            # numH[k, t] = sum over those pairs of X
        b["den"] = est_max * cnt         # denomH[k, t] = ... of est
        b["transconv"] = XMAX * cnt
        b["gram"] = max(cnt, 4 * T)      # lag-Gram taps of W (<= pairs per component), HH of a dense H (<= 4 T)
    b["est"] = est_max
    b["loss_tile"] = 64 * 64 * max(est_max, XMAX) ** 2
    b["exact"] = max(b["est"], b["num"], b["den"], b["transconv"], b["gram"]) < EXACT
    b["sensitive"] = max(b["num"], b["den"]) <= SENS
    b["loss_exact"] = b["loss_tile"] <= EXACT
    return b


def ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (got: float32 results, ref: the fp64 oracle), element-wise."""
    ref = np.asarray(ref, dtype=np.float64)
    sp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / sp


def first_bad(mask, names):
    """'k=.., n=.., l=..' of the first True entry of mask (Julia's (K, N, L) / (K, T) order), or None."""
    idx = np.argwhere(mask)
    if len(idx) == 0:
        return None
    return ", ".join(f"{a}={int(v)}" for a, v in zip(names, idx[0]))


# The launch paths of cmf_get_counter "launches:<path>" (csrc/cmf_internal.h kLaunchNames, in its order): the coverage test of
# tests/test_exact_parity.py expects every one reached (tests/test_gpu_divergence_paths.py: every one a divergence form can reach), and tests/test_exact_problems.py keeps this list equal to the C++ table.
LAUNCH_PATHS = [
    "conv_kernel", "conv2_kernel", "conv3_kernel:whole", "conv3_kernel:whole+4", "conv3_kernel:whole+16", "conv3_kernel:pieces4",
    "conv3_kernel:pieces16", "conv_small_kernel<1>", "conv_small_kernel<2>", "conv_small_kernel<3>", "conv_small_kernel<4>",
    "conv_small_kernel<6>", "conv_small_kernel<8>", "conv_small_kernel:quarter", "conv_small_kernel:pre", "conv_small_kernel:whole",
    "hxt_kernel<1>",
    "hxt_kernel<2>", "hxt_kernel<3>", "hxt_kernel<4>", "hxt_kernel<5>", "hxt_kernel<6>", "hxt_kernel<8>", "hxt_kernel:nsrc1",
    "hxt_kernel:nsrc2", "hxt_kernel:tail", "hxt_kernel:no_tail", "transconv_kernel<4>", "transconv_kernel<8>",
    "transconv_kernel<12>", "transconv_kernel<16>", "transconv_kernel<20>", "transconv_kernel<24>", "transconv_kernel<28>",
    "transconv_kernel<32>", "transconv_kernel:front_block", "transconv_kernel:xcd", "hxt_small_kernel<1>", "hxt_small_kernel<2>",
    "hxt_small_kernel<3>", "hxt_small_kernel<4>", "hxt_small_kernel<5>", "hxt_small_kernel<6>", "hxt_small_kernel<7>",
    "hxt_small_kernel<8>", "hxt_small_kernel<9>", "hxt_small_kernel<10>", "hxt_small_kernel<1,RV>", "hxt_small_kernel<2,RV>",
    "hxt_small_kernel<3,RV>", "g_gemm_fold_small_kernel<1>", "g_gemm_fold_small_kernel<2>", "g_gemm_fold_small_kernel<3>",
    "g_gemm_fold_small_kernel<4>", "g_gemm_fold_small_kernel<5>", "g_gemm_fold_small_kernel<6>",
    "g_gemm_fold_small_kernel<1,RV>", "g_gemm_fold_small_kernel<2,RV>", "g_gemm_fold_small_kernel<3,RV>",
    "g_gemm_fold_small_kernel:split", "g_gemm_fold_small_kernel:fused_h", "gram_w_kernel", "gram_lag_corr", "gram_w_taps",
    "gram_h_mfma_kernel", "gram_h_kernel", "slab_sum_kernel", "slab_sum_kernel:carry", "slab_sum_small_kernel",
    "slab_sum_small_kernel:carry", "halo_pack2_kernel", "halo_unpack2_kernel", "halo_pack3_kernel", "halo_unpack3_kernel",
]


# ---- the plan rules of cmf_api.hip plan() / cmf_internal.h launch_conv, restated for choosing and describing shapes -------
def rup(a, b):
    return (a + b - 1) // b * b


HXT_LP = (1, 2, 3, 4, 5, 6, 8)


def hxt_lp(L):
    best, bestP = 1, 1 << 30
    for lp in HXT_LP:
        P = rup(L, 2 * lp)
        if P < bestP or (P == bestP and lp > best):
            best, bestP = lp, P
    return best


def transconv_lt(L):
    return rup(L, 4) if L <= 32 else 32


def conv3_cut(N, T, conv_split=1, n_cu=N_CU):
    """(whole tiles, cut tiles, pieces per cut tile) of a conv3_kernel launch over T columns (cmf_internal.h conv_tail_cut)."""
    tiles, slots = rup(N, 128) // 64 * ((T + 63) // 64), 12 * n_cu
    rem, cut = tiles % slots, 0
    if conv_split:
        if 0 < rem <= 3 * n_cu:
            cut = rem
        if tiles // slots >= 4:
            cut += 3 * n_cu
        cut = min(cut, tiles)
    return tiles - cut, cut, 16 if (0 < cut < n_cu and conv_split != 4) else 4


def conv3_form(N, T, conv_split=1, n_cu=N_CU):
    """The conv3_kernel grid form of a tensor_conv launch that reads data (K a multiple of 32): "whole", "whole+4",
    "whole+16", "pieces4" or "pieces16"."""
    gx3, rows = rup(N, 128) // 64, (T + 63) // 64
    tiles, slots = gx3 * rows, 12 * n_cu
    rem, cut = tiles % slots, 0
    if conv_split:
        if 0 < rem <= 3 * n_cu:
            cut = rem
        if tiles // slots >= 4:
            cut += 3 * n_cu
        cut = min(cut, tiles)
    if cut == 0:
        return "whole"
    pieces = 16 if (cut < n_cu and conv_split != 4) else 4
    return ("whole+" if cut < tiles else "pieces") + str(pieces)


def small_k_plan(N, T, K, L, n_cu=N_CU, with_c3_ok=False):
    """(C2 MBW, C2 RV, C3 MBW, C3 RV, C3 pieces NS, conv k pairs) of the few-component kernels (K <= 16, L <= 64); with_c3_ok: (NS,
    whether the few-component C3 kernel runs) instead."""
    J = L * K
    mblocks = (J + 31) // 32
    MG = (mblocks + 9) // 10
    MBW = (mblocks + MG - 1) // MG
    RV = 0
    if MG == 1 and 2 <= MBW <= 4 and 1 <= J % 32 <= 4:
        RV, MBW = J % 32, MBW - 1
    MG3 = (K * L + 32 * 6 - 1) // (32 * 6)
    while True:
        Kg = (K + MG3 - 1) // MG3
        if Kg * L <= 32 * 6:
            break
        MG3 += 1
    MG3 = (K + Kg - 1) // Kg
    MBW3 = (Kg * L + 31) // 32
    RV3 = 0
    if MG3 == 1 and 2 <= MBW3 <= 4 and 1 <= (Kg * L) % 32 <= 4 and (8 * ((rup(N, 2) + 7) // 8) + 2) * 4 <= 32 * 132:
        RV3, MBW3 = (Kg * L) % 32, MBW3 - 1
    TG = rup(T + L - 1, 128)
    waves = (TG // 32) * MG3 * 2
    rounds = (rup(N, 2) + 7) // 8
    ns = max(1, min(8, (8 * n_cu + waves - 1) // waves, max(1, rounds // 8)))
    rps = (rounds + ns - 1) // ns
    NS = (rounds + rps - 1) // rps
    if with_c3_ok:  # (the few-component C3 runs at all: at least two waves per CU, else the general transconv_kernel)
        return NS, waves * NS >= 2 * n_cu
    return MBW, RV, MBW3, RV3, NS, (K + 1) // 2


# ---- the shape table of the two GPU files (tests/test_exact_parity.py, tests/test_gpu_divergence_paths.py) ------------------
GROUPS = [dict(devices=[0] * R, halo_in_allreduce=hal) for R in (2, 3, 8) for hal in (0, 1)]
CONV32 = [dict(), dict(conv_kernel=2), dict(conv_kernel=3), dict(conv_split=0), dict(conv_split=4)]
FULL32 = CONV32 + [dict(gram=1), dict(gram=2), dict(reuse_est=0)] + GROUPS
GENERAL = [dict(), dict(conv_split=0), dict(gram=1), dict(gram=2), dict(reuse_est=0), dict(devices=[0] * 2), dict(devices=[0] * 3, gram=1)]
SMALL = ([dict(), dict(small_k=0), dict(reuse_est=0), dict(gram=1)] + [dict(small_k=s, small_k_fuse=f) for s in (1, 2) for f in (0, 1, 2)]
         + [dict(devices=[0] * 2), dict(devices=[0] * 3, small_k=2, small_k_fuse=2)])

# (N, T, K, L, configurations, why)
SHAPES = [
    # conv3_kernel grid forms (K = 32, L = 20)
    (130, 700, 32, 20, FULL32, "conv3 pieces only, 16 pieces (44 tiles)"),
    (1001, 2500, 32, 20, CONV32 + [dict(gram=1)], "conv3 pieces only, 4 pieces (640 tiles)"),
    (2000, 3000, 32, 20, CONV32 + [dict(gram=1), dict(devices=[0] * 2, halo_in_allreduce=1)], "whole tiles only (1504 tiles)"),
    (2000, 6250, 32, 20, CONV32, "whole + 16 pieces (3136 tiles: the T/8 shard), hxt tail rows"),
    (2000, 6720, 32, 20, CONV32, "whole + 4 pieces (3360 tiles)"),
    # hxt_kernel<LP> / transconv_kernel<LT> instances on the general kernels (K > 16, not a multiple of 32: conv_kernel)
    (70, 600, 20, 2, GENERAL, "LP 1, LT 4"),
    (70, 600, 20, 4, GENERAL, "LP 2, LT 4"),
    (70, 600, 20, 6, GENERAL, "LP 3, LT 8"),
    (70, 600, 20, 8, GENERAL, "LP 4, LT 8"),
    (70, 600, 20, 10, GENERAL, "LP 5, LT 12"),
    (70, 600, 20, 12, GENERAL, "LP 6, LT 12"),
    (70, 600, 20, 16, GENERAL, "LP 8, LT 16"),
    (70, 600, 20, 22, GENERAL, "LP 1, LT 24"),
    (70, 600, 20, 26, GENERAL, "LP 1, LT 28"),
    (70, 600, 20, 31, GENERAL, "LP 8, LT 32"),
    (70, 600, 20, 40, GENERAL, "LP 5, LT 32 (L > 32)"),
    (200, 1500, 32, 33, [dict(), dict(conv_split=0)], "LP 1 at L = 33, K = 32"),
    (40, 40, 20, 16, GENERAL, "a recording shorter than one Gram tile past the lag window: gram_h_kernel"),
    (30, 24, 32, 12, [dict(), dict(gram=1)], "T shorter than 2 L"),
    # few components (K <= 16): C2 m blocks 1 .. 10 and 1 .. 3 + VALU rows, C3 1 .. 6 and 1 .. 3 + VALU rows, conv k pairs 1 .. 8
    (90, 610, 5, 7, SMALL, "C2 / C3 1 block + VALU rows"),
    (31, 420, 2, 33, SMALL, "C2 / C3 2 blocks + VALU rows, 1 k pair"),
    (250, 1500, 5, 20, SMALL, "C2 / C3 3 blocks + VALU rows, C3 in 4 pieces"),
    (48, 300, 4, 8, SMALL, "C2 / C3 1 block, 2 k pairs"),
    (70, 257, 5, 10, SMALL, "C2 / C3 2 blocks, 3 k pairs"),
    (300, 260, 13, 7, SMALL, "C2 / C3 3 blocks, 7 k pairs, C3 in 4 pieces"),
    (10, 64, 8, 16, SMALL, "C2 / C3 4 blocks, 4 k pairs"),
    (33, 400, 7, 19, SMALL, "C2 / C3 5 blocks"),
    (65, 520, 11, 12, SMALL, "C2 5 blocks, 6 k pairs"),
    (60, 400, 8, 22, SMALL, "C2 6 blocks"),
    (60, 400, 10, 20, SMALL, "C2 7 blocks"),
    (17, 150, 16, 64, SMALL, "C2 8 blocks, C3 6 blocks, L = 64"),
    (60, 400, 14, 20, SMALL, "C2 9 blocks"),
    (130, 700, 16, 20, SMALL, "C2 10 blocks, 8 k pairs, C3 in 2 pieces"),
    # whole few-component tiles: 16 x 65 = 1040 tiles on 1024 SIMDs, 1024 whole tiles and a tail of 16 in quarter pieces
    # (K = 8, L = 10 and not K = 5, L = 20: N L / K = 1250 terms per sum of the H half, as on the K = 32 rows above; with 4000 one term
    #  of a divergence form's sums is no longer 4 element-wise bars of its element -- exact_problems.sensitivity)
    (1000, 4100, 8, 10, [dict(), dict(small_k=0), dict(reuse_est=0), dict(conv_split=0), dict(small_k=2, small_k_fuse=2)],
     "whole few-component tiles + quarter-piece tail, preloaded data tile"),
]


def conv_small_form(N, T, conv_split=1, n_cu=N_CU):
    """(whole tiles, quarter-cut tiles) of a few-component conv launch over T columns (cmf_internal.h launch_conv)."""
    tiles, per_round = rup(N, 128) // 64 * ((T + 63) // 64), 4 * n_cu
    rem = tiles % per_round
    cut = rem if (conv_split and tiles >= per_round and 0 < rem <= per_round // 4) else 0
    if conv_split and tiles < per_round:
        cut = tiles
    return tiles - cut, cut


def hxt_chunks(N, T, K, L, nsrc=2, n_cu=N_CU):
    """(time chunks, rows per chunk, rows the chunks cover) of a C2 launch over nsrc sources (cmf_api.hip plan(): chunks).  Rows covered
    < T: the rows behind the last whole ring rotation are left to the slab sum ("hxt_kernel:tail")."""
    lp = hxt_lp(L)
    groups = rup(L, 2 * lp) // (2 * lp)
    slots = 4 * n_cu * (2 if lp <= 5 else 1)
    per_chunk = rup(N, 128) // 32 * nsrc * ((K + 31) // 32) * groups
    unit = 6 * lp
    nch = max(1, (slots + per_chunk // 2) // per_chunk)
    units_all, units_whole = (T + unit - 1) // unit, T // unit
    per, main = (units_all + nch - 1) // nch, T
    if units_whole > 0 and (units_whole + nch - 1) // nch < per:
        per, main = (units_whole + nch - 1) // nch, units_whole * unit
    return (main + per * unit - 1) // (per * unit), per * unit, main


def tc_plan(N, T, K, nsrc=2, n_cu=N_CU, extra_blocks=0):
    """(waves W, fragment slabs F, XCD placement) of a C3 launch over nsrc sources (cmf_api.hip plan(): tc_plan)."""
    C = rup(N, 8) // 8
    U = ((T + 127) // 128 + extra_blocks) * ((K + 31) // 32) * nsrc * C
    W = min(8 * n_cu, U)
    F = 1
    for w in range(W):
        pr = (w * U // W) // C
        F = max(F, w - ((pr * C + 1) * W - 1) // U + 1)
    return W, F, W >= 64 and W % 32 == 0


# ---- the same kernel paths under plans for fewer compute units (tests/test_gpu_exact_cu_plans.py) ------------------------------
# Every plan rule above is a function of the CU count the device reports; a partitioned MI355X shows 128, 64 or 32.  The library's test
# hook CMF_TEST_N_CU plans a handle for such a count on the whole chip.  The integer problems are exact in any summation order, so the
# assertions of tests/test_exact_parity.py hold unchanged under every plan, and the bits must be those of the handle planned for the
# whole chip.  Rows: (N, T, K, L, configurations, {launch path: reached or not}) -- the paths a row was chosen for AT THAT COUNT, for a
# one-device configuration without options unless the key carries one ("path|option=value"); tests/test_exact_problems.py holds every
# claim to the mirrors, the GPU file to the launch counters.
CU_COUNTS = (128, 64, 32, 1, 38)  # the partition sizes; the degenerate plan; a count that is no multiple of 4 (no XCD placement, no chase)
CU_FULL = (128, 64, 32)           # the counts that run the whole table and must reach CU_PATHS
_G2H, _G3 = dict(devices=[0] * 2, halo_in_allreduce=1), dict(devices=[0] * 3)
_C32 = [dict(), dict(conv_split=0), dict(conv_split=4)]
_SK = [dict(), dict(small_k=0), dict(conv_split=0), dict(small_k=2, small_k_fuse=2)]


_TAIL_T = {128: 961, 64: 481, 32: 481, 38: 301, 1: 448}  # the shortest recordings of 130 units whose C2 chunks leave tail rows to the slab sum


def _cu_rows(n_cu):
    """The rows of one count: the K = 32, L = 20 rows scale with the count (a conv3 form is a statement about tiles per CU), the
    few-component and general rows are the same shapes taking other branches.  The last entry names what the row is there for at
    that count; cu_plan says which branches it takes."""
    s = n_cu // 32
    one = n_cu == 1
    rows = [
        (130, 448, 32, 20, _C32 + [dict(gram=1), dict(gram=2), _G2H, _G3], ["conv3_kernel:whole", "hxt_kernel:tail"] if one else ["conv3_kernel:pieces16"]),
        (130, 700, 32, 20, _C32, ["conv3_kernel:whole"] if one else ["conv3_kernel:pieces4" if n_cu <= 44 else "conv3_kernel:pieces16"]),
        (250, 1500, 32, 20, [dict(), _G2H], ["conv3_kernel:whole+4"] if one else ["transconv_kernel:xcd"] if n_cu % 4 == 0 else ["!transconv_kernel:xcd"]),
        (70, 600, 20, 10, [dict(), dict(gram=1), dict(gram=2), dict(devices=[0] * 2)], ["hxt_kernel:no_tail"]),
        (90, 610, 5, 7, _SK, ["conv_small_kernel:whole"] if one else ["conv_small_kernel:quarter", "conv_small_kernel:pre"]),
        (250, 1500, 5, 20, _SK, ["g_gemm_fold_small_kernel<*>", "!g_gemm_fold_small_kernel:split"] if one else ["g_gemm_fold_small_kernel:split"]),
    ]
    if not one:
        rows.append((130, _TAIL_T[n_cu], 32, 20, [dict()], ["hxt_kernel:tail"]))
    if n_cu in CU_FULL:
        rows += [
            (250, 3200 * s, 32, 20, _C32, ["conv3_kernel:whole", "transconv_kernel:xcd"]),
            (250, 6400 * s, 32, 20, _C32, ["conv3_kernel:whole+16"]),
            (250, 7040 * s, 32, 20, _C32, ["conv3_kernel:whole+4"]),
            (1000, 4100 * n_cu // 256 + 60, 8, 10, _SK, ["conv_small_kernel:whole", "conv_small_kernel:quarter", "conv_small_kernel:pre"]),
            (90, 32 * n_cu, 5, 7, [dict()], ["g_gemm_fold_small_kernel<*>", "!g_gemm_fold_small_kernel:split"]),  # the few-component C3 in ONE piece
        ]
    return rows


CU_SHAPES = {n_cu: _cu_rows(n_cu) for n_cu in CU_COUNTS}
CU_SHAPES[32].append((500, 12800, 32, 20, [dict(), dict(conv_split=0)], ["conv3_kernel:whole+4"]))  # four whole rounds and the extra cut
# what the union over the rows of each of CU_FULL must reach
CU_PATHS = ["conv3_kernel:whole", "conv3_kernel:whole+4", "conv3_kernel:whole+16", "conv3_kernel:pieces4", "conv3_kernel:pieces16",
            "conv_small_kernel:quarter", "conv_small_kernel:pre", "conv_small_kernel:whole", "hxt_kernel:tail", "hxt_kernel:no_tail",
            "transconv_kernel:xcd", "transconv_kernel:front_block", "g_gemm_fold_small_kernel:split", "slab_sum_kernel:carry",
            "gram_w_kernel", "gram_h_mfma_kernel"]


def cu_plan(N, T, K, L, cfg=None, n_cu=N_CU):
    """What the mirrors say a ONE-DEVICE handle of the shape launches under cfg at n_cu: {launch path: True (reached) / False (not)} for
    the paths whose choice depends on the count."""
    cfg = cfg or {}
    split = cfg.get("conv_split", 1)
    out = {}
    small = K <= 16 and L <= 64 and cfg.get("small_k", 1) != 0
    if small:
        whole, cut = conv_small_form(N, T, split, n_cu)
        tiles = whole + cut
        ns, c3 = small_k_plan(N, T, K, L, n_cu, True)
        c3 = c3 or cfg.get("small_k") == 2  # (2: the few-component C3 whatever the plan says)
        out.update({"conv_small_kernel:quarter": cut > 0, "conv_small_kernel:whole": whole > 0,
                    "conv_small_kernel:pre": (K + 1) // 2 <= 4 and tiles <= 16 * n_cu,
                    "g_gemm_fold_small_kernel<*>": c3,  # (any instance: the few-component C3 runs)
                    "g_gemm_fold_small_kernel:split": c3 and ns > 1})
    elif K % 32 == 0:
        out.update({"conv3_kernel:" + f: f == conv3_form(N, T, split, n_cu) for f in ("whole", "whole+4", "whole+16", "pieces4", "pieces16")})
    if not small or cfg.get("gram"):
        nch, clen, main = hxt_chunks(N, T, K, L, 1 if cfg.get("gram") == 1 else 2, n_cu)
        out.update({"hxt_kernel:tail": main < T, "hxt_kernel:no_tail": main == T})
    if not small:
        out["transconv_kernel:xcd"] = tc_plan(N, T, K, 1 if cfg.get("gram") else 2, n_cu)[2]
    return out


# The storing epilogues and the cut tiles' loss partials differ per conv family: the masked MU rule, the PGD rule and the divergence
# forms "is", "kl_mask", "is_mask" and "beta050_mask" run at 32 CUs on one row per conv3 form and two few-component rows (quarter pieces only; whole tiles + tail)
CU_EPILOGUE_N_CU = 32
CU_EPILOGUE_ROWS = [r for r in CU_SHAPES[32] if r[:4] in {(130, 448, 32, 20), (130, 700, 32, 20), (250, 3200, 32, 20), (250, 6400, 32, 20),
                                                         (250, 7040, 32, 20), (90, 610, 5, 7), (1000, 572, 8, 10)}]
CU_EPILOGUE_FORMS = ("is", "kl_mask", "is_mask", "beta050_mask")

# The HALS sweeps under fewer CUs: rows of HALS_SHAPES (the bars of profiles/exact_hals.txt are made from them), each with the sweep
# configurations to run and what hals_plan must say at that count: (cfg, pullers per row -- 0: the stage pipeline --, chased or not).
# 134 is for the chase alone: divisible by 2 but not by 8, and large enough that every other condition of the chase holds.
_CHASE2 = dict(hals_chase=65, hals_persist=2)
CU_HALS_SHAPES = {
    128: [(37, 700, 18, 20, [(dict(), 4, False), (dict(hals_persist=3), 3, False)]),
          (37, 768, 32, 8, [(dict(), 3, False), (dict(hals_persist=2), 2, False)]),         # K = 32: (128 - 32) / 31 = 3 pullers fit
          (37, 1300, 64, 20, [(dict(), 0, False)]),                                       # K = 64: one puller per row fits -- the stage pipeline
          (130, 9000, 32, 20, [(_CHASE2, 2, True), (dict(hals_chase=65), 3, False)])],    # chased with 8 (16 - 12) = 32 CUs beside the pipeline (256 CUs: 128); 3 pullers leave none
    64: [(37, 150, 5, 4, [(dict(), 4, False)]),
         (37, 700, 18, 20, [(dict(), 2, False)]),                                         # (64 - 18) / 17 = 2
         (37, 700, 32, 20, [(dict(), 0, False)])],                                        # K = 32 at 64 CUs: (64 - 32) / 31 = 1 < 2 -- the stage pipeline
    32: [(37, 150, 5, 4, [(dict(), 4, False), (dict(hals_persist=2), 2, False), (dict(hals_persist=3), 3, False)]),
         (37, 700, 18, 20, [(dict(), 0, False)])],
    38: [(37, 150, 5, 4, [(dict(), 4, False)]), (9, 200, 4, 64, [(dict(), 4, False)])],
    134: [(130, 9000, 32, 20, [(_CHASE2, 2, False)])],                                    # 134 / 8 - 12 >= 4 as at 128, but 134 % 8 != 0: no chase
}


# ---- the divergence forms of the MU rule on these problems (tests/test_gpu_divergence_paths.py) ------------------------------
# est = tensor_conv(W, H) is a small integer, exact in fp32 on every conv path, so R, P and Q are element-wise functions of exact
# operands: every conv tile form must store the same bits.  The contractions that follow sum POSITIVE terms of comparable size, so
# the updated factor is compared with the fp64 restatement per element at a relative bar near fp32 rounding
# (profiles/mu_divergence_elementwise.txt, tools/mu_divergence_elementwise.py), far below what one missing term moves (sensitivity).
DIV_XMIN, DIV_XMAX = 16, 31  # strictly positive and narrow: the terms of one sum are comparable
EPS = float(np.finfo(np.float64).eps)
# form -> (divergence kind, beta, masked, accepts zeros, relative data); the names of the `bar` lines of
# profiles/mu_divergence_elementwise.txt.  Relative data (make_divergence_problem): at the left edge of a recording est counts up from
# 1 to its bulk value near 1.5 L, and P = data e^(beta - 2) of the forms with beta < 1 (Itakura-Saito: beta = 0) then spreads over
# L^2 (L^1.5) inside one sum of the H half: a bulk term of the first columns' numerators is below the bar, whatever range data has.
# With data / est in the narrow range instead, P spreads like Q does and every row meets the condition sensitivity >= 4 bars.
# The last three are Itakura-Saito and beta under the MU rule's 0/1 mask (the option pq_mask: the sentinel families of cmf_kernels.h),
# restated by tests/masked_pq_mu_restatement.py; zeros and relative data follow the unmasked twin.
FORMS = {"kl": (":kl", None, False, True, False), "kl_mask": (":kl", None, True, True, False),
         "is": (":itakura_saito", None, False, False, True), "beta050": (":beta", 0.5, False, True, True),
         "beta150": (":beta", 1.5, False, True, False),
         "is_mask": (":itakura_saito", None, True, False, True), "beta050_mask": (":beta", 0.5, True, True, True),
         "beta150_mask": (":beta", 1.5, True, True, False)}
JUNK = (np.nan, np.inf, -1.0, 0.0)  # what the library is handed under the mask of the last three (junk_under_mask)


def pq_masked(form):
    """Whether the form is one of the masked two-array forms (Itakura-Saito or beta under the mask: the option pq_mask)."""
    kind, _, masked = FORMS[form][:3]
    return masked and kind != ":kl"


def pq_beta(form):
    """The beta tests/masked_pq_mu_restatement.py knows the form by (0: Itakura-Saito)."""
    return FORMS[form][1] or 0.0


def junk_under_mask(X, mask, seed=0):
    """X with NaN, +inf, -1 and 0 in turn (by the entry's hash) wherever mask == 0: what the library is given under a masked two-array
    form.  The restatement never looks there (the fp64 reference is computed from X itself), so a sentinel copy that lets one raw
    value through shows as a non-finite or wrong element."""
    N, T = X.shape
    nn, tt = np.meshgrid(np.arange(N), np.arange(T), indexing="ij")
    junk = np.asarray(JUNK)[(_hash(nn, tt, salt=seed * 4 + 7) % np.uint64(len(JUNK))).astype(np.int64)]
    return np.asfortranarray(np.where(np.asarray(mask) != 0, X, junk))


def make_divergence_problem(N, T, K, L, family, zeros=False, seed=0, relative=False):
    """(W, H, X, mask): W and H of make_problem, X in {16 ... 31} from the hash X of make_problem comes from (zeros: about one entry in
    eight exactly 0, chosen by other bits of it), and a 0/1 mask in blocks of 1 x 8 entries (a quarter held out) for the masked form.
    relative: X is that value times est / 16, est = tensor_conv(W, H) -- a multiple of 1/16 below 2^12, exact in fp32, with data / est
    in [1, 2) (the forms FORMS marks)."""
    W, H, _ = make_problem(N, T, K, L, family, seed)
    h = _data_hash(N, T, seed)
    X = (DIV_XMIN + h % np.uint64(DIV_XMAX - DIV_XMIN + 1)).astype(np.float64)
    if relative:
        import kl_mu_restatement as kr

        X *= kr.tensor_conv(W, H) / DIV_XMIN
    if zeros:
        X[(h >> np.uint64(20)) % np.uint64(8) == 0] = 0.0
    nn, tb = np.meshgrid(np.arange(N), np.arange(T) // 8, indexing="ij")
    mask = ((_hash(nn, tb, salt=seed * 4 + 5) >> np.uint64(9)) % np.uint64(4) != 0).astype(np.float64)
    return W, H, np.asfortranarray(X), np.asfortranarray(mask)


def step_exponent(form):
    """The exponent the element-wise step raises num / den to."""
    kind, beta = FORMS[form][:2]
    return 0.5 if kind == ":itakura_saito" else (1.0 / (2.0 - beta) if beta < 1 else 1.0 if beta <= 2 else 1.0 / (beta - 1.0)) if beta else 1.0


def divergence_sources(form, X, mask, W, H, cdtype=np.float64, edtype=np.float64):
    """(P, Q) in fp64: the array the numerators contract and the one the denominators contract (None: plain KL, whose denominators
    are sums of the other factor), formed by the form's restatement."""
    import beta_mu_restatement as br
    import is_mu_restatement as ir
    import kl_mu_restatement as kr
    import masked_kl_mu_restatement as mk

    kind, beta, masked = FORMS[form][:3]
    if kind == ":kl":
        return (mk.ratio(mk.MaskedKL(X, mask), W, H, cdtype, edtype), mask) if masked else (kr.ratio(X, W, H, cdtype, edtype), None)
    if masked:  # (select(mask, data, 1), then P and Q with exact 0 where mask == 0)
        import masked_pq_mu_restatement as pm

        return pm.pq(pm.check_data(X, mask, pq_beta(form))[0], mask, W, H, pq_beta(form), cdtype, edtype)
    if kind == ":itakura_saito":
        return ir.pq(X, W, H, cdtype, edtype)
    return br.pq(X, W, H, beta, cdtype, edtype)


def divergence_loss(form, X, mask, W, H, cdtype=np.float64, edtype=np.float64):
    """The loss compute_loss() reports under the form, by its restatement."""
    import beta_mu_restatement as br
    import is_mu_restatement as ir
    import kl_mu_restatement as kr
    import masked_kl_mu_restatement as mk

    kind, beta, masked = FORMS[form][:3]
    if kind == ":kl":
        return mk.masked_kl_loss(mk.MaskedKL(X, mask), W, H, cdtype, edtype) if masked else kr.kl_loss(X, W, H, cdtype, edtype)
    if masked:
        import masked_pq_mu_restatement as pm

        xs, count = pm.check_data(X, mask, pq_beta(form))
        return pm.masked_loss(xs, mask, count, W, H, pq_beta(form), cdtype, edtype)
    if kind == ":itakura_saito":
        return ir.is_loss(X, W, H, cdtype, edtype)
    return br.beta_loss(X, W, H, beta, cdtype, edtype)


def divergence_half(form, family, X, mask, W, H, cdtype=np.float64, edtype=np.float64, corrupt=None):
    """One update_motifs! (family "W") or update_feature_maps! (family "H") of the form from (W, H), the restatement's operations
    with its intermediate arrays kept: a dict of P, Q (divergence_sources), num, den (the contractions; for plain KL the sums),
    den_total = ((den + l1) + 2 l2 x) + eps, new (the updated factor) and, family "H", loss (after the update), with L1 and L2 as
    regularisers.  tests/test_exact_problems.py holds it equal to the restatements' own update functions bit for bit.
    corrupt(stage, arrays): called with "sources" after P and Q exist and with "sums" after num and den do, to damage them in
    place (the mutation tests)."""
    import kl_mu_restatement as kr

    K, N, L = W.shape
    T = H.shape[1]
    P, Q = divergence_sources(form, X, mask, W, H, cdtype, edtype)
    a = dict(P=P, Q=Q, W=W, H=H, family=family, form=form, X=X, mask=mask)
    if corrupt:
        corrupt("sources", a)
    if family == "W":
        a["num"] = kr.hxt(H, a["P"], L, cdtype)
        a["den"] = kr.denom_W(H, N, L) if a["Q"] is None else kr.hxt(H, a["Q"], L, cdtype)
        x = W
    else:
        a["num"] = kr.tensor_transconv(W, a["P"], cdtype)
        a["den"] = kr.denom_H(W, T) if a["Q"] is None else kr.tensor_transconv(W, a["Q"], cdtype)
        x = H
    if corrupt:
        corrupt("sums", a)
    a["den_total"] = ((a["den"] + L1) + (2.0 * L2) * x) + EPS
    q = a["num"] / a["den_total"]
    g = step_exponent(form)
    a["new"] = np.maximum(x * (np.sqrt(q) if g == 0.5 else q if g == 1.0 else q ** g), EPS)
    if family == "H":
        a["loss"] = divergence_loss(form, X, mask, W, a["new"], cdtype, edtype)
    return a


def _min_positive_terms(family, src, W, H):
    """Per element of the updated factor, the smallest POSITIVE term of its contraction with src (inf where it has none).  On these
    problems the factor that is not updated holds one unit entry per column / per (n, l): the terms are entries of src."""
    K, N, L = W.shape
    T = H.shape[1]
    if src is None:  # (plain KL: the denominator sums the unit entries themselves)
        return np.ones((K, N, L) if family == "W" else (K, T))
    s = np.where(src > 0, src, np.inf)
    if family == "W":  # num[k, n, l] = sum over the columns t of component k, t + l < T, of src[n, t + l]
        comp = np.argmax(H, axis=0)
        m = np.full((K, N, L), np.inf)
        for k in range(K):
            cols = np.flatnonzero(comp == k)
            for lag in range(min(L, T)):
                c = cols[cols + lag < T] + lag
                if len(c):
                    m[k, :, lag] = s[:, c].min(axis=1)
        return m
    comp = np.argmax(W, axis=0)  # (N, L); num[k, t] = sum over the (n, l) of component k, t + l < T, of src[n, t + l]
    m = np.full((K, T), np.inf)
    for lag in range(min(L, T)):
        for k in range(K):
            rows = comp[:, lag] == k
            if rows.any():
                np.minimum(m[k, : T - lag], s[rows, lag:].min(axis=0), out=m[k, : T - lag])
    return m


def sensitivity(form, a, exact=True):
    """The smallest relative change of any element of the updated factor a["new"] (a: divergence_half in fp64) when ONE positive term
    is removed from its numerator or from its denominator contraction: min over elements of 1 - (1 - p / num)^g and
    (1 - q / den_total)^-g - 1, p and q the smallest positive terms of the element's two sums and g the step exponent.  (A term that
    is exactly 0 -- data 0, a held-out entry -- cannot be missed: removing it changes nothing.)  Elements on the floor eps (num == 0)
    have no term to lose and are left out.  exact=False: a lower bound in closed form, from the smallest positive entries of P and Q
    and the largest sums -- cheap, for the large shapes."""
    g = step_exponent(form)
    num, dt = a["num"], a["den_total"]
    live = num > 0
    if exact:
        p = _min_positive_terms(a["family"], a["P"], a["W"], a["H"])[live]
        q = _min_positive_terms(a["family"], a["Q"], a["W"], a["H"])[live]
        xn, xd = p / num[live], q / dt[live]
    else:
        xn = a["P"][a["P"] > 0].min() / num.max()
        xd = (1.0 if a["Q"] is None else a["Q"][a["Q"] > 0].min()) / dt[live].max()
    with np.errstate(divide="ignore"):
        xn, xd = np.minimum(xn, 1.0), np.minimum(xd, 1.0 - 1e-12)
        return float(min(np.min(1.0 - (1.0 - xn) ** g), np.min((1.0 - xd) ** -g - 1.0)))


def rel_err(got, ref):
    """|got - ref| / |ref| element-wise (ref: the fp64 restatement, every entry >= eps > 0)."""
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.abs(ref)


def check_elementwise(got, ref, bar, names):
    """None when every element of got is within the relative bar of ref (and finite); else a line that names the WORST element the way
    first_bad names the first: 'rel 3.1e-03 (bar 2e-06) at k=.., n=.., l=..: got .., want .. (17 elements over the bar)'."""
    r = rel_err(got, ref)
    r = np.where(np.isfinite(r), r, np.inf)
    if r.max() <= bar:
        return None
    i = np.unravel_index(np.argmax(r), r.shape)
    where = first_bad(r == r[i], names)
    return f"rel {r[i]:.2e} (bar {bar:g}) at {where}: got {got[i]!r}, want {ref[i]!r} ({int((r > bar).sum())} elements over the bar)"


def read_bars(path):
    """{"bar": {form: value}, "lossbar": {...}, "gpu": {...}} of profiles/mu_divergence_elementwise.txt."""
    out = {"bar": {}, "lossbar": {}, "gpu": {}, "gpuloss": {}}
    for line in open(path):
        f = line.split()
        if len(f) == 3 and f[0] in out:
            out[f[0]][f[1]] = float(f[2])
    return out


def divergence_configs(configs, form):
    """The configurations of a table row a divergence form accepts: no Gram form, one device."""
    return [c for c in configs if "gram" not in c and "devices" not in c]


# ---- the masked MU rule and the PGD rule on these problems (tests/test_gpu_exact_masked_mu.py, tests/test_gpu_exact_pgd.py) -------
# Masked MU: make_problem's X under the 0/1 mask of make_divergence_problem.  mask .* est, mask .* X, both numerators and denominators
# and the loss tile sums stay sums of small non-negative integers, so the argument of the module doc holds unchanged.
#
# PGD: the residual est - X is a SIGNED integer, gradW = hxt(H, resid) and gradH = transconv(W, resid) are signed integer sums whose
# every partial sum is bounded by the sum of absolute values; g = gscale G + 2 pen_sq x + pen_abs sign(x) is a multiple of 1/2;
# pgd_w_grad_kernel / pgd_h_grad_kernel sum g^2 in double (an exact integer multiple of 1/4 below 2^53 in any order), so
# alpha = (float)(step / (sqrt(sum g^2) + eps)) is ONE float32 number on every path, and x - alpha g, fused or not, is within
# 0.5 ulp (the result) + 0.5 ulp of alpha |g| (the product) + 2^-24 alpha |g| (alpha rounded) of the fp64 value: with alpha |g| at most
# a quarter of |x_new| (pgd_preconditions: no_clamp) that is below 1 ulp of x_new, inside the bar of 2.
STEP0 = 5.0  # PGDUpdate's first stepW, stepH (pgd.jl:149-150)
# name -> (loss, masked, (penaltiesW_sq, penaltiesW_abs), (penaltiesH_sq, penaltiesH_abs), nonneg); the first four are the loss kinds
# under the rule's defaults (penaltiesW = [SquarePenalty(1)], penaltiesH = [], NonnegConstraint), then the dyadic AbsolutePenalty on
# both factors and the rule without a constraint
PGD_VARIANTS = {
    "square": ("square", False, ((1.0,), ()), ((), ()), True),
    "abs": ("abs", False, ((1.0,), ()), ((), ()), True),
    "square_masked": ("square", True, ((1.0,), ()), ((), ()), True),
    "abs_masked": ("abs", True, ((1.0,), ()), ((), ()), True),
    "square_l1": ("square", False, ((1.0,), (0.5,)), ((), (0.5,)), True),
    "abs_masked_free": ("abs", True, ((1.0,), ()), ((), ()), False),
}
PGD_LARGE_VARIANTS = ("square", "abs_masked")  # the rows with N >= 1000: a test stays at a few seconds


def pgd_variants(N):
    return list(PGD_LARGE_VARIANTS) if N >= 1000 else list(PGD_VARIANTS)


_conv_last = [None, None, None]


def _conv(W, H):
    """tensor_conv(W, H) by the oracle; the last result is kept for the same two array objects (the helpers below never write into
    W or H, and every variant of a row asks for the same est)."""
    from oracle import cmf_oracle

    if _conv_last[0] is not W or _conv_last[1] is not H:
        _conv_last[:] = [W, H, cmf_oracle.tensor_conv(W, H)]
    return _conv_last[2]


def mu_mask(N, T, seed=0):
    """The 0/1 mask of make_divergence_problem (blocks of 1 x 8 entries, a quarter held out) on its own."""
    nn, tb = np.meshgrid(np.arange(N), np.arange(T) // 8, indexing="ij")
    return np.asfortranarray(((_hash(nn, tb, salt=seed * 4 + 5) >> np.uint64(9)) % np.uint64(4) != 0).astype(np.float64))


def holes_mask(N, T, seed=0):
    """mu_mask with one unit (N // 2) and one sample (T // 3) never observed."""
    m = mu_mask(N, T, seed)
    m[N // 2, :] = 0.0
    m[:, T // 3] = 0.0
    return m


PGD_R = 2  # the near-fit data's noise: r in {-PGD_R ... PGD_R}
# The first step of a fresh rule has norm 5 whatever the data is (alpha g = 5 g / |g|), so its largest entry is at least 5 / sqrt(number
# of entries of the factor): 0.2 ... 0.7 on the table's small rows, against entries of 1 and 2.  The dense factor is therefore
# make_problem's times 4 (entries 4 and 8, est four times as large, every sum still far below 2^24): the step stays below a quarter of
# every updated entry on every row, which is what the 2 ulp bound needs (pgd_preconditions: no_clamp).
PGD_SCALE = 4.0


def make_pgd_problem(N, T, K, L, family, seed=0):
    """(W, H, X, mask): W and H of make_problem, the dense one times PGD_SCALE; NEAR-FIT data X = max(est + r, 0), est = tensor_conv(W, H) and r in {-2 ... 2} from
    other bits of the hash make_problem's X comes from (a fifth of the residual is exactly 0: sign(0) = 0 of the AbsoluteLoss store;
    the gradient is small, so alpha = 5 / |g| is large and one lost unit of a contraction moves an element by many ulp:
    pgd_preconditions); and a WEIGHT mask in {0, 1, 2} in blocks of 1 x 8 entries, about a quarter 0 (the PGD mask is real-valued,
    cmf_set_mask: the weight 2 catches an epilogue that treats it as a flag)."""
    W, H, _ = make_problem(N, T, K, L, family, seed)
    if family == "W":
        W *= PGD_SCALE
    else:
        H *= PGD_SCALE
    h = _data_hash(N, T, seed)
    r = ((h >> np.uint64(24)) % np.uint64(2 * PGD_R + 1)).astype(np.float64) - PGD_R
    X = np.maximum(_conv(W, H) + r, 0.0)
    nn, tb = np.meshgrid(np.arange(N), np.arange(T) // 8, indexing="ij")
    v = (_hash(nn, tb, salt=seed * 4 + 6) >> np.uint64(9)) % np.uint64(8)
    mask = np.where(v < 2, 0.0, np.where(v < 5, 1.0, 2.0))
    return W, H, np.asfortranarray(X), np.asfortranarray(mask)


def _contract(family, W, H, E):
    """compute_gradW! (pgd.jl:206-214, family "W") or compute_gradH! (:218-221) of the array E, in fp64."""
    from oracle import cmf_oracle

    if family == "H":
        return cmf_oracle.tensor_transconv(W, E)
    K, N, L = W.shape
    T = H.shape[1]
    out = np.zeros(W.shape)
    for lag in range(min(L, T)):
        out[:, :, lag] = H[:, : T - lag] @ E[:, lag:].T
    return out


def pgd_sources(variant, W, H, X, mask, weights=True):
    """(E, gscale): the array the gradient contracts as the conv epilogue stores it -- est - data or its sign, times the mask -- and
    the factor the gradient kernels apply (2 for SquareLoss, 1 for AbsoluteLoss).  weights=False: the mask read as a 0/1 flag."""
    loss, masked = PGD_VARIANTS[variant][:2]
    E = _conv(W, H) - X
    if loss == "abs":
        E = np.sign(E)
    if masked:
        E = E * (mask if weights else (mask != 0))
    return E, (1.0 if loss == "abs" else 2.0)


def pgd_half(variant, family, W, H, X, mask, corrupt=None, step=STEP0):
    """The half-step of the variant from (W, H) with its intermediate arrays kept: E, gscale (pgd_sources), G (the contraction), g (the
    gradient with the penalties), sumsq, alpha, new (the updated factor, clamped where the variant projects).  The operations are
    oracle._pgd's (tests/test_exact_problems.py holds `new` equal to the oracle's factor bit for bit); this is what the preconditions,
    the float32 model and the mutation tests are computed from, NOT the reference of the GPU tests (that is the oracle itself).
    corrupt(stage, arrays): "sources" after E exists, "sums" after G does."""
    _, _, penW, penH, nonneg = PGD_VARIANTS[variant]
    pen_sq, pen_abs = penW if family == "W" else penH
    a = dict(W=W, H=H, family=family, variant=variant)
    a["E"], a["gscale"] = pgd_sources(variant, W, H, X, mask)
    if corrupt:
        corrupt("sources", a)
    a["G"] = _contract(family, W, H, a["E"])
    if corrupt:
        corrupt("sums", a)
    return pgd_finish(a, step)


def pgd_finish(a, step=STEP0):
    """g, sumsq, alpha, free and new of pgd_half from a["G"] (again after a mutation test has damaged G)."""
    _, _, penW, penH, nonneg = PGD_VARIANTS[a["variant"]]
    family = a["family"]
    pen_sq, pen_abs = penW if family == "W" else penH
    x = a["W"] if family == "W" else a["H"]
    g = a["G"] * a["gscale"]
    for w in pen_sq:
        g = g + 2.0 * w * x
    for w in pen_abs:
        g = g + w * np.sign(x)
    a["g"], a["x"] = g, x
    a["sumsq"] = float(np.sum(g * g))
    a["alpha"] = step / (np.sqrt(a["sumsq"]) + EPS)
    a["free"] = x - a["alpha"] * g
    a["new"] = np.maximum(a["free"], EPS) if nonneg else a["free"]
    return a


def pgd_f32_model(a, fused):
    """The device's half-step from the EXACT gradient: alpha rounded to float32 (pgd_w_apply_kernel), then x - alpha g in float32 with
    the product rounded (fused=False) or not (fused=True: fmaf(-alpha, g, x))."""
    al = np.float32(a["alpha"])
    x32, g32 = a["x"].astype(np.float32), a["g"].astype(np.float32)
    assert np.array_equal(x32, a["x"]) and np.array_equal(g32, a["g"])  # (both exact in fp32)
    if fused:
        new = (a["x"] - np.float64(al) * a["g"]).astype(np.float32)  # (the fp64 product of two floats is exact; one rounding)
    else:
        new = x32 - al * g32
    return np.maximum(new, np.float32(EPS)) if PGD_VARIANTS[a["variant"]][4] else new


def pgd_oracle_half(oracle, variant, family, W, H, X, mask):
    """(updated factor, (stepW, stepH), loss or None) of ONE oracle.pgd_update_motifs (family "W") or pgd_update_feature_maps (family
    "H") on a fresh oracle.PGDUpdate: the reference of tests/test_gpu_exact_pgd.py."""
    loss, masked, penW, penH, nonneg = PGD_VARIANTS[variant]
    Wc, Hc = W.copy(order="F"), H.copy(order="F")
    rule = oracle.PGDUpdate(X, Wc, Hc)
    kw = dict(nonneg=nonneg, mask=mask if masked else None, loss=loss)
    if family == "W":
        oracle.pgd_update_motifs(rule, X, Wc, Hc, penaltiesW_sq=penW[0], penaltiesW_abs=penW[1], **kw)
        return Wc, (rule.stepW, rule.stepH), None
    lv = oracle.pgd_update_feature_maps(rule, X, Wc, Hc, penaltiesH_sq=penH[0], penaltiesH_abs=penH[1], **kw)
    return Hc, (rule.stepW, rule.stepH), lv


def max_tile_sum(a, tile=128):
    """The largest sum of the non-negative array a over a tile x tile block (a bound for the 64 x 64 loss tiles of the conv epilogues)."""
    N, T = a.shape
    r = np.zeros((-(-N // tile) * tile, -(-T // tile) * tile))
    r[:N, :T] = a
    return r.reshape(r.shape[0] // tile, tile, r.shape[1] // tile, tile).sum(axis=(1, 3)).max()


def contract_cols(family, W, H, dE, t0):
    """The contraction (_contract) of an array that is dE on the columns t0 ... t0 + dE.shape[1] - 1 and 0 elsewhere: what a damaged
    block of the contracted array adds to every sum (the mutation tests)."""
    K, N, L = W.shape
    T = H.shape[1]
    t1 = t0 + dE.shape[1]
    out = np.zeros(W.shape if family == "W" else H.shape)
    for lag in range(min(L, T)):
        a, b = max(t0, lag), t1
        if a >= b:
            continue
        if family == "W":
            out[:, :, lag] = H[:, a - lag:b - lag] @ dE[:, a - t0:].T
        else:
            out[:, a - lag:b - lag] += W[:, :, lag] @ dE[:, a - t0:]
    return out


def pgd_preconditions(a, X, mask):
    """From the arrays of pgd_half (a) -- nothing here is met by skipping a row:
      exact        every accumulation's sum of ABSOLUTE values (est, the contraction of |E| with the mask's weight in it) < 2^24
      sumsq_exact  sum g^2 < 2^53 (a multiple of 1/4: exact in double in any order)
      no_clamp     alpha max|g| <= a quarter of the smallest |updated entry| (and that entry > eps): the clamp never acts, the step
                   itself is what is compared, and the product alpha g is rounded at most half as finely as the result
      units        gscale alpha / the float32 spacing at the largest |x_new|: one unit of one contraction in ulp; >= 8 is asked
      loss_exact   the 64 x 64 tile sums of the loss terms of the INTEGER factors (|E| or E^2, weights included) <= 2^24
    """
    W, H, family = a["W"], a["H"], a["family"]
    absG = _contract(family, W, H, np.abs(a["E"]))
    est = _conv(W, H)
    b = dict(absG=float(absG.max()), est=float(est.max()), sumsq=a["sumsq"])
    b["exact"] = max(b["absG"] * a["gscale"] + 2.0 * np.abs(a["x"]).max() + 0.5, b["est"], X.max()) < EXACT
    b["sumsq_exact"] = a["sumsq"] < 2.0 ** 53 and a["sumsq"] * 4 == np.round(a["sumsq"] * 4)
    b["alpha_g"] = float(a["alpha"] * np.abs(a["g"]).max())
    b["min_new"] = float(np.abs(a["free"]).min())
    b["no_clamp"] = b["alpha_g"] <= 0.25 * b["min_new"] and float(a["free"].min()) > EPS
    top = np.float32(np.abs(a["new"]).max())
    b["units"] = float(a["gscale"] * a["alpha"] / np.spacing(top))
    b["sensitive"] = b["units"] >= 8.0
    b["loss_tile"] = float(max_tile_sum(np.abs(a["E"]) if PGD_VARIANTS[a["variant"]][0] == "abs" else a["E"] ** 2))
    b["loss_exact"] = b["loss_tile"] <= EXACT
    return b


def assert_pgd_preconditions(a, X, mask, what):
    b = pgd_preconditions(a, X, mask)
    assert b["exact"], f"{what}: an fp32 accumulation would round ({b})"
    assert b["sumsq_exact"], f"{what}: sum g^2 is not exact in double ({b})"
    assert b["no_clamp"], f"{what}: alpha max|g| = {b['alpha_g']:.3f} against a smallest entry of {b['min_new']:.3g}: above a quarter of it"
    assert b["sensitive"], f"{what}: one unit of a contraction is {b['units']:.2f} ulp only (8 asked: 4 bars of 2 ulp)"
    return b


def masked_mu_half(family, W, H, X, mask, corrupt=None):
    """One update_motifs! (family "W") or update_feature_maps! (family "H") of the MU rule under the 0/1 mask, masked_mu_restatement's
    operations with the intermediate arrays kept (Xm, est = mask .* conv, num, den, new): for the preconditions and the mutation tests;
    tests/test_exact_problems.py holds `new` equal to the restatement's factor bit for bit.  corrupt: as in pgd_half."""
    a = dict(W=W, H=H, family=family, M=mask)
    a["Xm"] = np.where(mask != 0, X, 0.0)
    a["est"] = np.where(mask != 0, _conv(W, H), 0.0)
    if corrupt:
        corrupt("sources", a)
    a["num"], a["den"] = _contract(family, W, H, a["Xm"]), _contract(family, W, H, a["est"])
    if corrupt:
        corrupt("sums", a)
    x = W if family == "W" else H
    a["new"] = np.maximum(x * (a["num"] / (((a["den"] + L1) + (2.0 * L2) * x) + EPS)), EPS)
    return a


def assert_masked_mu_preconditions(a, what, holes=False):
    """assert_preconditions of tests/test_exact_parity.py on the masked sums, and every element of the updated factor keeps at least
    one observed term (holes: the deliberate exception) where the row gives every element at least 16 terms to begin with.  Where it
    does not -- an element of H sums the N L / K entries (n, t + l) of its component: 7 on the row (70, 600, 20, 2); on (40, 40, 20, 16)
    a component owns two columns of H -- blocks of 1 x 8 holding out a quarter now and then hold out all of an element's terms.
    Every such element has num = den = 0 and must come out as eps exactly, which is asserted on every row."""
    assert max(a["num"].max(), a["den"].max(), a["est"].max()) < EXACT, f"{what}: an fp32 accumulation would round"
    assert max(a["num"].max(), a["den"].max()) <= SENS, f"{what}: num / den above 2^20: the 2 ulp bar could miss a single term"
    seen = _contract(a["family"], a["W"], a["H"], (a["M"] != 0).astype(np.float64))
    terms = _contract(a["family"], a["W"], a["H"], np.ones(a["M"].shape))
    live = terms > 0
    if not holes and terms[live].min() >= 16:
        assert seen[live].min() >= 1, f"{what}: {(seen[live] == 0).sum()} elements of the updated factor have no observed term"
    assert np.all(a["new"][seen == 0] == EPS)
    seen[~live] = -1  # (no term at all, mask or not: lags beyond the recording, components without a column)
    return seen


# ---- the HALS rule on these problems (tests/test_gpu_exact_hals.py; CPU half in tests/test_exact_problems.py) ----------------------
# Every contraction the HALS rule makes on an integer problem -- G = resid * H_unfold' from the stored residual or as denomW - numW,
# HH and the lag correlations it is assembled from, P = transconv(W, resid) or denomH - numH, the lag Grams PW and the taps GW / GE --
# is an integer sum below 2^24 in absolute values (hals_preconditions): exact in fp32 in any order, so the projections reach the sweeps
# bit-identical on every path and under every value of hals_gram.  What is left is the rounding INSIDE the sequential recurrences.
# It is measured, not derived: hals_gram_form.w_half / h_half with the sweep's state in float32 against the same in fp64, per element
# in units of the fp32 spacing at scale = max(|value before the clamp|, |old value|).  Each half runs on the family whose updated factor
# is dense (W on "W", H on "H"): with the other factor dense the Gauss-Seidel sweep amplifies rounding a thousandfold and no bar near
# rounding exists.  The bar of a half is 4 times the worst model error over the table, and at least 8 (a kernel associates the cross-row
# sums differently, fuses multiply-adds, and multiplies by a reciprocal where the model divides); profiles/exact_hals.txt records it
# (tools/exact_hals_profile.py) and tests/test_exact_problems.py recomputes it.
HALS_LAUNCH_PATHS = [
    "hals_w_sweep_reg_kernel<2>", "hals_w_sweep_reg_kernel<4>", "hals_w_sweep_reg_kernel<6>", "hals_w_sweep_reg_kernel<8>",
    "hals_w_sweep_reg_kernel<10>", "hals_w_sweep_reg_kernel<12>", "hals_w_sweep_reg_kernel<16>", "hals_w_sweep_reg_kernel<20>",
    "hals_w_sweep_reg_kernel<24>", "hals_w_sweep_reg_kernel<32>", "hals_w_sweep_gen_kernel",
    "hals_g:residual", "hals_g:difference", "hals_g:speculated", "hals_w_speculate",
    "hals_p_init_kernel:den", "hals_p_init_kernel:residual", "hals_p_init_kernel:snapshot",
    "hals_h_persist_kernel", "hals_h_persist_kernel:P1", "hals_h_persist_kernel:P2", "hals_h_persist_kernel:P3", "hals_h_persist_kernel:P4",
    "hals_h_persist_kernel:chased", "conv3_chase_kernel", "conv3_chase_kernel:rest",
    "hals_h_stage_kernel", "hals_h_stage_kernel:lag2", "hals_h_stage_kernel:lag3", "hals_h_row_gen_kernel", "hals_h_push_gen_kernel",
]
HALS_NQ = (2, 4, 6, 8, 10, 12, 16, 20, 24, 32)  # the instances of hals_w_sweep_reg_kernel<NQ, WD>
HALS_PMAX = 4
HALS_REGS = [(0.0, 0.0), (L1, L2)]
HALS_BAR_FACTOR, HALS_BAR_FLOOR = 4.0, 8.0


def hals_plan(N, T, K, L, cfg=None, n_cu=N_CU):
    """cmf_rules.hip hals_plan / hals_w_impl / hals_h_project / hals_chase_rows restated: a dict of nq (the 64-lane slots the state
    L * K32 needs), NQ (the register instance, None under the general W sweep), pad_slots (NQ - nq), w_general, h_general, P (pullers
    per row; 0: the stage pipeline), nblk (64-column blocks of a row), chase (tile rows of the residual conv that chase the pipeline)
    and gram_window (the Gram form of P fits its LDS window), for the options of cfg."""
    cfg = cfg or {}
    K32 = rup(K, 32)
    general, persist, chase = cfg.get("hals_general", 0), cfg.get("hals_persist", 1), cfg.get("hals_chase", -1)
    p = dict(nq=(L * K32 + 63) // 64, nblk=(T + 63) // 64)
    p["w_general"] = bool(L * K32 > 2048 or 4 * K * L * 2 * 4 > 64 * 1024 or general & 1)
    p["h_general"] = bool(L > 64 or general & 2)
    p["NQ"] = None if p["w_general"] else min(q for q in HALS_NQ if q >= p["nq"])
    p["pad_slots"] = 0 if p["w_general"] else p["NQ"] - p["nq"]
    P = 0
    if persist != 0 and not p["h_general"]:
        P = min(HALS_PMAX, (n_cu - K) // (K - 1)) if K > 1 else 1
        if persist > 1:
            P = min(P, persist)
        if ((K - 1) * (2 * L - 1 + 64 + 2 * (L - 1)) + 1024) * 4 > 120 * 1024 or (P < 2 and K > 1):
            P = 0
        small_k = K <= 16 and L <= 64
        if P == 4 and persist == 1 and chase != 0 and K % 32 == 0 and not small_k and T >= 4096:
            P = 3
    p["P"] = P
    rows, ra = (T + 63) // 64, 0
    if (chase != 0 and P > 0 and K % 32 == 0 and cfg.get("hals_gram", 2) != 1 and n_cu % 8 == 0 and n_cu <= 256  # (the CU masks cut inside every XCD)
            and n_cu // 8 - (K + (K - 1) * P + 7) // 8 >= 4 and rows >= 64):
        pct = chase
        if pct < 0:
            conv_ms = 2.0 * K * N * (L * T) / (0.87 * 157.3e12) * 1e3
            pipe_ms = (T + (K - 1) * (L - 1)) * 43.0 / 2.4e9 / 0.63 * 1e3
            share = (n_cu // 8 - (K + (K - 1) * P + 7) // 8) / (n_cu // 8) * (0.76 * pipe_ms) / conv_ms
            pct = int(max(10.0, min(95.0, 110.0 * share)))
        ra = min(rows, rows * min(pct, 100) // 100)
    p["chase"] = ra
    p["gram_window"] = K32 * (64 + 2 * (L - 1)) * 4 <= 96 * 1024
    return p


_SWEEPS = [dict(), dict(hals_persist=2), dict(hals_persist=3), dict(hals_persist=0, hals_seg=256), dict(hals_persist=0, hals_seg=256, hals_lag=3),
           dict(hals_general=3)]
# (N, T, K, L, sweep configurations, why); every configuration runs under hals_gram = 2, 0 and 1
HALS_SHAPES = [
    # the W sweep's register instances (N odd: the guard of the last unit; 37: five workgroups), the H pipelines beside them
    (37, 150, 5, 4, [dict(), dict(hals_general=1)], "NQ 2; five rows, 3 blocks for 4 pullers, T no multiple of 64; the general W sweep forced"),
    (37, 768, 32, 8, [dict(), dict(hals_persist=2)], "NQ 4; T a multiple of 64"),
    (37, 700, 32, 12, [dict()], "NQ 6; L - 1 >= 8: a second chunk of edge taps"),
    (37, 700, 32, 16, [dict()], "NQ 8"),
    (37, 700, 32, 20, _SWEEPS, "NQ 10; every H pipeline: 4, 2, 3 pullers, the stage pipeline over three segments at lag 2 and 3, both general sweeps forced"),
    (37, 700, 32, 24, [dict()], "NQ 12"),
    (37, 700, 32, 32, [dict()], "NQ 16"),
    (37, 1300, 64, 20, [dict(), dict(hals_persist=2), dict(hals_persist=0)], "NQ 20 (ring 4 deep); K = 64: 3 pullers, D staged through LDS in more than one piece"),
    (37, 1300, 64, 24, [dict()], "NQ 24"),
    (37, 1300, 64, 32, [dict()], "NQ 32, all slots live"),
    (133, 700, 33, 3, [dict(), dict(hals_general=2)], "NQ 4 with 3 slots live; two k blocks; the general H sweep forced (half of X zero: HALS_XZERO)"),
    (37, 700, 33, 31, [dict()], "NQ 32 with 31 slots live"),
    (37, 1300, 64, 18, [dict()], "NQ 20 with 18 slots live"),
    (37, 1300, 64, 40, [dict()], "L * K32 = 2560: the general W sweep by the plan"),
    (37, 700, 18, 20, [dict(), dict(hals_persist=3)], "K = 18"),
    # hals_hh_kernel's four ways to an entry, short recordings, the window lengths
    (9, 5, 2, 8, [dict(), dict(hals_persist=0)], "T < L: every column an edge column, rows of H_unfold that are all zero"),
    (9, 30, 2, 20, [dict()], "L < T < 2 L: HH summed directly"),
    (9, 80, 1, 20, [dict()], "T <= 64 + L; K = 1: one sweeper, one puller slot, no cross-row term"),
    (9, 50, 2, 1, [dict(), dict(hals_persist=0)], "L = 1: no edge, no lag; T < 64.  No clamp share: at L = 1 no shape and no range of X has one (HALS_NO_CLAMP_AT_L)"),
    (9, 200, 4, 64, [dict(), dict(hals_persist=0)], "L = 64: the widest on-chip window; NQ 32"),
    (9, 200, 3, 70, [dict()], "L = 70: both general sweeps by the plan"),
    # the residual conv chasing the persistent pipeline (the shape of test_hals_residual_conv_chasing_the_row_pipeline)
    (130, 9000, 32, 20, [dict(hals_chase=65), dict(hals_chase=0)], "the chased form at 65 per cent (3 pullers), and 4 pullers without it; many slabs of the lag correlations"),
    # past the Gram form's LDS window (below)
    (29, 1200, 129, 46, [dict()], "K32 (64 + 2 (L - 1)) 4 = 98560 > 96 KB: P from the residual under every hals_gram; 129 rows: the stage pipeline by the plan; the general W sweep"),
]
# The last row lies past the LDS window of the Gram form of P, K32 * (64 + 2 (L - 1)) * 4 > 96 KB (160 * 154 * 4 = 98560): hals_h_project
# must then form P from the transposed residual under hals_gram = 2 and 1 as well ("hals_p_init_kernel:residual", the same bits as
# hals_gram = 0) -- if its condition were wrong, gram_denom_h would refuse the shape.  Shapes with fewer components are past the window
# too ((65, 98), (33, 162), (3, 354)), but est sums L entries of 1 and 2 and with L near 100 it lies above X in {0 ... 40} nearly
# everywhere: fewer than 9 % of the elements stay positive, and a wider X takes the float32 model to 110 ... 170 units, which would
# quadruple every row's bar.  (129, 46) keeps X and meets every precondition.


# est of a row sums min(L, T) entries of 1 and 2: with three lags it stays below 6, X in {0 ... 40} lies above it nearly everywhere
# and the clamp hardly acts (3 % of W).  On such a row every z-th entry of X, chosen by other bits of its hash, is 0 (a narrower range
# of X instead makes every sum a small integer and the clamp a tie on hundreds of elements).
HALS_XZERO = {(133, 700, 33, 3): 2}
# At L = 1 with one unit entry per column (per unit) the least-squares problem decouples: every updated element is a MEAN of entries of
# X, never negative, whatever N, T, K and the range of X are.  Under l1 = l2 = 0 an element sits on the clamp only where that mean is
# exactly 0 -- a tie, not a decision, and one of the close calls the same list of conditions forbids; under l1 > 0 sparse X would clamp
# the elements whose sum of X is below l1, but the row runs under both regulariser pairs and must meet the conditions under both.  So no
# shape meets the clamp share at L = 1, and it is not asked there (assert_hals_preconditions); every other condition is.
HALS_NO_CLAMP_AT_L = 1


def make_hals_problem(N, T, K, L, family, seed=0):
    """make_problem's integer factors and X in {0 ... XMAX} (HALS_XZERO: with the row's share of zeros)."""
    W, H, X = make_problem(N, T, K, L, family, seed)
    z = HALS_XZERO.get((N, T, K, L))
    if z is not None:
        X[(_data_hash(N, T, seed) >> np.uint64(20)) % np.uint64(z) != 0] = 0.0
    return W, H, X


def hals_half(family, W, H, X, reg, dtype=np.float64, corrupt=None, eps=None):
    """hals_gram_form.w_half (family "W") or h_half ("H") under the regularisers reg = (l1, l2)."""
    import hals_gram_form as hg
    from oracle import cmf_oracle

    return (hg.w_half if family == "W" else hg.h_half)(cmf_oracle, W, H, X, reg[0], reg[1], dtype, corrupt, eps)


def hals_units(got, a):
    """|got - a["new"]| in units of the fp32 spacing at a["scale"], element-wise (a: w_half / h_half in fp64); not finite -> inf."""
    sp = np.spacing(a["scale"].astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        u = np.abs(np.asarray(got, dtype=np.float64) - a["new"]) / sp
    return np.where(np.isfinite(u), u, np.inf)


def hals_excused(a, bar):
    """Elements whose value before the clamp is within the bar of 0: their zero pattern is not decided (they still meet the bar).
    Not among them: the steps whose squared norm is 0 (a lag beyond the recording, a component without an entry in the window).  Their
    projection is an empty sum, exactly 0 on every path and never added to, so the value before the clamp is -l1 / (eps + l2) in any
    arithmetic: 0 or negative, and the element is 0."""
    return (np.abs(a["pre"]) <= bar * np.spacing(a["scale"].astype(np.float32)).astype(np.float64)) & (a["diag"] != 0)


def hals_contractions(family, a):
    """name -> the largest sum of ABSOLUTE values of every contraction in front of the family's sweep, both forms of the projections
    (a: the fp64 half of the family).  Below 2^24 every partial sum of it is an exact fp32 integer in any order."""
    from oracle import cmf_oracle

    W, H, R = a["W"], a["H"], a["R"]
    K, N, L = W.shape
    T = H.shape[1]
    est = R + (cmf_oracle.tensor_conv(W, H) - R)  # (= est: R is est - X)
    X = est - R
    out = dict(est=est.max(), X=X.max())
    if family == "W":
        Hu = a["Hu"]
        out.update(G=(np.abs(R) @ Hu.T).max(), denomW=(est @ Hu.T).max(), numW=(X @ Hu.T).max(), HH=a["HH"].max(),
                   corr=max((H[:, : T - d] @ H[:, d:].T).max() for d in range(min(L, T))))
    else:
        PW = a["PW"]
        out.update(P=cmf_oracle.tensor_transconv(W, np.abs(R)).max(), denomH=cmf_oracle.tensor_transconv(W, est).max(),
                   numH=cmf_oracle.tensor_transconv(W, X).max(), PW=PW.max(),
                   taps=max(PW[np.arange(max(0, e), min(L, L + e)), :, np.arange(max(0, e), min(L, L + e)) - e, :].sum(axis=0).max() for e in range(-(L - 1), L)))
    return {k: float(v) for k, v in out.items()}


def hals_preconditions(family, a, bar):
    """From the arrays of the fp64 half: exact (every contraction < 2^24), the shares of the updated elements strictly positive (pos) and
    exactly on the clamp (clamp) -- for the H half also among the last L - 1 columns (edge_pos, edge_clamp) --, close (the elements
    within the bar of the clamp: excused from the zero-pattern check, counted) and min_pre (the closest |pre| / spacing of the others,
    the steps of norm 0 apart: hals_excused)."""
    c = hals_contractions(family, a)
    new, L = a["new"], a["W"].shape[2]
    b = dict(abs_sum=max(c.values()), exact=max(c.values()) < EXACT, pos=float((new > 0).mean()), clamp=float((new == 0).mean()))
    if family == "H" and L > 1:
        edge = new[:, max(0, new.shape[1] - L + 1):]
        b.update(edge_pos=float((edge > 0).mean()), edge_clamp=float((edge == 0).mean()))
    ex = hals_excused(a, bar)
    b["close"] = int(ex.sum())
    sp = np.spacing(a["scale"].astype(np.float32)).astype(np.float64)
    b["min_pre"] = float((np.abs(a["pre"]) / sp)[~ex & (a["diag"] != 0)].min())
    return b


def assert_hals_preconditions(b, size, L, what):
    assert b["exact"], f"{what}: a contraction reaches {b['abs_sum']:.0f} >= 2^24"
    for key in ("pos", "edge_pos"):
        assert b.get(key, 1.0) >= 0.15, f"{what}: {key} = {b[key]:.3f}: fewer than 15 % of the updated elements are strictly positive"
    for key in ("clamp", "edge_clamp"):
        assert L == HALS_NO_CLAMP_AT_L or b.get(key, 1.0) >= 0.05, f"{what}: {key} = {b[key]:.3f}: fewer than 5 % of the updated elements sit on the clamp"
    assert b["close"] <= 0.001 * size, f"{what}: {b['close']} of {size} elements decide their clamp within the bar"


def read_hals_profile(path):
    """{"row": {(shape, family, reg): {key: value}}, "bar": {"W": .., "H": .., "loss": ..}, "gpu": {name: value}} of profiles/exact_hals.txt."""
    out = dict(row={}, bar={}, gpu={})
    for line in open(path):
        f = line.split()
        if f and f[0] == "row":
            out["row"][(f[1], f[2], f[3])] = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in f[4:]}
        elif f and f[0] in ("bar", "gpu") and len(f) == 3:
            out[f[0]][f[1]] = float(f[2])
    return out


def hals_bars(path=None):
    """(bar of the W half, bar of the H half, relative bar of the loss: 4 times the worst float32 model, no floor) from the `row` lines of profiles/exact_hals.txt."""
    import os

    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exact_hals.txt")
    rows = read_hals_profile(path)["row"]
    bar = {f: max(HALS_BAR_FLOOR, HALS_BAR_FACTOR * max(v["model"] for k, v in rows.items() if k[1] == f)) for f in ("W", "H")}
    loss = HALS_BAR_FACTOR * max(v["loss_model"] for k, v in rows.items() if k[1] == "H")
    return bar["W"], bar["H"], loss


def check_hals(got, a, bar, names, launches=""):
    """(worst units, message or None): every element of got within the bar of a["new"] in hals_units, and the zero pattern a["new"]'s
    apart from the excused elements; the message names the worst element as check_elementwise does."""
    u = hals_units(got, a)
    worst = float(u.max())
    msg = None
    if not worst <= bar:
        i = np.unravel_index(np.argmax(u), u.shape)
        msg = (f"{u[i]:.1f} units (bar {bar:g}) at {first_bad(u == u[i], names)}: got {got[i]!r}, want {a['new'][i]!r} (old {a['old'][i]!r}, before the clamp "
               f"{a['pre'][i]!r}; {int((~(u <= bar)).sum())} elements over the bar); launches {launches}")
    else:
        bad = ((np.asarray(got) > 0) != (a["new"] > 0)) & ~hals_excused(a, bar)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            msg = (f"zero pattern differs at {first_bad(bad, names)}: got {got[i]!r}, want {a['new'][i]!r} (before the clamp {a['pre'][i]!r}; "
                   f"{int(bad.sum())} elements); launches {launches}")
    return worst, msg


# ---- what a local error of a sweep kernel does to the restatement (the mutation tests of tests/test_exact_problems.py) -------------
def _best(cands):
    """The candidate (score, ...) with the largest score, or None."""
    cands = [c for c in cands if c[0] > 0]
    return max(cands, key=lambda c: c[0]) if cands else None


def hals_w_mutations(a, plan):
    """name -> corrupt hook for hals_gram_form.w_half: the local errors of a W sweep kernel, each at a site where the reference (a: the
    fp64 half) says it matters -- the unit with the largest change at the step, a later column that is not clamped.  A name is absent
    where the row has no such site (L = 1: HH is diagonal, no step adds to a later one's state)."""
    W = a["W"]
    K, N, L = W.shape
    HH, d, live = a["HH"], a["new"] - a["old"], a["pre"] > 0
    order = lambda j: (j % K) * L + j // K  # the step at which column j = l K + k is swept
    out = {}
    k = K // 2
    cands = []
    for kk in [k] + [x for x in range(K) if x != k]:  # one term d[n] HH[j, j2] of one step never added to G[n, j2]
        for l in range(L):
            j = l * K + kk
            n = int(np.argmax(np.abs(d[kk, :, l])))
            for j2 in np.flatnonzero(HH[j]):
                k2, l2 = j2 % K, j2 // K
                if order(j2) > order(j) and live[k2, n, l2]:
                    cands.append((abs(d[kk, n, l]) * HH[j, j2] / HH[j2, j2], order(j), int(j2)))
        if _best(cands):
            break  # (the middle row where it has a site; on the shortest recordings another row)
    best = _best(cands)
    if best:
        _, s_at, j_drop = best

        def term(stage, x, s_at=s_at, j_drop=j_drop):
            if stage == "step" and x["s"] == s_at:
                x["row"] = x["row"].copy()
                x["row"][j_drop] = 0

        out["term"] = term
    cands = []
    for s in list(range(k * L, min(k * L + L, K * L - 1))) + list(range(K * L - 1)):  # one unit's update of step s + 1 made with the HH row of step s
        if s == 0 and _best(cands):
            break  # (the middle row has a site)
        (k0, l0), (k1, l1) = divmod(s, L), divmod(s + 1, L)
        j0, j1 = l0 * K + k0, l1 * K + k1
        n = int(np.argmax(np.abs(d[k1, :, l1])))
        later = np.array([order(j2) > s + 1 for j2 in range(K * L)])
        cands.append((abs(d[k1, n, l1]) * np.abs(HH[j0] - HH[j1])[later].sum(), s + 1, n, j0))
    best = _best(cands)
    if best:
        _, s_at, n_at, j_old = best

        def stale(stage, x, s_at=s_at, n_at=n_at, j_old=j_old):
            if stage == "step" and x["s"] == s_at:
                x["row_unit"] = (n_at, HH[j_old])

        out["stale_row"] = stale
    if plan["pad_slots"] > 0:  # the last live slot taken for padding at one step: its 64 columns miss that step's update
        K32 = rup(K, 32)
        cols = np.array([l * K + kk for l in range(L) for kk in range(K) if (l * K32 + kk) // 64 == plan["nq"] - 1])
        cands = []
        for l in range(L):
            j = l * K + k
            later = np.array([order(j2) > order(j) for j2 in cols])
            n = int(np.argmax(np.abs(d[k, :, l])))
            cands.append((abs(d[k, n, l]) * HH[j, cols[later]].sum() if later.any() else 0.0, order(j)))
        best = _best(cands)
        if best:
            s_at = best[1]

            def slot(stage, x, s_at=s_at):
                if stage == "step" and x["s"] == s_at:
                    x["row"] = x["row"].copy()
                    x["row"][cols] = 0

            out["slot"] = slot
    return out


def hals_h_mutations(a):
    """name -> corrupt hook for hals_gram_form.h_half: the local errors of an H sweep kernel, at sites the reference says matter.
    Absent where the row has no such site: K = 1 has no cross-row term, L = 1 no edge, no push and (one entry per (n, l)) no cross-row
    tap; "cross_interior" needs a 64-column block that is not the last."""
    import hals_gram_form as hg

    W, H = a["W"], a["H"]
    K, N, L = W.shape
    T = H.shape[1]
    D, live, nrm = a["new"] - a["old"], a["pre"] > 0, a["diag"]
    te0 = max(0, T - L + 1)
    Lt = np.minimum(L, T - np.arange(T))
    out = {}
    if L > 1:
        # a truncated window taken at full length: the norm and the taps of one of the last L - 1 columns
        full = np.array([hg.window_taps(a["PW"], k)[L - 1, k, L - 1] for k in range(K)])
        cands = [(abs(full[k] - nrm[k, t]) * live[k, t], k, t) for k in range(K) for t in range(te0, T) if Lt[t] < L]
        best = _best(cands)
        if best:
            _, k_at, t_at = best

            def window(stage, x, k_at=k_at, t_at=t_at):
                if stage == "row" and x["k"] == k_at:
                    x["Lt"] = x["Lt"].copy()
                    x["Lt"][t_at] = L

            out["window"] = window
        # one same-row push D[t] g[k, e] never added to P[k, t + e]
        cands = []
        for k in range(K):
            tap = hg.window_taps(a["PW"], k)
            if not tap[L - 1, k, L:].any():
                continue  # (this row's windows never overlap themselves at another lag)
            for t in range(T // 2, min(T // 2 + 16, T - 1)):
                for e in range(1, min(L, T - t)):
                    if live[k, t + e]:
                        cands.append((abs(D[k, t]) * tap[Lt[t] - 1, k, e + L - 1] / nrm[k, t + e], k, t, e))
        best = _best(cands)
        if best:
            _, k_at, t_at, e_at = best

            def push(stage, x, k_at=k_at, t_at=t_at, e_at=e_at):
                if stage == "row" and x["k"] == k_at:
                    x["skip_push"].add((t_at, e_at))

            out["push"] = push
    if K > 1 and L > 1:
        nblk = (T + 63) // 64
        k2 = max(0, K // 2 - 1)
        tap = hg.window_taps(a["PW"], k2)
        for name, cols in (("cross_interior", range(64 * (nblk // 2), 64 * (nblk // 2) + 64) if nblk >= 2 and nblk // 2 < nblk - 1 else ()),
                           ("cross_edge", range(64 * (nblk - 1), T))):
            cands = []
            es = np.arange(-(L - 1), L)
            for kt in range(k2 + 1, K):
                for tp in cols:
                    if not live[kt, tp]:
                        continue
                    ts = tp - es
                    ok = (ts >= 0) & (ts < T)
                    if name == "cross_edge" and tp < te0:
                        ok &= ts >= te0
                    tv, ev = ts[ok], es[ok]
                    score = np.abs(D[k2, tv]) * tap[Lt[tv] - 1, kt, ev + L - 1] / nrm[kt, tp]
                    if len(score) and score.max() > 0:
                        i = int(np.argmax(score))
                        cands.append((float(score[i]), kt, int(tv[i]), int(ev[i])))
                if len(cands) >= 8:
                    break  # (the rows next to the source row where they have a site; on sparse lag Grams a later one)
            best = _best(cands)
            if best:
                def cross(stage, x, site=best[1:]):
                    if stage == "row" and x["k"] == k2:
                        x["lose"].add(site)

                out[name] = cross
    return out


# ---- seqNMF's cross-orthogonality penalties on the MU rule (tests/test_gpu_exact_xortho.py; CPU half in tests/test_exact_problems.py) ----
# G = off(S(H)), xW = hxt(G, data), xH = off(S(numH)) and oW = off(Wflat) are sums of non-negative integers on the integer problems, so
# with data % 4 every one of them stays below 2^24 and is exact in fp32 in any order.  The weights are dyadic: lam x, lam2 o, their sum,
# den + pen, + l1 and + 2 l2 x are multiples of 1/8 below 2^21, exact in fp32 under any association and any fma contraction.  What is
# left is cmf_mu's one division and one multiply, so the bar is the 2 ulp of tests/test_exact_parity.py (xortho_preconditions asserts
# all of this from the arrays, and that one unit of every sum moves its element by at least 4 bars).
XO_WEIGHTS = (0.125, 0.5, 0.5)  # (lambda, lambda_H, lambda_W)
XO_XMOD = 4.0                    # data = make_problem's X % 4, as in tests/test_gpu_xortho_mu.py
XO_FOLD_ROW = (1537, 150, 33, 20)  # L K32 Np / 4 = 20 * 64 * 1664 / 4 = 532 480 > 2048 * 256: xo_fold_w_kernel's grid-stride loop comes round again
XO_FOLD_GRID = 2048 * 256       # threads of the fold launch (cmf_xortho.hip xo_fold_w)
XO_ULP_PER_REL = 2.0 ** 23      # a relative change r of a float32 number is at least r 2^23 of its ulp


def make_xortho_problem(N, T, K, L, family, seed=0):
    """make_problem with X % 4."""
    W, H, X = make_problem(N, T, K, L, family, seed)
    return W, H, np.asfortranarray(X % XO_XMOD)


def xo_smooth(A, L):
    """xortho_mu_restatement.smooth as 2 L - 1 shifted adds: every element receives its terms in ascending t', the restatement's order,
    so the two agree bit for bit on any input (tests/test_exact_problems.py)."""
    K, T = A.shape
    out = np.zeros((K, T), dtype=A.dtype)
    for d in range(-(L - 1), L):
        lo, hi = max(0, -d), min(T, T - d)
        if lo < hi:
            out[:, lo:hi] += A[:, lo + d:hi + d]
    return out


def xo_weight_sets(weights=XO_WEIGHTS):
    """All three weights, then each alone."""
    lam, lamH, lamW = weights
    return [weights, (lam, 0.0, 0.0), (0.0, lamH, 0.0), (0.0, 0.0, lamW)]


def xortho_half(family, X, W, H, weights=XO_WEIGHTS, corrupt=None):
    """One update_motifs! (family "W") or update_feature_maps! (family "H") under the penalties in fp64, xortho_mu_restatement's operations
    with the intermediate arrays kept:
      both      est, num, den, S (the window sum on its way into off: S(H) on the W side, S(numH) on the H side), G = off(S(H)), pen,
                den_total = ((((den + pen) + l1) + 2 l2 x) + eps), new
      "W"       xW = hxt(G, data), Wflat, oW = off(Wflat) over every lag
      "H"       A (the table the window reads: numH), xH = off(S(A)), SH = S(H), loss (after the update)
    with L1 and L2 as regularisers.  corrupt(stage, arrays) is called after "sums" (num, den, A), "window" (S), "off" (G on the W side,
    xH on the H side), "contract" (xW), "G" (the H side's G), "oW" and "weights" (a["weights"] is read after it) to damage them in place."""
    import xortho_mu_restatement as xr

    K, N, L = W.shape
    a = dict(W=W, H=H, X=X, family=family, weights=tuple(weights))

    def hook(stage):
        if corrupt:
            corrupt(stage, a)

    a["est"] = xr.tensor_conv(W, H)
    if family == "W":
        a["num"], a["den"] = xr.hxt(H, X, L), xr.hxt(H, a["est"], L)
        hook("sums")
        a["S"] = xo_smooth(H, L)
        hook("window")
        a["G"] = xr.off(a["S"])
        hook("off")
        a["xW"] = xr.hxt(a["G"], X, L)
        hook("contract")
        a["Wflat"] = W.sum(axis=2)
        a["oW"] = np.repeat(xr.off(a["Wflat"])[:, :, None], L, axis=2)
        hook("oW")
    else:
        a["num"], a["den"] = xr.tensor_transconv(W, X), xr.tensor_transconv(W, a["est"])
        a["A"] = a["num"].copy()
        hook("sums")
        a["S"] = xo_smooth(a["A"], L)
        hook("window")
        a["xH"] = xr.off(a["S"])
        hook("off")
        a["SH"] = xo_smooth(H, L)
        a["G"] = xr.off(a["SH"])
        hook("G")
    hook("weights")
    return xortho_finish(a, a["weights"])


def xortho_finish(a, weights, loss=True):
    """pen, den_total, new and (family "H", unless loss=False) loss of xortho_half from its tables under the weights given: a new dict that shares the
    tables (the weights alone change nothing else)."""
    import xortho_mu_restatement as xr

    a = dict(a, weights=tuple(weights))
    lam, lamH, lamW = a["weights"]
    if a["family"] == "W":
        a["pen"] = lam * a["xW"] + lamW * a["oW"]
        x = a["W"]
    else:
        a["pen"] = lam * a["xH"] + lamH * a["G"]
        x = a["H"]
    a["x"] = x
    a["den_total"] = (((a["den"] + a["pen"]) + L1) + (2.0 * L2) * x) + EPS
    a["new"] = np.maximum(x * (a["num"] / a["den_total"]), EPS)
    if a["family"] == "H" and loss:
        a["loss"] = xr.compute_loss(a["X"], a["W"], a["new"])
    return a


def _f32_exact(v):
    return np.array_equal(np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64), v)


def xortho_preconditions(a, what=""):
    """Asserted from the arrays of xortho_half, before any GPU call:
      * every integer table (num, den, est, G, S, xW / A and xH, oW, Wflat) is integral and below 2^24;
      * every stage of the denominator -- lam x, lam2 o, their sum, den + pen, + l1, + 2 l2 x, in the kernels' order (xo_fold_w_kernel /
        xo_off_kernel, then cmf_mu) -- survives the round trip through float32: the stages are then the same numbers under any
        association or fma contraction of them;
      * the smallest positive term of each sum (a unit of num, of den, of xW and of oW; a unit of G and one entry of numH in a window),
        weighted, over the largest den_total (for num: the larger of that and the largest num), is at least 8 ulp = 4 bars.
    Returns {"ulp": {term: ulp}, "weakest": (term, ulp)}."""
    family = a["family"]
    lam, lamH, lamW = a["weights"]
    tables = ["num", "den", "est", "G", "S"] + (["xW", "oW", "Wflat"] if family == "W" else ["A", "xH", "SH"])
    for name in tables:
        t = a[name]
        assert np.all(t == np.rint(t)) and t.min() >= 0 and t.max() < EXACT, f"{what}: {name} is not an integer table below 2^24 (max {t.max()})"
    x_tab, o_tab, lam2 = (a["xW"], a["oW"], lamW) if family == "W" else (a["xH"], a["G"], lamH)
    stages = [("lam x", lam * x_tab), ("lam2 o", lam2 * o_tab)]
    stages.append(("lam x + lam2 o", stages[0][1] + stages[1][1]))
    stages.append(("den + pen", a["den"] + stages[2][1]))
    stages.append(("+ l1", stages[3][1] + L1))
    stages.append(("+ 2 l2 x", stages[4][1] + (2.0 * L2) * a["x"]))
    for name, v in stages:
        assert _f32_exact(v), f"{what}: the denominator stage '{name}' rounds in float32"
    assert np.array_equal(stages[2][1], a["pen"]) and np.array_equal(stages[5][1] + EPS, a["den_total"])
    top = float(a["den_total"].max())
    terms = {"num": 1.0 / max(top, float(a["num"].max())), "den": 1.0 / top}
    data_unit = float(a["X"][a["X"] > 0].min())
    if family == "W":
        if lam > 0:
            terms["xW"] = lam * data_unit / top  # (a unit of G under the smallest positive data entry)
        if lamW > 0:
            terms["oW"] = lamW * float(a["W"][a["W"] > 0].min()) / top
    else:
        if lam > 0:
            terms["numH entry"] = lam * float(a["A"][a["A"] > 0].min()) / top
        if lamH > 0:
            terms["G"] = lamH * float(a["H"][a["H"] > 0].min()) / top
    ulp = {k: v * XO_ULP_PER_REL for k, v in terms.items()}
    weakest = min(ulp.items(), key=lambda kv: kv[1])
    assert weakest[1] >= 8.0, f"{what}: {weakest[0]} moves an element by {weakest[1]:.1f} ulp only (8 asked: 4 bars of 2 ulp)"
    return dict(ulp=ulp, weakest=weakest)


def xortho_configs(configs):
    """The configurations of a table row the penalties accept: no Gram form, one device (both are refused); everything else stays."""
    return [c for c in configs if "gram" not in c and "devices" not in c]


def xo_fold_passes(K32, Np, L):
    """Grid-stride passes of xo_fold_w_kernel over L K32 Np / 4 float4 lanes."""
    n4 = L * K32 * Np // 4
    return -(-n4 // XO_FOLD_GRID)


def xo_tail_contraction(left, X, L, t0):
    """sum over data columns t >= t0 of left[k, t - l] X[n, t]: what the rows behind the last whole ring rotation add to a C2 contraction."""
    K, T = left.shape
    out = np.zeros((K, X.shape[0], L))
    for lag in range(min(L, T)):
        a = max(t0, lag)
        if a < T:
            out[:, :, lag] = left[:, a - lag:T - lag] @ X[:, a:].T
    return out


def xortho_mutations(family, a):
    """name -> corrupt hook for xortho_half: the local errors the penalties' kernels could make, each at one place.  a: the undamaged
    half (for the sites).  Absent where the row has no such site (a 32-block of components needs K > 32)."""
    W, H, X = a["W"], a["H"], a["X"]
    K, N, L = W.shape
    T = H.shape[1]
    src = "H" if family == "W" else "A"  # what the window reads
    b0 = 64 * ((T // 2) // 64)  # one 64-column block of the window kernel, and its seam
    b1 = min(b0 + 64, T)
    seam = b0
    out = {}

    def on(stage, fn):
        def corrupt(st, x):
            if st == stage:
                fn(x)
        return corrupt

    if L > 1:
        def short_lo(x):  # the windows of one block one row short at their lower end
            lo = max(b0, L - 1)
            x["S"][:, lo:b1] -= x[src][:, lo - (L - 1):b1 - (L - 1)]

        def short_hi(x):
            hi = min(b1, T - (L - 1))
            x["S"][:, b0:hi] -= x[src][:, b0 + L - 1:hi + L - 1]

        def seam_cut(x):  # the columns from the seam on never see the rows in front of it
            for t in range(seam, min(seam + L - 1, T)):
                x["S"][:, t] -= x[src][:, max(0, t - (L - 1)):seam].sum(axis=1)

        if max(b0, L - 1) < b1:
            out["window_short_lo"] = on("window", short_lo)
        if b0 < min(b1, T - (L - 1)):
            out["window_short_hi"] = on("window", short_hi)
        if seam > 0:
            out["window_seam"] = on("window", seam_cut)
    out["S_first_column"] = on("window", lambda x: x["S"].__setitem__((slice(None), 0), 0.0))
    out["S_last_column"] = on("window", lambda x: x["S"].__setitem__((slice(None), T - 1), 0.0))
    tab = "G" if family == "W" else "xH"
    c0 = 256 * ((T // 2) // 256)  # one 256-column block of the off kernel
    cols = slice(c0, min(c0 + 256, T))
    kmiss = K // 2

    def off_one(x):
        rows = np.arange(K) != kmiss
        x[tab][rows, cols] -= x["S"][kmiss, cols]

    def off_self(x):
        x[tab][:, cols] += x["S"][:, cols]

    if K > 1:
        out["off_one_component"], out["off_with_itself"] = on("off", off_one), on("off", off_self)
    if K > 32:
        def off_block(x):  # the k block past 32 never reaches the components of the first
            x[tab][:32, cols] -= x["S"][32:, cols].sum(axis=0)

        out["off_one_k_block"] = on("off", off_block)
    if family == "W":
        def stale_G(x):  # G of the H before: the same factor one column earlier
            import xortho_mu_restatement as xr

            x["G"][...] = xr.off(xo_smooth(np.roll(x["H"], 1, axis=1), L))

        def tail_from_H(x):  # the rows behind the last whole ring rotation contracted with H in G's place
            t0 = T - max(1, T % 30 or 30)
            x["xW"] += xo_tail_contraction(x["H"], X, L, t0) - xo_tail_contraction(x["G"], X, L, t0)

        out["G_of_the_previous_H"] = on("off", stale_G)
        out["tail_reads_H"] = on("contract", tail_from_H)
        if L > 1:
            out["oW_first_lag_only"] = on("oW", lambda x: x["oW"].__setitem__((slice(None), slice(None), slice(1, None)), 0.0))
    else:
        def slab_lost(x):  # one C3 slab -- the units of one 8-row chunk on one 128-column block -- never reaches the window's table
            import xortho_mu_restatement as xr

            t1 = min(c0 + 128, T)
            Xc = np.zeros_like(X)
            Xc[:8, c0:min(t1 + L - 1, T)] = X[:8, c0:min(t1 + L - 1, T)]
            x["A"][:, c0:t1] -= xr.tensor_transconv(W, Xc)[:, c0:t1]

        def stale_G(x):
            import xortho_mu_restatement as xr

            x["G"][...] = xr.off(xo_smooth(np.roll(x["H"], 1, axis=1), L))

        def swapped(x):
            lam, lamH, lamW = x["weights"]
            x["weights"] = (lamH, lam, lamW)

        out["slab_lost_before_the_window"] = on("sums", slab_lost)
        out["G_of_the_previous_H"] = on("G", stale_G)
        out["lambda_and_lambda_H_exchanged"] = on("weights", swapped)
    return out


# The penalised rule under plans for fewer compute units (tests/test_gpu_exact_cu_plans.py).  The penalty contraction is a ONE-source C2
# launch with G as the left operand, chunked by its own plan (hxt_chunks with nsrc = 1): the count's own tail row (CU_SHAPES) leaves tail
# rows for the rule's two-source launch, which at 128, 64 and 38 CUs the one-source launch does not -- XO_TAIL_T adds the shortest
# recordings of 130 units (plus 16 columns: a tail of 17 rows, not of one) whose one-source chunks leave a tail too, the rows
# CmfHxtTail reads out of G.
XO_TAIL_T = {128: 1937, 64: 977, 32: 497, 38: 587, 1: 448}
XO_SLAB_ROW_1CU = (130, 700, 32, 20)  # at 1 CU the only row whose C3 launch writes more than one fragment slab


def xo_cu_predicates(N, T, K, L, n_cu):
    """What the plan mirrors say of the general kernels (K > 16) at n_cu: tail / left_tail -- the two-source / the one-source C2 launch
    leaves rows to the slab sum (the latter reads them out of G) --, slabs: the fragment slabs xo_h_tables sums with stride 2 Tl K32."""
    return dict(tail=hxt_chunks(N, T, K, L, 2, n_cu)[2] < T, left_tail=hxt_chunks(N, T, K, L, 1, n_cu)[2] < T, slabs=tc_plan(N, T, K, 2, n_cu)[1])


def xo_cu_rows(n_cu):
    """[(N, T, K, L)]: the count's row that names hxt_kernel:tail, the row of XO_TAIL_T, and a row of more than one C3 slab."""
    rows = [r[:4] for r in CU_SHAPES[n_cu] if "hxt_kernel:tail" in r[5]]
    rows.append((130, XO_TAIL_T[n_cu], 32, 20))
    if not any(xo_cu_predicates(*r, n_cu)["slabs"] > 1 for r in rows):
        rows.append(XO_SLAB_ROW_1CU)
    return list(dict.fromkeys(rows))
