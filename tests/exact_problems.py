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
    nn, tt = np.meshgrid(np.arange(N), np.arange(T), indexing="ij")
    X = (_hash(nn, tt, salt=seed * 4) % np.uint64(XMAX + 1)).astype(np.float64)
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
# tests/test_exact_parity.py expects every one reached, and tests/test_exact_problems.py keeps this list equal to the C++ table.
LAUNCH_PATHS = [
    "conv_kernel", "conv2_kernel", "conv3_kernel:whole", "conv3_kernel:whole+4", "conv3_kernel:whole+16", "conv3_kernel:pieces4",
    "conv3_kernel:pieces16", "conv_small_kernel<1>", "conv_small_kernel<2>", "conv_small_kernel<3>", "conv_small_kernel<4>",
    "conv_small_kernel<6>", "conv_small_kernel<8>", "conv_small_kernel:quarter", "conv_small_kernel:pre", "hxt_kernel<1>",
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


def small_k_plan(N, T, K, L, n_cu=N_CU):
    """(C2 MBW, C2 RV, C3 MBW, C3 RV, C3 pieces NS, conv k pairs) of the few-component kernels (K <= 16, L <= 64)."""
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
    return MBW, RV, MBW3, RV3, NS, (K + 1) // 2
