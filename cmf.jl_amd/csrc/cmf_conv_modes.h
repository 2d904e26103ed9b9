// cmf_conv_modes.h -- the modes of the C1 kernels (the template parameter `int MODE` of conv_*_kernel and launch_conv) by name.
//
// A mode is family + base.  The family says which rule's arithmetic the epilogue applies, the base what it does with the tile:
//
//   base                 0 store [t][n]      1 store' [n][t]      2 loss sum only     3 loss sum + store [t][n]
//   CONV_FAM_PLAIN       est                 est'                 (est - data)^2      both
//   CONV_FAM_MU_MASKED   mask .* est         (mask .* est)'       over mask != 0      both           (p.loss_abs: over mask == 0)
//   CONV_FAM_KL          R = data / e        R'                   KL terms            both           e = est + eps
//   CONV_FAM_KL_MASKED   (unassigned)        (unassigned)         over mask != 0      both           (p.loss_abs: over mask == 0)
//   CONV_FAM_IS          P, Q                P', Q'               IS terms            both           Q = 1 / e, P = (data * Q) * Q
//   CONV_FAM_BETA        P, Q                P', Q'               d_beta terms        both           Q = e^(beta - 1), P = data * e^(beta - 2)
//   CONV_FAM_IS_MASKED   M .* P, M .* Q      (M .* P)', (M .* Q)' over mask != 0      both           (p.loss_abs: over mask == 0)
//   CONV_FAM_BETA_MASKED M .* P, M .* Q      (M .* P)', (M .* Q)' over mask != 0      both           (p.loss_abs: over mask == 0)
//
//   CONV_FAM_PGD         residual + loss     residual'            masked ~ + loss     masked residual'   (p.loss_abs: AbsoluteLoss)
// (KL under a mask stores through the KL family's own modes, given Xm / XmT as data.  The two masked P, Q families are given Xs / XsT,
// the copy of data whose held-out entries hold a negative sentinel: x < 0 IS "held out", no mask tile; only their loss-only mode with
// p.loss_abs, on the raw data, reads the mask.)  The arithmetic: cmf_kernels.h at ConvParams; the
// tile forms: DESIGN.md 4a.  The numbers are part of the kernels' symbol names (conv3_kernel<19> in profiles/): they never change.
#pragma once

enum : int { CONV_FAM_PLAIN = 0, CONV_FAM_PGD = 4, CONV_FAM_MU_MASKED = 8, CONV_FAM_KL = 12, CONV_FAM_KL_MASKED = 16, CONV_FAM_IS = 20, CONV_FAM_BETA = 24,
              CONV_FAM_IS_MASKED = 28, CONV_FAM_BETA_MASKED = 32 };
enum : int { CONV_BASE_STORE = 0, CONV_BASE_STORE_T = 1, CONV_BASE_LOSS = 2, CONV_BASE_LOSS_STORE = 3 };
enum : int { PGD_BASE_RESID = 0, PGD_BASE_RESID_T = 1, PGD_BASE_MASKED_RESID = 2, PGD_BASE_MASKED_RESID_T = 3 }; // the PGD family's own bases

enum : int {
    CONV_EST = 0, CONV_EST_T, CONV_LOSS, CONV_LOSS_EST,                                      // plain (mult.jl:28, :44, :55-57)
    CONV_RESID, CONV_RESID_T, CONV_MASKED_RESID, CONV_MASKED_RESID_T,                        // PGD / HALS residuals (pgd.jl, hals.jl)
    CONV_MUM_EST, CONV_MUM_EST_T, CONV_MUM_LOSS, CONV_MUM_LOSS_EST,                          // the MU rule under a 0/1 mask
    CONV_KL_R, CONV_KL_R_T, CONV_KL_LOSS, CONV_KL_LOSS_R,                                    // KL
    CONV_KLM_LOSS = 18, CONV_KLM_LOSS_R,                                                     // KL under the mask (16, 17 unassigned)
    CONV_IS_PQ, CONV_IS_PQ_T, CONV_IS_LOSS, CONV_IS_LOSS_PQ,                                 // Itakura-Saito
    CONV_BETA_PQ, CONV_BETA_PQ_T, CONV_BETA_LOSS, CONV_BETA_LOSS_PQ,                         // the beta-divergence
    CONV_ISM_PQ, CONV_ISM_PQ_T, CONV_ISM_LOSS, CONV_ISM_LOSS_PQ,                             // Itakura-Saito under the 0/1 mask
    CONV_BETAM_PQ, CONV_BETAM_PQ_T, CONV_BETAM_LOSS, CONV_BETAM_LOSS_PQ                      // the beta-divergence under the 0/1 mask
};

constexpr int conv_family(int m) { return m / 4 * 4; }
constexpr int conv_base(int m) { return m % 4; }
constexpr int conv_mode(int family, int base) { return family + base; }

static_assert(CONV_EST == 0 && CONV_EST_T == 1 && CONV_LOSS == 2 && CONV_LOSS_EST == 3 && CONV_RESID == 4 && CONV_RESID_T == 5 && CONV_MASKED_RESID == 6 &&
              CONV_MASKED_RESID_T == 7 && CONV_MUM_EST == 8 && CONV_MUM_EST_T == 9 && CONV_MUM_LOSS == 10 && CONV_MUM_LOSS_EST == 11 && CONV_KL_R == 12 &&
              CONV_KL_R_T == 13 && CONV_KL_LOSS == 14 && CONV_KL_LOSS_R == 15 && CONV_KLM_LOSS == 18 && CONV_KLM_LOSS_R == 19 && CONV_IS_PQ == 20 &&
              CONV_IS_PQ_T == 21 && CONV_IS_LOSS == 22 && CONV_IS_LOSS_PQ == 23 && CONV_BETA_PQ == 24 && CONV_BETA_PQ_T == 25 && CONV_BETA_LOSS == 26 &&
              CONV_BETA_LOSS_PQ == 27 && CONV_ISM_PQ == 28 && CONV_ISM_PQ_T == 29 && CONV_ISM_LOSS == 30 && CONV_ISM_LOSS_PQ == 31 && CONV_BETAM_PQ == 32 &&
              CONV_BETAM_PQ_T == 33 && CONV_BETAM_LOSS == 34 && CONV_BETAM_LOSS_PQ == 35, "the mode numbers are symbol names: they never change");
static_assert(CONV_MASKED_RESID_T == conv_mode(CONV_FAM_PGD, PGD_BASE_MASKED_RESID_T) && CONV_MUM_LOSS == conv_mode(CONV_FAM_MU_MASKED, CONV_BASE_LOSS) &&
              CONV_KL_R_T == conv_mode(CONV_FAM_KL, CONV_BASE_STORE_T) && CONV_KLM_LOSS_R == conv_mode(CONV_FAM_KL_MASKED, CONV_BASE_LOSS_STORE) &&
              CONV_IS_LOSS == conv_mode(CONV_FAM_IS, CONV_BASE_LOSS) && CONV_BETA_LOSS_PQ == conv_mode(CONV_FAM_BETA, CONV_BASE_LOSS_STORE) &&
              CONV_ISM_LOSS == conv_mode(CONV_FAM_IS_MASKED, CONV_BASE_LOSS) && CONV_BETAM_PQ_T == conv_mode(CONV_FAM_BETA_MASKED, CONV_BASE_STORE_T), "a mode is family + base");

constexpr bool conv_pgd(int m) { return conv_family(m) == CONV_FAM_PGD; }             // the residual modes
constexpr bool conv_plain(int m) { return conv_family(m) == CONV_FAM_PLAIN; }
constexpr bool conv_mu_masked(int m) { return conv_family(m) == CONV_FAM_MU_MASKED; } // the 0/1 mask of the MU rule: a select
constexpr bool conv_kl_masked(int m) { return conv_family(m) == CONV_FAM_KL_MASKED; } // the KL terms under that mask: a select
constexpr bool conv_kl(int m) { return conv_family(m) == CONV_FAM_KL || conv_kl_masked(m); } // R = data / (est + eps) stored, the divergence summed
// Itakura-Saito and beta under the MU rule's 0/1 mask: held-out entries store exact 0 in P and in Q and add 0, by a select.  The data
// operand of the storing modes and of the training loss is the sentinel copy (held out = negative, conv_pq_sentinel)
constexpr bool conv_pq_masked(int m) { return conv_family(m) == CONV_FAM_IS_MASKED || conv_family(m) == CONV_FAM_BETA_MASKED; }
constexpr bool conv_is(int m) { return conv_family(m) == CONV_FAM_IS || conv_family(m) == CONV_FAM_IS_MASKED; }       // P and Q stored, the divergence summed
constexpr bool conv_beta(int m) { return conv_family(m) == CONV_FAM_BETA || conv_family(m) == CONV_FAM_BETA_MASKED; } // the same with the powers of the beta-divergence
// the families whose ONE accumulator tile stores TWO arrays (P -> p.out, Q -> p.out2) from the data tile, with the padding columns
// selected to exact 0 (Q of an empty column is not 0): an epilogue of their own (conv_pq_epilogue_), the arithmetic per family (ConvPQ)
constexpr bool conv_pq(int m) { return conv_is(m) || conv_beta(m); }
constexpr bool conv_transposed(int m) { return conv_pgd(m) ? conv_base(m) % 2 == 1 : conv_base(m) == CONV_BASE_STORE_T; } // stores in the [n][t] layout
constexpr bool conv_writes_loss(int m) { return conv_pgd(m) ? conv_base(m) % 2 == 0 : conv_base(m) >= CONV_BASE_LOSS; } // a per-tile sum -> partial[]
constexpr bool conv_stores(int m) { return conv_pgd(m) || conv_base(m) != CONV_BASE_LOSS; }
constexpr bool conv_stores_tn(int m) { return conv_stores(m) && !conv_transposed(m); }   // ... in the [t][n] layout
constexpr bool conv_reads_mask(int m) { return conv_mu_masked(m) || conv_kl_masked(m) || (conv_pq_masked(m) && conv_base(m) == CONV_BASE_LOSS) || (conv_pgd(m) && conv_base(m) >= PGD_BASE_MASKED_RESID); }
constexpr bool conv_mask_transposed(int m) { return conv_reads_mask(m) && conv_transposed(m); }     // MT [n][t] instead of M [t][n]
constexpr bool conv_reads_data(int m) { return conv_pgd(m) || conv_kl(m) || conv_pq(m) || conv_base(m) >= CONV_BASE_LOSS; }
constexpr bool conv_data_transposed(int m) { return conv_reads_data(m) && conv_transposed(m); }     // XT [Np][TP] instead of X [TP][Np]
constexpr bool conv_reads_tile(int m) { return conv_reads_data(m) || conv_reads_mask(m); }          // (everything but est and est')
constexpr bool conv_loss_abs_is_absolute_loss(int m) { return conv_pgd(m); }          // store sign(est - data) [.* mask], sum |.|  (pgd.jl:41-47)
constexpr bool conv_loss_abs_is_complement(int m) { return (conv_mu_masked(m) || conv_kl_masked(m) || conv_pq_masked(m)) && conv_base(m) == CONV_BASE_LOSS; } // sum over mask == 0
// the masked P, Q modes decide "observed" from the data value itself: !(x < 0).  Their data is the sentinel copy; the held-out score
// (loss only, p.loss_abs, raw data) turns the entries its mask tile deselects into the sentinel first, so one rule serves every mode
constexpr bool conv_pq_sentinel(int m) { return conv_pq_masked(m); }
// PRE: the data tile requested before the MFMA loop of a short few-component launch (conv3_tile): the loss + store modes
constexpr bool conv_has_pre(int m) { return !conv_pgd(m) && conv_base(m) == CONV_BASE_LOSS_STORE; }
// The 128 x 128 tiles (conv2_kernel) exist for the epilogues that only store or only sum without a second operand tile beside the
// data: with a data tile read AND a store they need more than the 168 registers three workgroups per CU leave (launch_conv).
// (The loss-only modes of the masked P, Q families are on them too: their held-out score, p.loss_abs, does load the mask tile beside
// the data, but folds each value into its data register at once -- cmf_pq_held_out -- so no second tile stays live: 165 registers.)
constexpr bool conv_on_tiles128(int m) { return (conv_plain(m) || conv_mu_masked(m)) ? conv_base(m) != CONV_BASE_LOSS_STORE : (conv_family(m) == CONV_FAM_KL || conv_pq(m)) && conv_base(m) == CONV_BASE_LOSS; }
// four few-component tiles per SIMD instead of three (conv_small_kernel's launch bounds): the epilogues light enough in registers
constexpr bool conv_small_four_per_simd(int m) { return m == CONV_EST || m == CONV_EST_T || m == CONV_RESID_T; }
