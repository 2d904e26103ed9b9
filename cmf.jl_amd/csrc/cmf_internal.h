#pragma once
// cmf_api.hip -- host side of libcmf_hip.so: the C ABI of include/cmf_hip.h over the gfx950
// kernels in cmf_kernels.h.  No CPU fallback exists: every compute entry needs a HIP device.
#pragma GCC visibility push(default) // (the library is built with -fvisibility=hidden: only the C ABI is exported)
#include "cmf_hip.h"
#pragma GCC visibility pop
#include "cmf_kernels.h"
#include "cmf_rng.h"
#include "cmf_writeback.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
inline thread_local std::string g_err; // (one per thread for the whole library: C++17 inline variable)

static int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// The library's test hooks (include/cmf_hip.h lists them): integer variables of the environment that count ONLY together with
// CMF_TEST_HOOKS=1, so that a stray variable in a production environment changes nothing.  Read by the calling thread at public
// entries only (getenv is not safe against a concurrent setenv of the host program).
static bool test_hooks_on()
{
    const char *hooks = getenv("CMF_TEST_HOOKS");
    return hooks && atoi(hooks) == 1;
}
static long long test_hook(const char *name, long long dflt)
{
    if (!test_hooks_on()) return dflt;
    const char *e = getenv(name);
    return e ? atoll(e) : dflt;
}
// CMF_TEST_N_CU: the CU count the plan of every handle a creating call makes is dealt for (create_impl), in 1 ... the device's own count.
// Read by the creating entry (cmf_create, cmf_create_shard, cmf_create_multi) and handed down to create_impl; kNoCuHook: not asked for.
constexpr long long kNoCuHook = -(1LL << 62);
static inline long long n_cu_hook() { return test_hook("CMF_TEST_N_CU", kNoCuHook); }

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(CMF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define KCHK(name)                                                                                \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess)                                                                     \
            return fail(CMF_ERR_HIP, "launch of %s failed: %s", name, hipGetErrorString(e_));     \
    } while (0)
#define CMFTRY(expr)              \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != CMF_OK) return rc_; \
    } while (0)

static inline int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// The timed repetition of cmf_time_kernel: one warm-up call of `once`, then `reps` calls between ev0 and ev1 on `stream`; *avg_ms = the
// events' span per call.  `once` returns a CMF code and leaves the device of `stream` current; the first failure ends the measurement.
template <class F> static int timed_reps(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, int reps, F once, double *avg_ms)
{
    CMFTRY(once()); // warm-up
    HIPCHK(hipEventRecord(ev0, stream));
    for (int r = 0; r < reps; ++r) CMFTRY(once());
    HIPCHK(hipEventRecord(ev1, stream));
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    *avg_ms = (double)ms / reps;
    return CMF_OK;
}

// ------------------------------------------------------------------------------------------
// roctx ranges (tracing)
// ------------------------------------------------------------------------------------------
// The phases of an iteration and every collective are bracketed with roctx ranges on the thread that enqueues them, so that
// a `rocprofv3 --marker-trace --kernel-trace` timeline of a multi-GPU run reads as "W phase | all-reduce | H phase | halo
// all-gather | loss conv" per shard.  The marker library is bound at run time and only when it is wanted: a copy the
// process has already mapped (the profiler preloads it) is used, CMF_ROCTX=1 loads it on request; otherwise a range is
// two predictable branches.
#include <dlfcn.h>
struct RoctxApi {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
static const RoctxApi &roctx_api()
{
    static const RoctxApi api = [] {
        RoctxApi a;
        const char *env = getenv("CMF_ROCTX");
        if (env && atoi(env) == 0 && *env) return a; // CMF_ROCTX=0: never
        void *dl = nullptr;
        for (const char *nm : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            dl = dlopen(nm, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
            if (dl) break;
        }
        if (!dl && env && atoi(env) == 1)
            for (const char *nm : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/libroctx64.so.4"}) {
                dl = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
                if (dl) break;
            }
        if (!dl) return a;
        a.push = reinterpret_cast<int (*)(const char *)>(dlsym(dl, "roctxRangePushA"));
        a.pop = reinterpret_cast<int (*)()>(dlsym(dl, "roctxRangePop"));
        if (!a.push || !a.pop) a.push = nullptr, a.pop = nullptr;
        return a;
    }();
    return api;
}
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char *name) : on(roctx_api().push != nullptr)
    {
        if (on) roctx_api().push(name);
    }
    RoctxRange(const char *fmt, int a) : on(roctx_api().push != nullptr)
    {
        if (!on) return;
        char buf[96];
        snprintf(buf, sizeof(buf), fmt, a);
        roctx_api().push(buf);
    }
    ~RoctxRange()
    {
        if (on) roctx_api().pop();
    }
};

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
// Launch paths of the contraction kernels (cmf_get_counter "launches:<name>"): a per-handle count per path, incremented on the
// host at the launch site -- no device work, no change to any plan.  Instances and forms are counted separately (a launch of
// hxt_kernel<5> with two sources and tail rows adds one to each of "hxt_kernel<5>", "hxt_kernel:nsrc2" and "hxt_kernel:tail"), so
// that a test can reach every name with a handful of shapes.  tests/test_exact_parity.py expects exactly this list.
enum { LA_CONV = 0, LA_CONV2, LA_CONV3_WHOLE, LA_CONV3_WHOLE_P4, LA_CONV3_WHOLE_P16, LA_CONV3_P4, LA_CONV3_P16,
       LA_CONV_SMALL, /* + 6: NKP 1, 2, 3, 4, 6, 8 */ LA_CONV_SMALL_Q = LA_CONV_SMALL + 6, LA_CONV_SMALL_PRE, LA_CONV_SMALL_WHOLE,
       LA_HXT, /* + 7: kHxtLP */ LA_HXT_NSRC1 = LA_HXT + 7, LA_HXT_NSRC2, LA_HXT_TAIL, LA_HXT_NO_TAIL,
       LA_TC, /* + 8: LT 4 .. 32 */ LA_TC_FRONT = LA_TC + 8, LA_TC_XCD,
       LA_HXT_SMALL, /* + 10: MBW 1 .. 10 */ LA_HXT_SMALL_RV = LA_HXT_SMALL + 10, /* + 3 */
       LA_GFOLD = LA_HXT_SMALL_RV + 3, /* + 6: MBW 1 .. 6 */ LA_GFOLD_RV = LA_GFOLD + 6, /* + 3 */ LA_GFOLD_SPLIT = LA_GFOLD_RV + 3, LA_GFOLD_FUSED_H,
       LA_GRAM_W, LA_GRAM_CORR, LA_GRAM_TAPS, LA_GRAM_H_MFMA, LA_GRAM_H,
       LA_SLAB_SUM, LA_SLAB_SUM_CARRY, LA_SLAB_SUM_SMALL, LA_SLAB_SUM_SMALL_CARRY,
       LA_HALO_PACK2, LA_HALO_UNPACK2, LA_HALO_PACK3, LA_HALO_UNPACK3, LA_NCLS };
static const char *const kLaunchNames[] = {
    "conv_kernel", "conv2_kernel", "conv3_kernel:whole", "conv3_kernel:whole+4", "conv3_kernel:whole+16", "conv3_kernel:pieces4", "conv3_kernel:pieces16",
    "conv_small_kernel<1>", "conv_small_kernel<2>", "conv_small_kernel<3>", "conv_small_kernel<4>", "conv_small_kernel<6>", "conv_small_kernel<8>",
    "conv_small_kernel:quarter", "conv_small_kernel:pre", "conv_small_kernel:whole",
    "hxt_kernel<1>", "hxt_kernel<2>", "hxt_kernel<3>", "hxt_kernel<4>", "hxt_kernel<5>", "hxt_kernel<6>", "hxt_kernel<8>",
    "hxt_kernel:nsrc1", "hxt_kernel:nsrc2", "hxt_kernel:tail", "hxt_kernel:no_tail",
    "transconv_kernel<4>", "transconv_kernel<8>", "transconv_kernel<12>", "transconv_kernel<16>", "transconv_kernel<20>", "transconv_kernel<24>",
    "transconv_kernel<28>", "transconv_kernel<32>", "transconv_kernel:front_block", "transconv_kernel:xcd",
    "hxt_small_kernel<1>", "hxt_small_kernel<2>", "hxt_small_kernel<3>", "hxt_small_kernel<4>", "hxt_small_kernel<5>", "hxt_small_kernel<6>",
    "hxt_small_kernel<7>", "hxt_small_kernel<8>", "hxt_small_kernel<9>", "hxt_small_kernel<10>",
    "hxt_small_kernel<1,RV>", "hxt_small_kernel<2,RV>", "hxt_small_kernel<3,RV>",
    "g_gemm_fold_small_kernel<1>", "g_gemm_fold_small_kernel<2>", "g_gemm_fold_small_kernel<3>", "g_gemm_fold_small_kernel<4>",
    "g_gemm_fold_small_kernel<5>", "g_gemm_fold_small_kernel<6>",
    "g_gemm_fold_small_kernel<1,RV>", "g_gemm_fold_small_kernel<2,RV>", "g_gemm_fold_small_kernel<3,RV>",
    "g_gemm_fold_small_kernel:split", "g_gemm_fold_small_kernel:fused_h",
    "gram_w_kernel", "gram_lag_corr", "gram_w_taps", "gram_h_mfma_kernel", "gram_h_kernel",
    "slab_sum_kernel", "slab_sum_kernel:carry", "slab_sum_small_kernel", "slab_sum_small_kernel:carry",
    "halo_pack2_kernel", "halo_unpack2_kernel", "halo_pack3_kernel", "halo_unpack3_kernel"};
static_assert(sizeof(kLaunchNames) / sizeof(kLaunchNames[0]) == LA_NCLS, "one name per launch path");

// Launch paths of the HALS entries (cmf_rules.hip), a table of its own answered by the same cmf_get_counter "launches:<name>" and
// counted the same way: on the host at the launch site, instances and forms separately (a chased persistent sweep with three pullers
// per row adds one to "hals_h_persist_kernel", "hals_h_persist_kernel:P3", "hals_h_persist_kernel:chased" and "conv3_chase_kernel").
// tests/test_exact_problems.py keeps exact_problems.HALS_LAUNCH_PATHS equal to this list; tests/test_gpu_exact_hals.py reaches every name.
enum { HL_W_REG = 0, /* + 10: NQ 2 .. 32 (kHalsNQ) */ HL_W_GEN = HL_W_REG + 10,
       HL_G_RESID, HL_G_DIFF, HL_G_SPEC, HL_W_SPECULATE,
       HL_P_INIT_DEN, HL_P_INIT_RESID, HL_P_INIT_SNAP,
       HL_PERSIST, /* + 4: P 1 .. 4 */ HL_PERSIST_CHASED = HL_PERSIST + 5, HL_CHASE, HL_CHASE_REST,
       HL_STAGE, HL_STAGE_LAG2, HL_STAGE_LAG3, HL_ROW_GEN, HL_PUSH_GEN, HL_NCLS };
static const int kHalsNQ[10] = {2, 4, 6, 8, 10, 12, 16, 20, 24, 32};
static const char *const kHalsLaunchNames[] = {
    "hals_w_sweep_reg_kernel<2>", "hals_w_sweep_reg_kernel<4>", "hals_w_sweep_reg_kernel<6>", "hals_w_sweep_reg_kernel<8>", "hals_w_sweep_reg_kernel<10>",
    "hals_w_sweep_reg_kernel<12>", "hals_w_sweep_reg_kernel<16>", "hals_w_sweep_reg_kernel<20>", "hals_w_sweep_reg_kernel<24>", "hals_w_sweep_reg_kernel<32>",
    "hals_w_sweep_gen_kernel",
    "hals_g:residual", "hals_g:difference", "hals_g:speculated", "hals_w_speculate",
    "hals_p_init_kernel:den", "hals_p_init_kernel:residual", "hals_p_init_kernel:snapshot",
    "hals_h_persist_kernel", "hals_h_persist_kernel:P1", "hals_h_persist_kernel:P2", "hals_h_persist_kernel:P3", "hals_h_persist_kernel:P4",
    "hals_h_persist_kernel:chased", "conv3_chase_kernel", "conv3_chase_kernel:rest",
    "hals_h_stage_kernel", "hals_h_stage_kernel:lag2", "hals_h_stage_kernel:lag3", "hals_h_row_gen_kernel", "hals_h_push_gen_kernel"};
static_assert(sizeof(kHalsLaunchNames) / sizeof(kHalsLaunchNames[0]) == HL_NCLS, "one name per HALS launch path");

#include "cmf_mu_install.h" // CMF_DIV_BETA; what each divergence needs to be installed and when a request is refused (free of HIP)
#include "cmf_options.h"    // the table of cmf_set_option and the options a handle stores as values (CmfOptionFields; free of HIP)

// What est / estT hold for the resident W, H (cmf_handle_s::est_kind): a reader recomputes on a mismatch, every writer passes through set_est.
enum EstKind : int {
    EST_NONE = 0,            // nothing
    EST_CONV = 1,            // tensor_conv(W,H)
    EST_RESID = 2,           // tensor_conv(W,H) - data
    EST_RESID_MASKED = 3,    // mask .* (tensor_conv(W,H) - data)
    EST_SIGN = 4,            // sign(tensor_conv(W,H) - data)  (the AbsoluteLoss gradient)
    EST_SIGN_MASKED = 5,     // mask .* sign(...)
    EST_MU_MASKED = 6,       // mask .* tensor_conv(W,H)  (the MU rule under a mask)
    EST_KL_R = 7,            // data ./ (tensor_conv(W,H) + eps)  (the KL form of the MU rule)
    EST_KL_R_MASKED = 8,     // Xm ./ (tensor_conv(W,H) + eps)  (R of the KL form under a mask: exactly 0 where the mask is 0)
    EST_IS_PQ = 9,           // P of the Itakura-Saito form (and est2 holds Q)
    EST_BETA_PQ = 10,        // P of the beta form for the installed beta (and est2 holds Q); a change of beta voids it
    EST_IS_PQ_MASKED = 11,   // mask .* P of the Itakura-Saito form under a mask (and est2 holds mask .* Q)
    EST_BETA_PQ_MASKED = 12  // the same of the beta form
};
// the residual the PGD rule keeps (resid_and_loss): masked by MaskedLoss, its sign under AbsoluteLoss
static inline int pgd_est_kind(bool masked, bool loss_abs) { return EST_RESID + (masked ? 1 : 0) + (loss_abs ? 2 : 0); }
static_assert(EST_RESID_MASKED == EST_RESID + 1 && EST_SIGN == EST_RESID + 2 && EST_SIGN_MASKED == EST_RESID + 3, "pgd_est_kind");

struct cmf_handle_s : CmfOptionFields {
    int device = 0;
    CmfDims d{};
    int64_t t_offset = 0, T_global = 0;
    int halo_r = 0;       // data / H right halo columns actually present (0 on the last shard)
    bool has_left = false; // a left neighbour exists (t_offset > 0)
    bool sharded = false;

    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    float *H = nullptr, *Ht = nullptr, *Wt = nullptr, *Wn = nullptr;
    float *X = nullptr, *XT = nullptr, *est = nullptr, *estT = nullptr;
    float *wslabs = nullptr; // [nchunks][2][L][K32][Np]
    float *numden = nullptr; // [2][L][K32][Np]   (summed; the all-reduce buffer)
    float *numden_own = nullptr;
    float *hslabs = nullptr; // [S][2][Tl][K32]
    float *halo[4] = {nullptr, nullptr, nullptr, nullptr};
    float *halo_own[4] = {nullptr, nullptr, nullptr, nullptr};
    double *partial = nullptr; // loss partials
    double *d_scalar = nullptr; // device double[4]
    double *d_scalar_own = nullptr;
    double *h_scalar = nullptr; // pinned host double[4]
    double *stage = nullptr;    // fp64 staging for layout conversion
    size_t stage_elems = 0;

    // launch plans
    int hxt_LP = 1, hxt_groups = 1, hxt_nchunks = 1, hxt_chunk_len = 2;
    int tc_LT = 4, tc_S = 1, tc_W = 4;   // fragment slabs and participating waves of the two-source transconv
    int tc_S1 = 1, tc_W1 = 4;            // ... when only one source is contracted
    int tc_S2 = 1, tc_W2 = 4;            // ... two sources with one more 128-column block in FRONT of the own columns (shards that carry the halo of H in
                                         // the W-phase all-reduce update the L-1 columns in front of their own themselves: cmf_groups.hip)
    int halo_ext = 0;                    // that form is possible on this handle: L-1 (a shard with a left neighbour, the one-wave conv tiles, L-1 <= 64), else 0
    bool left_data = false;              // the L-1 columns of data in front of the own block are resident (data' only: the transconv's operand)
    std::vector<int4> tc_tab_host[3];    // per-wave work tables of the variants ([0]: two sources, [1]: one, [2]: two sources + the block in front)
    int4 *tc_tab[3] = {nullptr, nullptr, nullptr};
    int hxt_nchunks1 = 1, hxt_chunk_len1 = 6; // time chunks when only one source is contracted
    int hxt_main = 0, hxt_main1 = 0;          // rows the C2 kernel contracts in the two forms; the < 6*LP rows behind them are added by the slab sum
    // few components (K <= 16): the contractions on the flattened (lag, component) index (cmf_small_k.h)
    bool small_k = false;                   // option "small_k" (default on where the shape allows it)
    bool small_k_ok = false;                // the shape allows it
    bool sk_tc_ok = false, sk_tc = false;   // ... and its C3 form (G GEMM + fold) has enough columns to fill the chip; sk_tc: in use
    int sk_J = 0, sk_JP = 0, sk_MG = 1, sk_MBW = 4, sk_chunk_len = 16, sk_ngroups = 1, sk_TG = 128;
    int sk_RV = 0;                          // C2: the last sk_RV rows j on the VALU instead of in a padded MFMA block (hxt_small_kernel)
    int sk3_MG = 1, sk3_MBW = 4, sk3_Kg = 1, sk3_JP = 128; // C3: whole components per row group (g_gemm_fold_small_kernel)
    int sk3_NS = 1, sk3_RPS = 1;            // short recordings: C3's reduction over n in sk3_NS pieces of sk3_RPS rounds of 8 rows (2 slabs per piece)
    int sk3_GR = 128, sk3_RV = 0;           // rows of a row group in Wj (32-row blocks); the last sk3_RV live rows on the VALU (sk3_MBW then counts the MFMA blocks only)
    float *sk_slabs = nullptr, *sk_Wj = nullptr;
    int *sk_cnt = nullptr;                  // ticket counters of the fused few-component launches (one per 128-column block of H; zero between launches)
    int64_t sk_fused_h = 0;                 // cmf_get_counter "small_k_fused_h_updates"
    int64_t sk_wj_gen = -1;                 // est_gen at which sk_Wj was packed from the resident W (w_update_small_kernel, wj_pack_kernel): every writer of W
                                            // passes through set_est, so a stale operand cannot be taken for a fresh one (-1: never packed)
    int tc_S_full = 1, tc_S1_full = 1;      // fragment slabs of the general transconv kernel (tc_S / tc_S1 are 1 while small_k is on)
    int conv_gx = 1, conv_gy = 1, conv_gy_ext = 1;
    int conv_partials = 1;  // loss partials written by the last conv launch
    int n_cu = 256;

    // HALS scratch (allocated on first use)
    bool hals_ready = false;
    bool gram_ready = false;                // the scratch the Gram form and HALS share (gram_ensure)
    int hals_NpH = 0, hals_NpC = 0, hals_TPp = 0, hals_ne = 0, hals_t_edge0 = 0, hals_corr_R = 4;
    float *hals_HX = nullptr, *hals_cslabs = nullptr, *hals_C = nullptr, *hals_HH = nullptr, *hals_PT = nullptr, *hals_D = nullptr;
    float *hals_PW = nullptr, *hals_GW = nullptr, *hals_GE = nullptr, *hals_GWt = nullptr;
    int hals_seg = 256, hals_nseg = 1;      // column segments of the pipelined H sweep
    bool hals_w_general = false, hals_h_general = false; // shapes beyond the on-chip sweeps' limits: the general sweep kernels
    // The residual conv CHASING the row pipeline (option "hals_chase" = per cent of its tile rows, 0 = off): the pipeline runs on a
    // stream masked to the CUs its K + (K-1)P workgroups need, the first tile rows of the conv on a stream masked to the other CUs,
    // each tile waiting for the last row's progress flag (conv3_chase_kernel); the rest of the conv follows on the whole chip.
    hipStream_t hals_sA = nullptr, hals_sB = nullptr; // CU-masked: pipeline | chasing conv (created at the first chased sweep)
    hipEvent_t hals_ev[3] = {nullptr, nullptr, nullptr}; // fork, pipeline done, chasing part done
    int hals_mask_aper = 0;                 // CUs per XCD the pipeline's stream is masked to (the streams are remade when the plan changes)
    int hals_cuB = 0;                       // CUs of the chasing stream (the launch plans its tail pieces for them)
    int hals_chased_rows = 0, hals_chased_partials = 0; // tile rows / loss partials the chasing launch of the sweep in flight covers (0: none)
    int hals_pullers = 0;                   // persistent H pipeline: puller workgroups per row (0 = stage pipeline)
    int *hals_flags = nullptr;              // its progress flags (device)
    int *hals_status = nullptr;             // pinned host word: 1 = a wait of the persistent pipeline ran out
    float *hals_snap = nullptr;             // [2][TP][K32]: H and Ht as they were when the persistent sweep started
    double hals_l1 = 0.0, hals_l2 = 0.0;    // regularisers of the sweep in flight (for a rerun)
    int64_t hals_reruns = 0;                // H sweeps redone on the stage pipeline after such an expiry (cmf_get_counter)
    int64_t hals_masked_convs = 0;          // mode-6 / mode-7 conv launches of the HALS entries under a mask (cmf_get_counter "hals_masked_convs")
    int64_t hals_resid_gen = -1;            // est_gen at which the HALS entries stored mask .* (est - Xm): the PGD rule's masked residual has the same kind
                                            // but reads the raw data, whose held-out entries may hold anything, so only this one is taken as current

    // PGD rule state (pgd.jl:139-154)
    double pgd_stepW = 5.0, pgd_stepH = 5.0, pgd_cur_loss = -1.0;
    float *pgd_gradH = nullptr;
    int pgd_loss_abs = 0;      // 0 SquareLoss (pgd.jl:29-36), 1 AbsoluteLoss (pgd.jl:41-47)
    double *pgd_knorm = nullptr; // [K32] per-component sums of squares of UnitNormConstraint (pgd.jl:100-110)
    float *M = nullptr, *MT = nullptr; // mask of MaskedLoss (pgd.jl:58-70) in the layouts of X and XT; null = no mask
    // the forms of the MU rule (kMuForms below says what each contracts).  Under a mask of cmf_mu_set_mask: M / MT hold 0 and 1,
    // Xm / XmT = select(mask, data, 0) in the layouts of X and XT; cmf_set_mask switches it off again
    bool mu_mask = false;
    float *Xm = nullptr, *XmT = nullptr;
    double xm_sumsq = 0.0, xm_norm = 0.0; // sum of Xm^2 and its root: what the masked MU loss is divided by
    int mu_div = 0;              // CMF_DIV_SQUARE / CMF_DIV_KL / CMF_DIV_IS (cmf_mu_set_divergence), CMF_DIV_BETA (cmf_mu_set_beta_divergence)
    double mu_beta = 0.0;        // the beta of CMF_DIV_BETA
    float mu_gamma = 1.f;        // ... and its step exponent (1: the element-wise kernels of the plain rule)
    int64_t pow_launches = 0;    // launches of w_update_pow_kernel / h_update_pow_kernel (cmf_get_counter "pow_update_launches")
    float beta_consts[11] = {};  // ... and what its convs read, in the order of ConvParams::beta_m1 .. beta_c
    double data_sum = 0.0;       // what the divergence is divided by: sum(data) (under a mask: sum(Xm)); Itakura-Saito: N * Tl, the mean per entry
    float *kl_denH = nullptr;    // [Tl][K32]: denomH[k, t] broadcast for h_update_kernel
    double *kl_sums = nullptr;   // [K32 * max(L, KL_HCHUNKS)]: row sums of H in chunks / sums over n of W per (lag, k)
    float *Xs = nullptr, *XsT = nullptr; // while the Itakura-Saito / beta forms and a mask are both installed (option "pq_mask"): data with a negative sentinel at the held-out entries, in the layouts of X and XT
                                         // (what the masked P, Q convs read: conv_pq_sentinel); data_sum then holds the observed count
    float *est2 = nullptr, *est2T = nullptr; // Q = 1 ./ e of the Itakura-Saito form beside P in est / estT: [TP][Np] / [Np][TP], zero-filled; allocated when the form is first installed, kept until the handle goes

    double data_sumsq = 0.0, data_norm = 0.0;
    bool factors_set = false;
    bool have_data = false;
    float *gram_numden_h = nullptr; // [1][2][Tl][K32]: numH | denomH in the h_update slab layout
    // in-loop kernel timing (option "profile"): HIP event pairs around the contraction launches, on the launch stream
    bool prof = false;
    int prof_every = 1;          // bracket every n-th launch of a class (option value n)
    int prof_seen[32] = {0};
    int64_t launches[LA_NCLS] = {0}; // cmf_get_counter "launches:<name>" (kLaunchNames)
    int64_t hals_launches[HL_NCLS] = {0}; // ... of the HALS entries (kHalsLaunchNames)
    struct ProfRec { hipEvent_t a, b; int cls; };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    int est_kind = EST_NONE; // what est[t][n] holds for the resident W, H (EstKind)
    void *arena = nullptr;  // the small buffers of the handle as ONE device allocation (cmf_create): 21 hipFree calls cost 1.3 ms, one 0.16
    size_t arena_bytes = 0;
    bool streams_may_hang = false;  // set on the shards of a FAILED group: their streams are not waited for when they are given back
    int64_t est_gen = 0;    // counts the assignments of est_kind (set_est): whatever changes H, W or est passes through one
    int64_t spec_gen = -1;  // est_gen for which the C2 contraction of the NEXT update_motifs! has already been enqueued (w_speculate); -1: none
    int last_rule_call = 0; // 1: cmf_update_motifs, 2: cmf_update_feature_maps (MU rule, single handle): speculation follows the alternation only
    std::function<int()> after_reduce;  // run once by the next reduce_partials between its launch and its wait for the sum (the HALS rule's speculation)
    int64_t hals_spec_gen = -1; // est_gen for which G (the C2 contraction on the residual) and HH of the NEXT HALS update_motifs! have been enqueued; -1: none
    int64_t spec_hits = 0;  // update_motifs! calls that found their contraction done (cmf_get_counter "speculated_contractions")

    // T-sharded groups (cmf_group.h): the handle the caller holds fronts a group when `group` is set
    struct cmf_group_s *group = nullptr;
    bool root_only = false;               // cmf_create_multi's front handle: no device state of its own
    hipStream_t own_comm_stream = nullptr, comm_stream = nullptr; // overlap form: the numW all-reduce runs here
    hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;
    // pipelined loss read-back of cmf_iterate (single handle): two pinned slots + events
    double *h_ring = nullptr;
    bool dev_stamps = false;              // set by cmf_fit around its pipelined batch: time_hist from HIP timing events on the stream
    CmfLossCarry carry{};                 // a loss reduction waiting for the next W phase's slab sum (cmf_iterate only)
    CmfWriteback *wb = nullptr;           // cmf_arm_writeback: the factors written into the caller's arrays behind a rule call
    struct AdmmState *admm = nullptr;     // the ADMM rule's fp64 state (cmf_admm_prepare; cmf_admm.hip)
    struct AnlsState *anls = nullptr;     // the ANLS rule's fp64 state (cmf_anls_prepare; cmf_anls.hip)
    struct SepState *sep = nullptr;       // the separable fit's fp64 state (cmf_sep_prepare; cmf_sep.hip)
    // seqNMF's cross-orthogonality penalties on the squared-error MU rule (cmf_mu_set_xortho; cmf_xortho.hip): the weights lambda, lambda_H, lambda_W
    // (all 0: today's path, launch for launch), the tables of the penalty terms (allocated with the first non-zero weight or the first
    // cmf_mu_xortho_cost / cmf_mu_xortho_terms) and the launches of the kernels of cmf_xortho.h (cmf_get_counter "xortho_launches")
    double xo_lam[3] = {0.0, 0.0, 0.0};
    struct XoState *xo = nullptr;
    int64_t xo_launches = 0;
    // seqNMF's significance test on held-out data (cmf_null_moments; cmf_signif.hip): its scratch (allocated on first use) and the launches
    // of its kernels (cmf_get_counter "signif_launches")
    struct SignifState *signif = nullptr;
    int64_t signif_launches = 0;
    // seqNMF's re-centring of motifs (cmf_mu_set_recentre, cmf_recentre; cmf_recentre.hip): the switch the MU entries read (0: today's path,
    // launch for launch), the tables and scratch of the step (allocated with the first step) and the launches of its kernels
    // (cmf_get_counter "recentre_launches").  wb_hold: the H update in flight is followed by a step, so the write-back hook waits for it
    int mu_recentre = 0;
    struct RecentreState *rc = nullptr;
    int64_t recentre_launches = 0;
    bool wb_hold = false;
};
// The HALS entries under a mask of cmf_mu_set_mask (option "hals_mask"): HALS on the data with its held-out entries imputed by the current
// estimate.  est - imputed data = mask .* (est - data), so both projections are contracted from the masked residual (conv modes 6 / 7 on Xm /
// XmT), whatever "hals_gram" says: its difference forms would read the imputed data itself, which is never formed.
static inline bool hals_masked(const cmf_handle_s *h) { return h->mu_mask && h->hals_mask != 0; }
static inline int hals_gram_form(const cmf_handle_s *h) { return hals_masked(h) ? 0 : h->hals_gram; }
static inline bool xo_active(const cmf_handle_s *h) { return h->xo_lam[0] > 0.0 || h->xo_lam[1] > 0.0 || h->xo_lam[2] > 0.0; }
// the refusals of cmf_mu_install.h asked of this handle: CMF_OK, or the code with its text as the thread's last error
static inline int mu_ask(const cmf_handle_s *h, const MuAsk &q)
{
    const MuFacts f{h->mu_div, h->mu_beta, h->mu_mask, h->kl_mask, h->pq_mask, h->is_div, h->gram, xo_active(h), h->group || h->root_only || h->sharded, h->have_data,
                    h->hals_mask};
    std::string msg;
    const int rc = mu_refusal(f, q, &msg);
    return rc == CMF_OK ? rc : fail(rc, "%s", msg.c_str());
}
// cmf_xortho.hip: frees the tables (destroy_impl); the W side -- lambda xW + lambda_W oW folded into denomW behind numW in h->numden,
// between the C2 contraction and w_apply_impl --; W has been updated and H has not (G stays current); the H side -- numH summed into a
// finished table and the finished denominator table denomH + (lambda xH + lambda_H G), both in the single-slab form of launch_h_update
void xo_free(cmf_handle_s *h);
int xo_fold_w(cmf_handle_s *h);
void xo_after_w(cmf_handle_s *h);
int xo_h_tables(cmf_handle_s *h, int nslabs, size_t stride, int num_pos, int den_pos, const float **num, const float **den);
// cmf_signif.hip: frees the scratch of cmf_null_moments (destroy_impl); the timing pair of cmf_time_kernel ("signif_draw": one batch of null
// draws, per draw; "transconv1_sum": the rule's one-source C3 contraction plus its slab sum)
void signif_free(cmf_handle_s *h);
int signif_time(cmf_handle_s *h, bool draws, int reps, double *avg_ms, double *flops);
// cmf_recentre.hip: frees the tables of the re-centring step (destroy_impl); one step enqueued on the handle's stream (W, H and est pass
// through set_est); cmf_api.hip: an armed write-back forgotten (whoever replaces the factors outside a rule call)
void recentre_free(cmf_handle_s *h);
int recentre_step(cmf_handle_s *h);
void wb_disarm(cmf_handle_s *h);

// cmf_admm.hip: frees a handle's ADMM state (destroy_impl); answers the counters "admm_W_reverts" / "admm_H_reverts" (1 if `name` is one)
void admm_free(cmf_handle_s *h);
int admm_counter(const cmf_handle_s *h, const char *name, int64_t *value);
// cmf_anls.hip: the same for the ANLS state and the counters "anls_W_exchanges" / "anls_H_exchanges" / "anls_backup" / "anls_capped"
void anls_free(cmf_handle_s *h);
int anls_counter(const cmf_handle_s *h, const char *name, int64_t *value);
// cmf_sep.hip: the same for the state of the separable fit and the counter "sep_nnls_exchanges"
void sep_free(cmf_handle_s *h);
int sep_counter(const cmf_handle_s *h, const char *name, int64_t *value);

#define HALS_PMAX 4 // puller workgroups per row of the persistent H pipeline (4 -> 7 measured the same span: profiles/r04_hals_pullers_sweep.txt)

// cmf_group.h -- T-sharded groups behind the C ABI (included by cmf_api.hip).
//
// A *group* is R contiguous column blocks ("shards") of one problem: data / est / H are partitioned along T, W is
// replicated.  The caller holds ONE handle and makes the reference's two calls per iteration
// (update_motifs! / update_feature_maps!, alternating.jl:52,54); the library runs the sharded iteration:
//
//   update_motifs!        per shard: est = conv(W,H) (reused), [numW | denomW] partial sums        (mult.jl:28-34)
//                         ONE all-reduce(sum) of [numW | denomW | tail]   <- the only bulk exchange; the tail carries
//                                                                            the previous loss scalar of every rank
//                         per shard: the identical W update                                        (mult.jl:37-38)
//   update_feature_maps!  per shard: est (new W) on own columns + right lag halo, numH, denomH, H  (mult.jl:44-52)
//                         ONE all-gather of every shard's [first | last] L-1 columns of H (2 x 2.4 KB per shard)
//                         per shard: loss conv, sum((est - data)^2) -> the tail of the next all-reduce (mult.jl:55-57)
//
// Two ways to form a group:
//   cmf_create_multi       one process drives all shards (ndev devices, per-device streams; RCCL communicators from
//                          ncclCommInitAll, collectives inside ncclGroupStart/End) -- what a Julia caller of `fit` gets;
//   cmf_create_shard + cmf_comm_init_rccl / cmf_comm_init_callbacks
//                          one process per shard (torchrun-style launchers; bench.py --gpus N).
// Transports: RCCL over xGMI (the product path), "loopback" (all shards of a cmf_create_multi group on ONE device:
// the collectives are plain kernels -- exercises middle-rank shards on a one-GPU box), and host callbacks (the
// library stages the buffers through pinned host memory and the host performs the collective, e.g. gloo in the tests).
//
// Who enqueues (one-process groups with a stream per shard -- RCCL, peer, loopback-streams): by default one ENQUEUE WORKER
// thread per shard, bound to the shard's device, takes the shard's whole share of an iteration -- its kernels and its
// collective calls -- from a small queue, so the calling thread only posts (and polls the pinned loss words): eight shards
// are enqueued in parallel instead of one after the other.  Each worker calls ncclAllReduce / ncclAllGather on ITS
// communicator from ITS thread, without ncclGroupStart/End: that is RCCL's one-thread-per-device mode, in which no thread
// ever manages two devices -- chosen over "workers meet at a barrier, the caller issues one grouped call" because the
// barrier would put a host round trip back into every collective (two per iteration), which is exactly what the workers
// are there to remove.  Option "enqueue_threads" = 0 (or CMF_ENQUEUE_THREADS=0) restores the single-thread form with
// grouped RCCL calls.  The phases are written once, as lists of per-shard segments and collectives (GroupStep), and run
// either way.
#pragma once
#include <dlfcn.h>
#include <memory>
#include <mutex>
#include "cmf_workers.h"

// The handful of RCCL types this file passes through function pointers, declared here (values as in rccl.h of ROCm 7:
// the NCCL ABI these have had since NCCL 2.0) so that the library builds -- and loads -- on hosts without the RCCL
// development package; RCCL itself is bound with dlopen below.
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;      // non-zero codes are only ever turned into text by ncclGetErrorString
typedef enum { ncclFloat32 = 7 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
}

// ---- RCCL, bound at run time --------------------------------------------------------------------------------------
// librccl is opened with dlopen the first time a communicator is needed: the library then loads on hosts without
// RCCL, and when the process already holds an RCCL (e.g. PyTorch's bundled copy, same SONAME) that copy is reused
// instead of a second one being mapped.
struct RcclApi {
    void *dl = nullptr;
    std::string path;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr; // optional
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr; // optional
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
};
inline RcclApi g_rccl; // (one table for the whole library: C++17 inline variable)

#define RCCLCHK(expr)                                                                                          \
    do {                                                                                                       \
        ncclResult_t r_ = (expr);                                                                              \
        if (r_ != ncclSuccess) return fail(CMF_ERR_COMM, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));   \
    } while (0)

// ---- the group ----------------------------------------------------------------------------------------------------
enum { CMF_TR_LOOPBACK = 0, CMF_TR_RCCL = 1, CMF_TR_CALLBACKS = 2, CMF_TR_PEER = 3 };
enum { CMF_ERR_ECHO = -1000 }; // internal: a worker that gave up because ANOTHER shard's job failed (never crosses the ABI)

// ---- enqueue workers ----------------------------------------------------------------------------------------------
// One thread per local shard of a one-process group (see the file comment); the queue, the meeting point and the abort
// protocol live in cmf_workers.h (free of HIP: stress-tested under ThreadSanitizer on the CPU).
struct cmf_group_s {
    int nranks = 1;
    int transport = CMF_TR_LOOPBACK;
    bool one_process = false;            // cmf_create_multi: all shards are local, H crosses the ABI as the global K x T matrix
    std::vector<cmf_handle_s *> sh;      // local shards
    std::vector<int> rank;               // global rank of each local shard
    std::vector<ncclComm_t> comm;        // RCCL communicators (one per local shard)
    std::vector<ncclComm_t> comm2;       // ... of the communication stream ("lane 1": the overlap form's bulk all-reduce never shares a
                                         // communicator with a collective of the main stream); created when the overlap form is switched on
    cmf_allreduce_fn ar_cb = nullptr;    // host-callback transport
    cmf_allgather_fn ag_cb = nullptr;
    void *cb_user = nullptr;
    float *cb_host = nullptr;            // pinned staging of the callback transport
    size_t cb_host_elems = 0;
    // device buffers, one per local shard
    std::vector<float *> red;            // [LKN2 + tail]: numW | denomW | loss tail  (the shard's numden points here)
    std::vector<float *> halo_send;      // [2 * HC]: own first | last L-1 columns of H
    std::vector<float *> halo_all;       // [nranks * 2 * HC]: every rank's send block (the shard's receive halos point inside)
    std::vector<float *> loss_all;       // [tail]: gathered (hi, lo) loss pairs of the synchronous path
    float *h_tail = nullptr;             // pinned host: 2 ring slots (the late loss read-back: pairs + stamp) + 1 for the synchronous one
    int64_t slot_len = 0;                // floats per slot
    int64_t LKN2 = 0, tail = 0, HC = 0;
    int64_t HHsz = 0;                    // floats of HH = H_unfold H_unfold' ((L*Kpad) x its 128-padded pitch): the Gram form's share
    int gram = 0;                        // option "gram" on a group: the all-reduce carries [numW | HH | tail] instead of [numW | denomW | tail]
    int64_t N = 0, T = 0, K = 0, L = 0;
    std::vector<int64_t> t0, t1;         // column block of every rank
    double data_sumsq = 0.0, data_norm = 0.0;
    bool overlap = false;                // option "allreduce_overlap": numW contracted + all-reduced under the loss conv
    bool num_ready = false;              // overlap form: the numW half belongs to the current H and is reduced (or in flight)
    bool halos_current = false;
    // The halo of H in the tail of the W-phase all-reduce (option "halo_in_allreduce", default on where every shard can: K a multiple of
    // 32, 1 <= L-1 <= 64, the L-1 columns of data in front of every shard resident; the default formulation): no collective between the
    // H update and the loss conv -- ONE collective per iteration.  Every shard with a left neighbour updates the L-1 columns in front
    // of its own itself (h_update_impl, front = true), from an H that is valid 2(L-1) columns out on the left; its own outer columns
    // (last 2(L-1), first L-1) travel in per-rank slots behind the loss tail of the NEXT all-reduce.
    bool halo_opt = true, halo_can = false;
    bool halos_pending = false;          // the H phase has run in that form: the L-1 columns in front are locally valid, everything else of
                                         // the halos is stale until the next all-reduce has brought the slots (halos_current is false meanwhile)
    bool halo_wide = false;              // the left halo is valid 2(L-1) columns out (set by the wide exchanges only)
    int64_t halo_len = 0;                // floats of the slots: nranks * 3 * HC
    std::vector<float *> halo3_send, halo3_all; // the same exchange as an all-gather (set-up, and whenever no all-reduce follows an H phase)
    int64_t n_allreduce = 0, n_allgather = 0;   // collectives built into step lists (cmf_get_counter "allreduce_calls" / "allgather_calls")
    // loopback with one stream PER SHARD (CMF_COMM_LOOPBACK_STREAMS): the collectives keep RCCL's stream semantics -- the
    // operation starts when every shard's stream has reached it and every shard's stream continues when it is done --
    // through events, so a missing dependency between shards cannot hide behind a shared stream (tests on a one-GPU box)
    std::vector<float *> gbuf;           // scratch of group_gather_doubles (one per local shard)
    size_t gbuf_words = 0;
    bool loop_ms = false;
    hipEvent_t ev_in[2][CMF_MAX_LOCAL] = {};  // [main | comm stream][shard]
    hipEvent_t ev_out[2] = {nullptr, nullptr};
    // peer transport: events of the stream fences around its kernels, [lane][before | after the kernel][shard]
    hipEvent_t ev_peer[2][2][CMF_MAX_LOCAL] = {};
    // enqueue workers (empty: the calling thread enqueues every shard itself)
    CmfWorkerPool pool;
    int test_fail_shard = -1;             // test hook CMF_TEST_FAIL_SHARD (group_check_ready)
    int64_t enqueue_ns = 0, enqueue_iters = 0; // cmf_iterate: time the calling thread spent enqueueing / posting, and the iterations it covers
    int force_inline = 0;                // > 0: step lists run on the calling thread although workers exist (GroupInline)
    bool failed = false;                 // a wait for the group ran out (or a collective reported an error): streams and communicators
                                         // may never drain -- destruction aborts the communicators and does not wait for the streams
};


// ---- prototypes of the functions the three translation units share (cmf_api.hip, cmf_rules.hip, cmf_groups.hip) ----
int hals_ensure(cmf_handle_s *h);
void hals_plan(cmf_handle_s *h);
static inline void set_est(cmf_handle_s *h, int kind) // every change of what est holds (and with it: of H, W) passes through here
{
    h->est_kind = kind;
    ++h->est_gen;
}
// ---- the forms of the MU rule: one row each ----
// The single-handle MU path (cmf_api.hip: w_phase_impl, h_update_impl, launch_loss_conv, w_speculate, cmf_masked_loss) reads the active form from
// mu_form(h).  A new form: a row here, its conv modes in mu_launch_conv (cmf_api.hip), and what it needs to be installed in its divergence's row of kMuDivs
// (cmf_mu_install.h: gates, data rule, buffers; mu_refusal there for what it cannot live beside) -- mu_set_form (cmf_api.hip) installs every form from those.
using MuBuf = float *cmf_handle_s::*; // a buffer of the handle
constexpr MuBuf MU_NONE = nullptr, MU_X = &cmf_handle_s::X, MU_XT = &cmf_handle_s::XT, MU_XM = &cmf_handle_s::Xm, MU_XMT = &cmf_handle_s::XmT, MU_M = &cmf_handle_s::M,
                MU_XS = &cmf_handle_s::Xs, MU_XST = &cmf_handle_s::XsT,
                MU_MT = &cmf_handle_s::MT, MU_EST = &cmf_handle_s::est, MU_EST_T = &cmf_handle_s::estT, MU_EST2 = &cmf_handle_s::est2, MU_EST2_T = &cmf_handle_s::est2T;
struct MuForm {
    int store_family, loss_family;  // conv family (cmf_conv_modes.h) of the bases store / store' and of loss / loss + store
    int est_kind;                   // what the storing convs leave in est
    MuBuf data;                     // the data the form fits: raw, or select(mask, data, 0)
    MuBuf conv_data[4];             // data operand per conv base (MU_NONE: launch_conv's default, the raw data in the base's layout)
    int c2_nsrc; MuBuf c2_src[2];   // C2 (update_motifs!): sources contracted with H_shift -> [numW | denomW] (one source: the same buffer named twice)
    int c3_nsrc; MuBuf c3_first;    // C3 (update_feature_maps!): source count and first source; the second (or only) one is estT
    int h_num, h_den;               // positions of numH and denomH among the c3_nsrc slabs of hslabs; h_den < 0, kl_den(): the denominators
                                    // come from the sums of H / W (kl_hsum / kl_den_w / kl_wsum / kl_den_h), not from a contraction
    bool sqrt_update;               // the element-wise updates take the square root of the quotient
    bool square_fusions;            // the few-component fusions (w_update_small_kernel, the H update inside the C3 launch) and the speculated C2 apply
    bool loss_is_mean;              // mu_loss: sum / data_sum (a divergence) instead of sqrt(sum) / norm(data)
    int held_out_family;            // cmf_masked_loss: family of its loss-only conv on the raw data.  KL under its own mask scores by its divergence;
                                    // every other row by squared error under the handle's mask, which may be the PGD entries' (cmf_set_mask)
    bool pow_update = false;        // the element-wise updates raise the quotient to the handle's mu_gamma where that is not 1 (last: the older rows do not name it)
    constexpr bool kl_den() const { return h_den < 0; }
};
enum { MU_SQUARE = 0, MU_SQUARE_MASKED, MU_KL, MU_KL_MASKED, MU_IS, MU_BETA, MU_IS_MASKED, MU_BETA_MASKED, MU_NFORMS };
constexpr MuForm kMuForms[MU_NFORMS] = { // (in the order of the enum)
    {CONV_FAM_PLAIN, CONV_FAM_PLAIN, EST_CONV, MU_X, {MU_NONE, MU_NONE, MU_NONE, MU_NONE},
     2, {MU_X, MU_EST}, 2, MU_XT, 0, 1, false, true, false, CONV_FAM_MU_MASKED},
    {CONV_FAM_MU_MASKED, CONV_FAM_MU_MASKED, EST_MU_MASKED, MU_XM, {MU_NONE, MU_NONE, MU_NONE, MU_NONE},
     2, {MU_XM, MU_EST}, 2, MU_XMT, 0, 1, false, true, false, CONV_FAM_MU_MASKED},
    {CONV_FAM_KL, CONV_FAM_KL, EST_KL_R, MU_X, {MU_NONE, MU_NONE, MU_NONE, MU_NONE},
     1, {MU_EST, MU_EST}, 1, MU_EST_T, 0, -1, false, false, true, CONV_FAM_MU_MASKED},
    // (the KL family's store modes given Xm / Xm' store 0 / e = 0 at the held-out entries: only the loss bases need the masked family;
    //  the denominators are the same contractions on the mask itself, which lands in FRONT of the numerator in hslabs)
    {CONV_FAM_KL, CONV_FAM_KL_MASKED, EST_KL_R_MASKED, MU_XM, {MU_XM, MU_XMT, MU_XM, MU_XM},
     2, {MU_EST, MU_M}, 2, MU_MT, 1, 0, false, false, true, CONV_FAM_KL_MASKED},
    // (P and Q from one conv; C3 contracts (Q', P'): the numerator second)
    {CONV_FAM_IS, CONV_FAM_IS, EST_IS_PQ, MU_X, {MU_NONE, MU_NONE, MU_NONE, MU_NONE},
     2, {MU_EST, MU_EST2}, 2, MU_EST2_T, 1, 0, true, false, true, CONV_FAM_MU_MASKED},
    // (the Itakura-Saito row with the beta family's epilogues and the power step)
    {CONV_FAM_BETA, CONV_FAM_BETA, EST_BETA_PQ, MU_X, {MU_NONE, MU_NONE, MU_NONE, MU_NONE},
     2, {MU_EST, MU_EST2}, 2, MU_EST2_T, 1, 0, false, false, true, CONV_FAM_MU_MASKED, true},
    // (the two rows above under the mask: every base reads the sentinel copy of data, so P and Q come out exactly 0 at the held-out
    //  entries and the contractions on them are the masked sums; cmf_masked_loss scores by the form's own divergence)
    {CONV_FAM_IS_MASKED, CONV_FAM_IS_MASKED, EST_IS_PQ_MASKED, MU_XS, {MU_XS, MU_XST, MU_XS, MU_XS},
     2, {MU_EST, MU_EST2}, 2, MU_EST2_T, 1, 0, true, false, true, CONV_FAM_IS_MASKED},
    {CONV_FAM_BETA_MASKED, CONV_FAM_BETA_MASKED, EST_BETA_PQ_MASKED, MU_XS, {MU_XS, MU_XST, MU_XS, MU_XS},
     2, {MU_EST, MU_EST2}, 2, MU_EST2_T, 1, 0, false, false, true, CONV_FAM_BETA_MASKED, true},
};
// the element-wise step of the active form: 0 the plain quotient, 1 its square root, 2 its power mu_gamma (cmf_mu_step)
static inline int mu_step_kind(const cmf_handle_s *h, const MuForm &f) { return (f.pow_update && h->mu_gamma != 1.f) ? 2 : f.sqrt_update ? 1 : 0; }
static inline const MuForm &mu_form(const cmf_handle_s *h)
{
    return kMuForms[h->mu_div == CMF_DIV_BETA ? (h->mu_mask ? MU_BETA_MASKED : MU_BETA) : h->mu_div == CMF_DIV_IS ? (h->mu_mask ? MU_IS_MASKED : MU_IS) : h->mu_div ? (h->mu_mask ? MU_KL_MASKED : MU_KL) : (h->mu_mask ? MU_SQUARE_MASKED : MU_SQUARE)];
}
// the few-component fusions and the speculated C2 of the active form; never under the penalties of cmf_mu_set_xortho, whose terms enter
// the denominators between the contractions and the element-wise updates
static inline bool mu_fusions(const cmf_handle_s *h) { return mu_form(h).square_fusions && !xo_active(h); }
static inline float *mu_buf(const cmf_handle_s *h, MuBuf b) { return b ? h->*b : nullptr; }
// What the MU entries read for data / "est is current".  reuse_est, the speculated C2 contraction and the deferred loss carry all
// compare against mu_est_kind.
static inline const float *mu_X(const cmf_handle_s *h) { return mu_buf(h, mu_form(h).data); }
static inline int mu_est_kind(const cmf_handle_s *h) { return mu_form(h).est_kind; }
// the loss of the MU entries from the sum its loss conv leaves: norm(est - data) / norm(data), or D(data, est) / sum(data) under KL
// (Itakura-Saito and beta: data_sum holds N * T, the mean divergence per entry)
static inline double mu_loss(const cmf_handle_s *h, double ss)
{
    const MuForm &f = mu_form(h);
    return f.loss_is_mean ? ss / h->data_sum : std::sqrt(ss) / (f.data == MU_XM ? h->xm_norm : h->data_norm);
}
int wb_after_H(cmf_handle_s *h); // hook: the kernels that make H final have been enqueued (cmf_writeback.h)
int gram_ensure(cmf_handle_s *h);
int hals_w_impl(cmf_handle_s *h, double l1W, double l2W);
int hals_w_speculate(cmf_handle_s *h);
int resid_and_loss(cmf_handle_s *h, double *sumsq, bool masked = false, bool loss_abs = false, const float *data = nullptr); // (data == NULL: the handle's raw data)
int hals_resid_and_loss(cmf_handle_s *h, double *sumsq);
int gram_w_impl(cmf_handle_s *h, double l1W, double l2W);
int gram_w_partial(cmf_handle_s *h, float *hh_out);
int gram_w_finish(cmf_handle_s *h, const float *HH, double l1W, double l2W, const float *tail_src = nullptr, float *tail_dst = nullptr,
                         int tail_n = 0);
int gram_h_update(cmf_handle_s *h, double l1H, double l2H);
int gram_h_impl(cmf_handle_s *h, double l1H, double l2H, double *loss);
// the PGD phases over a set of shards: the shards of g, or (g == NULL) the lone handle st
int pgd_w_phase(cmf_handle_s *st, struct cmf_group_s *g, double pen_sq, double pen_abs, int nonneg);
int pgd_h_phase(cmf_handle_s *st, struct cmf_group_s *g, double pen_sq, double pen_abs, int nonneg, double *loss);
int hals_h_impl(cmf_handle_s *h, double l1H, double l2H);
int hals_h_rerun(cmf_handle_s *h);
int gram_denom_h(cmf_handle_s *h, float *out);
int gram_tables(cmf_handle_s *h);
int group_pgd_prepare(cmf_handle_s *st, struct cmf_group_s *g);
int group_sum_doubles(struct cmf_group_s *g, const std::vector<double *> &ptr, int n, std::vector<double> *host_out = nullptr);
int group_exchange_halos(struct cmf_group_s *g);
size_t n_partial(const cmf_handle_s *h);
hipError_t stream_acquire(int device, hipStream_t *s);
void plan(cmf_handle_s *h, int n_cu);
int upload_cols(cmf_handle_s *h, const double *src, int64_t tc, int64_t ncols, bool rows_layout, bool accumulate_sumsq,
                       float *rows_dst = nullptr, float *cols_dst = nullptr);
int create_impl(cmf_handle *out, int device, int64_t N, int64_t Tl, int64_t K, int64_t L,
                       const double *data, int64_t t_offset, int64_t T_global, bool sharded, long long n_cu_asked = kNoCuHook);
int launch_hxt_on(cmf_handle_s *h, const float *X0, const float *X1, int NpX, int nsrc, float *slabs, int nchunks, int chunk_len,
                         int main_rows = -1, const float *left = nullptr);
int launch_transconv(cmf_handle_s *h, int nsrc, const float *xt0 = nullptr, bool front_block = false);
int launch_slab_sum(cmf_handle_s *h, float *out, const float *in, int nslabs, size_t stride, bool take_carry = false,
                           CmfHxtTail tail = CmfHxtTail{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0});
// left / leftT (NULL: H / Ht of the handle): the left operand of the contraction in the layouts of H and Ht -- an H-shaped table whose padding
// rows and columns k >= K are exact zeros (the penalty contraction of cmf_mu_set_xortho puts G = off(S(H)) there)
int hxt_contract(cmf_handle_s *h, const float *X0, const float *X1, int nsrc, float *out, bool take_carry = false, bool slabs_only = false,
                 const float *left = nullptr, const float *leftT = nullptr);
int hxt_contract_small(cmf_handle_s *h, const float *X0, const float *X1, int nsrc, float *out, bool take_carry, bool slabs_only,
                       const float *leftT = nullptr); // cmf_small.hip
bool sk_can_fuse_h(const cmf_handle_s *h); // cmf_small.hip
int launch_transconv_small(cmf_handle_s *h, int nsrc, const float *xt0, bool update_h = false, float l1 = 0.f, float two_l2 = 0.f);                                                          // cmf_small.hip
int read_scalar(cmf_handle_s *h, int slot, double *v);
int w_partial_impl(cmf_handle_s *h);
int w_partial_half_impl(cmf_handle_s *h, int den);
int w_apply_impl(cmf_handle_s *h, double l1W, double l2W, const float *tail_src = nullptr, float *tail_dst = nullptr, int tail_n = 0,
                        const float *den = nullptr);
int h_update_impl(cmf_handle_s *h, double l1H, double l2H, bool front = false);
int launch_loss_conv(cmf_handle_s *h);
int loss_partial_impl(cmf_handle_s *h, double *sumsq, bool readback = true, double *host_out = nullptr, bool speculate = false);
int set_factors_impl(cmf_handle_s *h, const double *W, const double *H);
int get_factors_impl(cmf_handle_s *h, double *W, double *H);
int reduce_partials(cmf_handle_s *h, const double *partial, int n, int slot, double *v);
double wait_timeout_s();
int ensure_resid(cmf_handle_s *h, bool masked = false, bool loss_abs = false);
HalsRowParams hals_row_params(cmf_handle_s *h, double l1H, double l2H);
int hals_persist_launch(cmf_handle_s *h, const HalsRowParams &q, int debug = 0, bool clear_flags = true);
int rccl_load();
int group_use(cmf_handle_s *s);
int group_join(cmf_group_s *g);
int group_start_workers(cmf_group_s *g);
int group_allreduce(cmf_group_s *g, const std::vector<float *> &bufs, size_t off, size_t count, int lane = 0);
int group_allgather(cmf_group_s *g, const std::vector<float *> &send, const std::vector<float *> &recv, size_t count);
int group_gather_doubles(cmf_group_s *g, const std::vector<double> &vals, std::vector<double> &out, int n = 1);
int group_check_ready(cmf_group_s *g);
int group_sync(cmf_group_s *g);
int group_update_motifs(cmf_group_s *g, double l1W, double l2W);
int group_update_feature_maps(cmf_group_s *g, double l1H, double l2H, double *sumsq);
int group_compute_loss(cmf_group_s *g, double *loss);
int group_iterate(cmf_group_s *g, int64_t n, int eval_mode, double l1W, double l2W, double l1H, double l2H,
                         double *losses, double *stamps);
int group_set_factors(cmf_group_s *g, const double *W, const double *H);
int group_get_factors(cmf_group_s *g, double *W, double *H);
bool group_destroy(cmf_group_s *g);
int group_ensure_lane1(cmf_group_s *g, const void *id128 = nullptr);

// small helpers
static inline size_t group_tail_off(const cmf_group_s *g) { return (size_t)(g->gram ? g->LKN2 / 2 + g->HHsz : g->LKN2); }
static size_t group_stop_workers(cmf_group_s *g) { return cmf_pool_stop(g->pool, g->failed); }

// The entries that are not on the MU hot path (PGD, masks, stand-alone timings, ...) enqueue from the calling thread as they
// always did: inside this scope the workers are idle and every step list runs in line.  g == NULL (a lone handle): nothing to hold.
struct GroupInline {
    cmf_group_s *g;
    int rc;
    explicit GroupInline(cmf_group_s *g_) : g(g_), rc(g_ ? group_join(g_) : CMF_OK) { if (g) ++g->force_inline; }
    ~GroupInline() { if (g) --g->force_inline; }
};

template <typename T>
static int dalloc_zero(T **p, size_t n)
{
    HIPCHK(hipMalloc(p, n * sizeof(T)));
    HIPCHK(hipMemset(*p, 0, n * sizeof(T)));
    // hipMemset of device memory runs on the null stream and may return before it has finished; the handle's work runs on
    // non-blocking streams, which the null stream does not order -- a lagging fill would wipe what they wrote meanwhile
    HIPCHK(hipStreamSynchronize(nullptr));
    return CMF_OK;
}

// the C2 kernel adds CG consecutive time chunks inside a workgroup: it writes nchunks / CG slabs
static int hxt_cg(int nchunks) { return nchunks % 4 == 0 ? 4 : (nchunks % 2 == 0 ? 2 : 1); }
static int hxt_nslabs(int nchunks) { return nchunks / hxt_cg(nchunks); }

static const int kHxtLP[] = {1, 2, 3, 4, 5, 6, 8}; // 2*LP*16 accumulator registers must fit the 256 AGPRs

// kernel classes of the "profile" option
enum { PROF_CONV = 0, PROF_CONV_T, PROF_CONV_LOSS, PROF_CONV_LOSS_STORE, PROF_HXT, PROF_TRANSCONV, PROF_HXT_NUM, PROF_HXT_DEN, PROF_OTHER,
       PROF_HALS_PIPE, PROF_HALS_WSWEEP,
       // the contraction launches of the HALS / PGD / Gram rules (one source, or on the stored residual)
       PROF_CONV_RESID, PROF_HXT_RESID, PROF_HXT_HH, PROF_TRANSCONV_1, PROF_GRAM_DENOM_H, PROF_GRAM_TABLES, PROF_GRAM_W, PROF_NCLS };
static const char *kProfNames[PROF_NCLS] = {"conv", "conv_t", "conv_loss", "conv_loss_store", "hxt", "transconv", "hxt_num", "hxt_den", "other",
                                            "hals_h_pipeline", "hals_w_sweep",
                                            "conv_resid", "hxt_resid", "hxt_hh", "transconv_1src", "gram_denom_h", "gram_tables", "gram_w"};
static_assert(PROF_NCLS <= 32, "cmf_handle_s::prof_seen holds 32 classes");

// the "profile" class of a C2 launch, from what it contracts: data (and est) of the MU rule, est of the active form alone (a
// denominator), a stored residual, the HALS rule's HX
static inline int hxt_prof_class(const cmf_handle_s *h, const float *X0, int nsrc)
{
    const bool x0_data = X0 == mu_X(h);
    return (nsrc == 2 && x0_data) ? PROF_HXT : (nsrc == 1 && x0_data) ? PROF_HXT_NUM : (nsrc == 1 && X0 == h->est && h->est_kind == mu_est_kind(h)) ? PROF_HXT_DEN
           : (nsrc == 1 && X0 == h->est) ? PROF_HXT_RESID : (X0 == h->hals_HX && h->hals_HX) ? PROF_HXT_HH : PROF_OTHER;
}

struct ProfScope {
    cmf_handle_s *h;
    hipEvent_t b = nullptr;
    ProfScope(cmf_handle_s *h_, int cls) : h(h_)
    {
        if (!h->prof || h->prof_recs.size() >= 8192) return;
        if (h->prof_mask && !(((unsigned)h->prof_mask >> cls) & 1u)) return;
        if ((h->prof_seen[cls]++ % h->prof_every) != 0) return;
        hipEvent_t ev[2] = {nullptr, nullptr};
        for (int q = 0; q < 2; ++q) {
            if (!h->prof_pool.empty()) { ev[q] = h->prof_pool.back(); h->prof_pool.pop_back(); }
            else if (hipEventCreate(&ev[q]) != hipSuccess) { if (q == 1) h->prof_pool.push_back(ev[0]); return; }
        }
        (void)hipEventRecord(ev[0], h->stream);
        h->prof_recs.push_back({ev[0], ev[1], cls});
        b = ev[1];
    }
    ~ProfScope() { if (b) (void)hipEventRecord(b, h->stream); }
};

// The tiles at the end of the one-wave conv grid (conv3_kernel, conv3_chase_kernel) are cut into one-wave pieces: the remainder of the
// last round when it is thin, and, from kConvSplitMinRounds rounds on, kConvSplitExtraPerCu tiles per CU more -- after several rounds
// of dynamic dispatch the waves of a SIMD are out of step and the launch ends in a ragged drain one tile long; small pieces at the end
// of the queue fill it (config 2, 8.1 rounds: -1.5 % in every mode; below 4 rounds it costs +1-4 %: profiles/r02*_conv_split*).
constexpr int kConvWaveSlotsPerCu = 12;  // one-wave workgroups resident on a CU
constexpr int kConvThinTilesPerCu = 3;   // a remainder of at most this many tiles per CU is cut; a larger one is left as whole tiles
constexpr int kConvSplitMinRounds = 4, kConvSplitExtraPerCu = 3;
struct ConvTailCut { int cut, n_full, pieces; }; // tiles cut | whole tiles in front | pieces per cut tile: 4, or 16 below one cut tile per CU
static inline ConvTailCut conv_tail_cut(const cmf_handle_s *h, int tiles, int n_cu)
{
    const int slots = kConvWaveSlotsPerCu * n_cu, rem = tiles % slots;
    int cut = 0;
    if (h->conv_split) {
        if (rem > 0 && rem <= kConvThinTilesPerCu * n_cu) cut = rem;
        if (tiles / slots >= kConvSplitMinRounds) cut += kConvSplitExtraPerCu * n_cu;
        cut = std::min(cut, tiles);
    }
    return {cut, tiles - cut, (cut > 0 && cut < n_cu && h->conv_split != 4) ? 16 : 4};
}

// data == NULL: the handle's data in the layout the mode reads (the masked rules pass Xm / XmT, cmf_masked_loss the raw data)
// loss_abs: ConvParams::loss_abs of the modes that read it -- the residual modes' loss kind (1 = AbsoluteLoss), the masked loss-only
// modes' complement (1 = the sum runs over mask == 0)
template <int MODE>
static int launch_conv(cmf_handle_s *h, float *out, int T_store, int gy, const float *data = nullptr, int loss_abs = 0)
{
    ProfScope prof_(h, conv_pgd(MODE) ? PROF_CONV_RESID : conv_base(MODE) == CONV_BASE_STORE ? PROF_CONV : conv_base(MODE) == CONV_BASE_STORE_T ? PROF_CONV_T
                       : conv_base(MODE) == CONV_BASE_LOSS ? PROF_CONV_LOSS : PROF_CONV_LOSS_STORE);
    const CmfDims &d = h->d;
    if ((conv_mu_masked(MODE) || conv_kl_masked(MODE) || conv_pq_masked(MODE)) && !(h->M && h->MT)) return fail(CMF_ERR_STATE, "internal: a masked conv without a mask");
    ConvParams p;
    if (conv_pq(MODE) && !(h->est2 && h->est2T)) return fail(CMF_ERR_STATE, "internal: an Itakura-Saito or beta conv without its second pair of buffers");
    p.Ht = h->Ht; p.Wt = h->Wt; p.out = out; p.data = data ? data : (conv_data_transposed(MODE) ? h->XT : h->X); p.partial = h->partial;
    p.out2 = !conv_pq(MODE) ? nullptr : conv_transposed(MODE) ? h->est2T : h->est2; // (Q; out takes P)
    if (conv_beta(MODE)) {
        const float *c = h->beta_consts;
        p.beta_m1 = c[0]; p.beta_m2 = c[1]; p.beta = c[2]; p.beta_inv = c[3]; p.beta_inv_bb = c[4];
        for (int k = 0; k < 6; ++k) p.beta_c[k] = c[5 + k];
    }
    p.mask = conv_mask_transposed(MODE) ? h->MT : h->M;
    p.Np = d.Np; p.TP = d.TP; p.PADL = d.PADL; p.K = d.K; p.KB = d.KB; p.L = d.L; p.T_store = T_store;
    p.N = d.N; // (n blocks that are all padding are skipped)
    p.loss_abs = (conv_loss_abs_is_absolute_loss(MODE) || conv_loss_abs_is_complement(MODE)) ? loss_abs : 0;
    dim3 grid(h->conv_gx, gy), block(256);
    const int gx3 = d.Np / 64, tiles3 = gx3 * ((T_store + 63) / 64);
    if (h->small_k) { // few components: one-wave tiles over the ceil(K/2) live k pairs per lag (conv_small_kernel)
        const int nkp = (d.K + 1) / 2;
        // the tiles beyond whole rounds of one tile per SIMD slot-triple (3 per SIMD) go out as quarter pieces at the end of the
        // grid, when they are few (at most one tile per SIMD: otherwise whole tiles balance well enough)
        const int per_round = 4 * h->n_cu;                          // one tile per SIMD
        const int remq = tiles3 % per_round;
        int cutq = (h->conv_split && tiles3 >= per_round && remq > 0 && remq <= per_round / 4) ? remq : 0;
        if (h->conv_split && tiles3 < per_round) cutq = tiles3; // fewer tiles than SIMDs (short recordings): quarter pieces only (configs[0]: 9-12 -> 5-8 us)
        const int n_full = tiles3 - cutq;
        grid = dim3(n_full + 4 * cutq);
        // (loss + store on a short launch: the data tile is requested before the MFMA loop, conv3_tile)
        const bool pre = conv_has_pre(MODE) && nkp <= 4 && tiles3 <= 4 * per_round;
#define CASE(NKP_) do { if (pre) hipLaunchKernelGGL((conv_small_kernel<MODE, NKP_, (conv_has_pre(MODE) && NKP_ <= 4)>), grid, dim3(64), 0, h->stream, p, gx3, n_full); \
                        else hipLaunchKernelGGL((conv_small_kernel<MODE, NKP_>), grid, dim3(64), 0, h->stream, p, gx3, n_full); } while (0)
        if (nkp <= 1) CASE(1); else if (nkp == 2) CASE(2); else if (nkp == 3) CASE(3); else if (nkp == 4) CASE(4);
        else if (nkp <= 6) CASE(6); else CASE(8);
#undef CASE
        h->launches[LA_CONV_SMALL + (nkp <= 4 ? std::max(nkp, 1) - 1 : nkp <= 6 ? 4 : 5)] += 1;
        if (cutq > 0) h->launches[LA_CONV_SMALL_Q] += 1;
        if (pre) h->launches[LA_CONV_SMALL_PRE] += 1;
        if (n_full > 0) h->launches[LA_CONV_SMALL_WHOLE] += 1; // (whole tiles in front of the quarter pieces, or alone)
        h->conv_partials = (int)grid.x;
        KCHK("conv_small_kernel");
        return CMF_OK;
    }
    // measured at config 2 (tools/time_kernels.py): the one-wave kernel wins for the epilogues that read data (0.924 vs 0.931 ms loss
    // only, 0.936 vs 0.943 ms loss + store), the 128 x 128 tiles for the store-only ones (0.911 vs 0.932 ms est, 0.910 vs 0.924 ms est').
    // A cut tail (short shards: 3136 tiles on 3072 slots at T/8) decides for the one-wave kernel in every mode, and so does a mode
    // without 128 x 128 tiles (conv_on_tiles128), whatever option "conv_kernel" says: the one-wave kernel won those modes anyway.
    const ConvTailCut tc = conv_tail_cut(h, tiles3, h->n_cu);
    const int variant = (h->conv_variant && conv_on_tiles128(MODE)) ? h->conv_variant : ((conv_reads_tile(MODE) || tc.cut > 0) ? 3 : 2);
    if (d.K % 32 == 0 && variant == 3) {
        grid = dim3(tc.n_full + tc.pieces * tc.cut);
        hipLaunchKernelGGL((conv3_kernel<MODE>), grid, dim3(64), 0, h->stream, p, gx3, tc.n_full, tc.pieces);
        h->launches[tc.cut == 0 ? LA_CONV3_WHOLE : tc.n_full > 0 ? (tc.pieces == 4 ? LA_CONV3_WHOLE_P4 : LA_CONV3_WHOLE_P16)
                                                 : (tc.pieces == 4 ? LA_CONV3_P4 : LA_CONV3_P16)] += 1;
    } else if (d.K % 32 == 0) {
        if constexpr (conv_on_tiles128(MODE)) hipLaunchKernelGGL((conv2_kernel<MODE>), grid, block, 0, h->stream, p);
        if constexpr (conv_on_tiles128(MODE)) h->launches[LA_CONV2] += 1;
    } else {
        hipLaunchKernelGGL((conv_kernel<MODE, 0>), grid, block, 0, h->stream, p);
        h->launches[LA_CONV] += 1;
    }
    h->conv_partials = (int)(grid.x * grid.y);
    KCHK("conv_kernel");
    return CMF_OK;
}

// The one-wave conv tiles of tile rows [row0, row0 + nrows) on h->stream (conv3_chase_kernel; K a multiple of 32): the tail of the
// grid is cut into pieces for a chip of n_cu CUs like launch_conv does.  gate != NULL: every tile waits for *gate >= its row + 1 (the
// HALS row pipeline's last progress flag) and reads H with agent-scope loads.  Loss partials pidx0 ... pidx0 + *npartials - 1.
// data == NULL: the handle's raw data in the layout the mode reads (the masked residual of the HALS rule passes Xm); the mask is the handle's.
template <int MODE>
static int launch_conv_rows(cmf_handle_s *h, float *out, int row0, int nrows, int pidx0, int n_cu, const int *gate, int *abort_word,
                            int *host_status, int *npartials, int T_store = -1, const float *data = nullptr)
{
    ProfScope prof_(h, MODE == CONV_EST_T ? PROF_CONV_T : MODE == CONV_LOSS_EST ? PROF_CONV_LOSS_STORE : PROF_CONV_RESID);
    const CmfDims &d = h->d;
    ConvParams p;
    if (conv_reads_mask(MODE) && !h->M) return fail(CMF_ERR_STATE, "internal: a masked conv without a mask");
    p.Ht = h->Ht; p.Wt = h->Wt; p.out = out; p.data = data ? data : (conv_data_transposed(MODE) ? h->XT : h->X); p.partial = h->partial; p.mask = h->M;
    p.out2 = nullptr;
    p.Np = d.Np; p.TP = d.TP; p.PADL = d.PADL; p.K = d.K; p.KB = d.KB; p.L = d.L; p.T_store = T_store >= 0 ? T_store : d.Tl;
    p.N = d.N;
    p.loss_abs = 0;
    const int gx3 = d.Np / 64;
    const ConvTailCut tc = conv_tail_cut(h, gx3 * nrows, n_cu);
    const int grid = tc.n_full + tc.pieces * tc.cut;
    if (conv_writes_loss(MODE) && (size_t)(pidx0 + grid) > n_partial(h)) return fail(CMF_ERR_STATE, "internal: loss partial buffer too small for a split conv");
    if (gate) hipLaunchKernelGGL((conv3_chase_kernel<MODE, true>), dim3(grid), dim3(64), 0, h->stream, p, gx3, tc.n_full, tc.pieces, row0, pidx0, gate, abort_word, host_status);
    else hipLaunchKernelGGL((conv3_chase_kernel<MODE, false>), dim3(grid), dim3(64), 0, h->stream, p, gx3, tc.n_full, tc.pieces, row0, pidx0, gate, abort_word, host_status);
    KCHK("conv3_chase_kernel");
    *npartials = grid;
    return CMF_OK;
}

inline std::atomic<int64_t> g_liveness_checks{0}; // stream queries / health checks made by waits for a loss (process-wide; cmf_get_counter "liveness_checks")

template <typename U>
static int wait_words(hipStream_t stream, const volatile U *p, int n, U sentinel, const std::function<int()> *health = nullptr,
                      const std::function<bool()> *enqueued = nullptr)
{
    auto all_there = [&]() {
        for (int j = 0; j < n; ++j)
            if (p[j] == sentinel) return false;
        return true;
    };
    // The liveness checks below are made after 50 ms of waiting and every 50 ms from then on, not every few thousand polls:
    // hipStreamQuery makes the runtime put a marker packet (a barrier with a system-scope release) into the stream when the last
    // command carries no signal, and the device paid for it -- 5.9 us between the loss conv and the next iteration's first
    // contraction, every iteration whose loss took longer than the first 4096 polls (profiles/r06_stream_query_gap.txt).
    const auto t_begin = std::chrono::steady_clock::now();
    auto next_check = t_begin + std::chrono::milliseconds(50);
    for (unsigned spins = 1;; ++spins) {
        if (all_there()) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return CMF_OK;
        }
        if ((spins & 0x3FF) == 0 && std::chrono::steady_clock::now() >= next_check) {
            // (enqueue workers that are still posting leave the stream idle: only a stream that has been given all its work
            // and has drained it proves that the words will never come)
            g_liveness_checks.fetch_add(1, std::memory_order_relaxed);
            const hipError_t e = (enqueued && !(*enqueued)()) ? hipErrorNotReady : hipStreamQuery(stream);
            if (e == hipSuccess) { // everything enqueued has run: the words must be there now
                if (all_there()) return CMF_OK;
                return fail(CMF_ERR_HIP, "the stream drained without posting the loss");
            }
            if (e != hipErrorNotReady) return fail(CMF_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(e));
            if (health) CMFTRY((*health)());
            next_check = std::chrono::steady_clock::now() + std::chrono::milliseconds(50);
            if (std::chrono::duration<double>(next_check - t_begin).count() > wait_timeout_s())
                return fail(health ? CMF_ERR_COMM : CMF_ERR_HIP, "no loss arrived within %.0f s (CMF_WAIT_TIMEOUT_S): %s", wait_timeout_s(),
                            health ? "a collective of the group did not complete -- is every rank / device of the group still running?"
                                   : "the device did not finish the iteration");
        }
        __builtin_ia32_pause();
    }
}

// HIP timing events behind the iterations of a pipelined batch (cmf_fit's time_hist): begin() records the start, mark(it) goes
// behind iteration it's loss conv, finish() turns them into seconds since the start.  Inactive unless begin() was called.
struct DevStamps {
    std::vector<hipEvent_t> ev;
    bool active = false;
    int begin(hipStream_t st, int64_t n)
    {
        if (n < 1 || n > 8192) return CMF_OK; // (a batch that long keeps the host stamps)
        ev.assign((size_t)n + 1, nullptr);
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(ev[0], st));
        active = true;
        return CMF_OK;
    }
    int mark(hipStream_t st, int64_t it)
    {
        if (active) HIPCHK(hipEventRecord(ev[(size_t)it + 1], st));
        return CMF_OK;
    }
    int finish(double *stamps, int64_t n)
    {
        if (!active) return CMF_OK;
        HIPCHK(hipEventSynchronize(ev[(size_t)n]));
        for (int64_t it = 0; it < n; ++it) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[(size_t)it + 1]));
            stamps[it] = 1e-3 * (double)ms;
        }
        return CMF_OK;
    }
    ~DevStamps()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

