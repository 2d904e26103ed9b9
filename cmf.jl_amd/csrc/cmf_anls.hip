// cmf_anls.hip -- the ANLS rule (src/algs/anls.jl) on one device, in fp64 end to end: cmf_anls_prepare, cmf_anls_update_motifs,
// cmf_anls_update_feature_maps (include/cmf_hip.h).  The kernels are in cmf_anls.h, the contraction and the part of the state
// that the ADMM rule has too in cmf_fp64.h; the Gram form of the two steps and what is assumed about the reference's NNLS
// package are in DESIGN.md, "The ANLS rule".
#include "cmf_internal.h"
#include "cmf_anls.h"
#include "cmf_nnls_large.h"

using namespace fp64;
using namespace anls;

static const char RULE[] = "ANLS";
constexpr double ANLS_TOL = 1e-5; // NNLS_TOL, anls.jl:18

struct AnlsState : Fp64State { // Hd: [k][t] in the W call (the stacked loaders), Julia's [t][k] in the H call
    double *G = nullptr, *C = nullptr, *X = nullptr; // W step: LK x LK, LK x N [i][n] twice
    double *Bt = nullptr;               // H step: transconv(W, data) as [t][k]
    double *Alag = nullptr;             // L x (2L-1) x K x K (anls_lag_gram_kernel)
    unsigned long long *st = nullptr;   // ST_N counters of the running call
    LargeScratch large;                 // the slabs of nnls_large_kernel (option "nnls_large"), made by the first call that needs them
    struct Host { unsigned long long st[ST_N]; double sum; } *host = nullptr; // pinned
    int64_t w_exchanges = 0, h_exchanges = 0, backup = 0, capped = 0; // of the last call (exchanges: of the last call of each kind)
};

void anls_free(cmf_handle_s *h)
{
    if (!h || !h->anls) return;
    fp64_release(h, h->anls);
    large_release(&h->anls->large);
    if (h->anls->host) (void)hipHostFree(h->anls->host);
    delete h->anls;
    h->anls = nullptr;
}

int anls_counter(const cmf_handle_s *h, const char *name, int64_t *value)
{
    const AnlsState *s = h->anls;
    if (std::strcmp(name, "anls_W_exchanges") == 0) { *value = s ? s->w_exchanges : 0; return 1; }
    if (std::strcmp(name, "anls_H_exchanges") == 0) { *value = s ? s->h_exchanges : 0; return 1; }
    if (std::strcmp(name, "anls_backup") == 0) { *value = s ? s->backup : 0; return 1; }
    if (std::strcmp(name, "anls_capped") == 0) { *value = s ? s->capped : 0; return 1; }
    return 0;
}

static int anls_state(cmf_handle h, AnlsState **out)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    CMFTRY(fp64_single_gpu(h, RULE, false));
    if (!h->anls) return fail(CMF_ERR_STATE, "call cmf_anls_prepare before the ANLS rule entries");
    *out = h->anls;
    HIPCHK(hipSetDevice(h->device));
    return CMF_OK;
}

int cmf_anls_prepare(cmf_handle h, const double *data)
{
    if (!h || !data) return fail(CMF_ERR_ARG, "NULL argument");
    CMFTRY(fp64_single_gpu(h, RULE, true));
    const int64_t N = h->d.N, T = h->d.Tl, K = h->d.K, L = h->d.L;
    if (T > (int64_t)65535 * TP) return fail(CMF_ERR_UNSUPPORTED, "ANLS: T = %lld > %lld", (long long)T, (long long)65535 * TP);
    if (L > (1 << 20) || K > (1 << 20)) return fail(CMF_ERR_UNSUPPORTED, "ANLS: K = %lld, L = %lld", (long long)K, (long long)L);
    HIPCHK(hipSetDevice(h->device));
    anls_free(h);
    auto *s = new AnlsState();
    h->anls = s;
    auto bail = [&](int rc) { anls_free(h); return rc; };
    int rc = fp64_prepare_common(h, s, data);
    // the entries refuse what is beyond; the state of the other one is still made.  (WMAX < K*L <= WLARGE: option "nnls_large" is set
    // after the rule is made, so update_motifs! makes G, C, X when it first runs there.)
    const bool w_ok = s->LK <= WMAX, h_ok = K <= KMAX;
    if (rc == CMF_OK && w_ok) rc = fp64_alloc(s, &s->G, (size_t)s->LK * s->LK);
    if (rc == CMF_OK && w_ok) rc = fp64_alloc(s, &s->C, (size_t)s->LK * N);
    if (rc == CMF_OK && w_ok) rc = fp64_alloc(s, &s->X, (size_t)s->LK * N);
    if (rc == CMF_OK && h_ok) rc = fp64_alloc(s, &s->Bt, (size_t)K * T);
    if (rc == CMF_OK && h_ok) rc = fp64_alloc(s, &s->Alag, (size_t)L * (2 * L - 1) * K * K);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->st, ST_N);
    if (rc != CMF_OK) return bail(rc);
    if (hipHostMalloc(&s->host, sizeof(AnlsState::Host)) != hipSuccess) return bail(fail(CMF_ERR_HIP, "hipHostMalloc failed"));
    return CMF_OK;
}

// the counters of the call that has just been enqueued; an irregular end of any problem fails the call
static int finish(AnlsState *s, hipStream_t st, const char *what, int64_t *exchanges)
{
    HIPCHK(hipMemcpyAsync(s->host->st, s->st, sizeof(s->host->st), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *exchanges = (int64_t)s->host->st[ST_ROUNDS];
    s->backup = (int64_t)s->host->st[ST_BACKUP];
    s->capped = (int64_t)s->host->st[ST_CAPPED];
    if (s->host->st[ST_BADPIVOT])
        return fail(CMF_ERR_UNSUPPORTED, "ANLS %s: the Gram of a passive set is not positive definite in %llu problem(s) (rank-deficient or non-finite input); "
                                         "the factor is left as it was", what, s->host->st[ST_BADPIVOT]);
    if (s->capped)
        return fail(CMF_ERR_UNSUPPORTED, "ANLS %s: %lld problem(s) hit the cap on pivoting rounds (counter anls_capped); the factor is left as it was", what,
                    (long long)s->capped);
    return CMF_OK;
}

int cmf_anls_update_motifs(cmf_handle h, const double *H, double *W)
{
    AnlsState *s = nullptr;
    CMFTRY(anls_state(h, &s));
    if (!H || !W) return fail(CMF_ERR_ARG, "NULL argument");
    const int64_t N = s->N, T = s->T, K = s->K, L = s->L, LK = s->LK;
    const bool large = LK > WMAX && h->nnls_large;
    if (LK > WMAX && !large)
        return fail(CMF_ERR_UNSUPPORTED, "ANLS: update_motifs! solves K*L <= %d unknowns per unit in LDS (K*L = %lld)", WMAX, (long long)LK);
    if (LK > WLARGE)
        return fail(CMF_ERR_UNSUPPORTED, "ANLS: update_motifs! solves K*L <= %d unknowns per unit (option \"nnls_large\"; K*L = %lld)", WLARGE, (long long)LK);
    hipStream_t st = h->stream;
    if (!s->G) { // (only where cmf_anls_prepare left them out: K*L > WMAX)
        CMFTRY(fp64_alloc(s, &s->G, (size_t)LK * LK));
        CMFTRY(fp64_alloc(s, &s->C, (size_t)LK * N));
        CMFTRY(fp64_alloc(s, &s->X, (size_t)LK * N));
    }
    std::vector<double> Hr;
    CMFTRY(fp64_upload_H_rows(s, st, H, Hr));
    HIPCHK(hipMemsetAsync(s->st, 0, ST_N * sizeof(unsigned long long), st));
    // G = Hstk*Hstk', C = Hstk*data' (anls.jl:49-52: t(H_unfold), t(data) as the solver's normal equations)
    const HstkRT hs{s->Hd, (int)K, (int)T};
    const HstkTR hst{s->Hd, (int)K, (int)T};
    CMFTRY((fp64_gemm<false, false>(s, st, RULE, hs, hst, EpiStore{s->G, LK, 0.0}, LK, LK, T, false)));
    CMFTRY((fp64_gemm<false, true>(s, st, RULE, hs, RowMajor{s->data, N}, EpiStore{s->C, N, 0.0}, LK, N, T, false)));
    const int bo = h->anls_backup_only;
    if (large) {
        CMFTRY(nnls_large(&s->large, st, RULE, s->G, s->C, s->X, (int)LK, N, ANLS_TOL, bo, s->st));
    } else {
        hipLaunchKernelGGL(anls_nnls_w_kernel, dim3((unsigned)N), dim3(256), 0, st, s->G, s->C, s->X, (int)LK, N, ANLS_TOL, anls_round_cap((int)LK, bo), bo, s->st);
        KCHK("anls_nnls_w_kernel");
    }
    std::vector<double> Xh((size_t)LK * N);
    HIPCHK(hipMemcpyAsync(Xh.data(), s->X, Xh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    CMFTRY(finish(s, st, "update_motifs!", &s->w_exchanges));
    fp64_fold_W(Xh.data(), W, K, N, L);
    return CMF_OK;
}

static int sweep(cmf_handle h, AnlsState *s, int64_t t0, int64_t t1)
{
    const int64_t K = s->K, L = s->L;
    const size_t ring = (size_t)(L - 1) * K * sizeof(double), full = (size_t)(2 * L - 1) * K * K * sizeof(double);
    const int a_lds = full <= 32768;
    const size_t dyn = ring + (a_lds ? full : 0);
    static std::mutex mu; // (the attribute belongs to the kernel, not to a launch)
    {
        std::lock_guard<std::mutex> g(mu);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(anls_h_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(49152 + 32768)));
    }
    const int bo = h->anls_backup_only;
    hipLaunchKernelGGL(anls_h_sweep_kernel, dim3(1), dim3(64), dyn, h->stream, s->Alag, s->Bt, s->Hd, (int)K, (int)L, s->T, t0, t1, ANLS_TOL,
                       anls_round_cap((int)K, bo), bo, a_lds, s->st);
    KCHK("anls_h_sweep_kernel");
    return CMF_OK;
}

int cmf_anls_update_feature_maps(cmf_handle h, const double *W, double *H, int variant, double *loss)
{
    AnlsState *s = nullptr;
    CMFTRY(anls_state(h, &s));
    if (!H || !W) return fail(CMF_ERR_ARG, "NULL argument");
    if (variant != 0 && variant != 1) return fail(CMF_ERR_ARG, "ANLS: variant must be 0 (:basic) or 1 (:block), got %d", variant);
    const int64_t N = s->N, T = s->T, K = s->K, L = s->L;
    if (variant == 1 && T < L)
        return fail(CMF_ERR_ARG, "ANLS: variant=:block needs T >= L (anls.jl:136 indexes T-L+2:T); T = %lld, L = %lld", (long long)T, (long long)L);
    if (K > KMAX) return fail(CMF_ERR_UNSUPPORTED, "ANLS: update_feature_maps! solves K <= %d unknowns per column on one wave (K = %lld)", KMAX, (long long)K);
    if ((L - 1) * K > 6144)
        return fail(CMF_ERR_UNSUPPORTED, "ANLS: update_feature_maps! keeps the last L-1 columns in LDS: (L-1)*K <= 6144 (K = %lld, L = %lld)", (long long)K, (long long)L);
    hipStream_t st = h->stream;
    const size_t KT = (size_t)K * T;
    HIPCHK(hipMemcpyAsync(s->Wd, W, (size_t)K * N * L * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->Hd, H, KT * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(s->st, 0, ST_N * sizeof(unsigned long long), st));
    // B = transconv(W, data) and the lag-Grams stand for the residual windows of anls.jl:27, :76-82
    CMFTRY((fp64_gemm<true, false>(s, st, RULE, WkR{s->Wd, (int)K}, ShiftColsLin{s->data, (int)N, T}, EpiStoreT{s->Bt, K}, K, T, N * L, false)));
    const int64_t per = (2 * L - 1) * K * K;
    hipLaunchKernelGGL(anls_lag_gram_kernel, dim3((unsigned)blocks(per, 256)), dim3(256), 0, st, s->Wd, s->Alag, (int)K, N, (int)L);
    KCHK("anls_lag_gram_kernel");
    const int bo = h->anls_backup_only;
    if (variant == 1) { // anls.jl:105-134: L phases of columns whose windows are disjoint, then the last L-1 columns one by one (:136)
        const double *Afull = s->Alag + (L - 1) * per;
        for (int64_t l = 0; l < L; ++l) {
            if (l > T - L) break;
            const int64_t ncols = (T - L - l) / L + 1;
            hipLaunchKernelGGL(anls_h_block_kernel, dim3((unsigned)ncols), dim3(64), 0, st, Afull, s->Bt, s->Hd, (int)K, (int)L, T, l, ncols, ANLS_TOL,
                               anls_round_cap((int)K, bo), bo, s->st);
            KCHK("anls_h_block_kernel");
        }
        if (L > 1) CMFTRY(sweep(h, s, T - L + 1, T));
    } else {
        CMFTRY(sweep(h, s, 0, T)); // anls.jl:63-94
    }
    // anls.jl:35: norm(resids) / data_norm, the residual formed once from the new H
    CMFTRY((fp64_gemm<false, false>(s, st, RULE, WnR{s->Wd, (int)K, (int)N}, LagHT{s->Hd, (int)K}, EpiLossN{s->data, N}, N, T, K * L, true)));
    HIPCHK(hipMemcpyAsync(&s->host->sum, s->dsum, sizeof(double), hipMemcpyDeviceToHost, st));
    std::vector<double> Hn(KT);
    HIPCHK(hipMemcpyAsync(Hn.data(), s->Hd, KT * sizeof(double), hipMemcpyDeviceToHost, st));
    CMFTRY(finish(s, st, "update_feature_maps!", &s->h_exchanges));
    std::memcpy(H, Hn.data(), KT * sizeof(double));
    if (loss) *loss = std::sqrt(s->host->sum) / s->datanorm;
    return CMF_OK;
}
