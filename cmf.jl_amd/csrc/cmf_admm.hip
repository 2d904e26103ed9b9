// cmf_admm.hip -- the ADMM rule (src/algs/admm.jl) on one device, in fp64 end to end: cmf_admm_prepare,
// cmf_admm_update_motifs, cmf_admm_update_feature_maps (include/cmf_hip.h).  The kernels are in cmf_admm.h, the contraction and
// the part of the state that the ANLS rule has too in cmf_fp64.h; the rewritings that keep the K x N x T tensor `wh` and the T
// Gram products of the reference out of the computation are in DESIGN.md, "The ADMM rule".
#include "cmf_internal.h"
#include "cmf_admm.h"

using namespace fp64;
using namespace admm;

static const char RULE[] = "ADMM";

struct AdmmState : Fp64State { // Hd: K x T row-major, the H the W call reads
    int64_t F = 0;  // frequencies solved: 0..T/2 (the spectrum of real rows is Hermitian)
    int64_t M = 1;  // Bluestein length: a power of two >= 2T-1
    double *Z1 = nullptr, *D1 = nullptr, *est = nullptr; // N x T: Z1, its dual (U1' / Q1), est (H side)
    double *G = nullptr, *Gt = nullptr;              // LK x LK: Cholesky factor of Hstk*Hstk' + 2I and its transpose
    double *Wstk = nullptr, *Z2w = nullptr, *Z3w[2] = {nullptr, nullptr}, *U2 = nullptr, *U3 = nullptr; // LK x N, [i][n]
    double *Hh = nullptr, *Z2h = nullptr, *Z3h[2] = {nullptr, nullptr}, *Q2 = nullptr, *Q3 = nullptr, *yr = nullptr; // K x T row-major
    double2 *Y = nullptr;                            // K x T complex
    double2 *fa = nullptr, *fb = nullptr;            // K x M complex: Bluestein work
    double2 *chirp = nullptr, *bh = nullptr;         // T, M
    double *Alag = nullptr;                          // (2L-1) x K x K
    double2 *Lf = nullptr;                           // K x K x F: the per-frequency factors
    double *hsum = nullptr;                          // pinned: the loss sum read back
    int64_t w_reverts = 0, h_reverts = 0;            // of the last call of each kind
};

void admm_free(cmf_handle_s *h)
{
    if (!h || !h->admm) return;
    fp64_release(h, h->admm);
    if (h->admm->hsum) (void)hipHostFree(h->admm->hsum);
    delete h->admm;
    h->admm = nullptr;
}

// the sum the last loss contraction left in dsum, as norm / datanorm
static int read_loss(AdmmState *s, hipStream_t st, double *loss)
{
    HIPCHK(hipMemcpyAsync(s->hsum, s->dsum, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *loss = std::sqrt(*s->hsum) / s->datanorm;
    return CMF_OK;
}

// radix-2 Stockham FFT of length M on `rows` rows, ping-ponging between *a and *b; the result ends in *a
static int stockham(hipStream_t st, double2 **a, double2 **b, int64_t M, int rows, double sign)
{
    const dim3 grid((unsigned)blocks(std::max<int64_t>(M / 2, 1), 256), (unsigned)rows);
    for (int64_t Ns = 1; Ns < M; Ns <<= 1) {
        hipLaunchKernelGGL(admm_fft_stage_kernel, grid, dim3(256), 0, st, *a, *b, M, Ns, sign);
        KCHK("admm_fft_stage_kernel");
        std::swap(*a, *b);
    }
    return CMF_OK;
}

// DFT along the K rows of x (length T, row stride T): out[k][f] = sum_s x[k][s] exp(-2 pi i f s / T).
// INV: x is complex and is conjugated on the way in, and out receives Re(result) * scale (real rows): with scale = 1/T that is
// real(ifft(x)) of the reference (admm.jl:270-271).  Else x is real and out complex.
template <bool INV>
static int dft_rows(AdmmState *s, hipStream_t st, const void *x, void *out, double scale)
{
    const int K = (int)s->K;
    const dim3 gM((unsigned)blocks(s->M, 256), (unsigned)K), gT((unsigned)blocks(s->T, 256), (unsigned)K);
    hipLaunchKernelGGL((admm_fft_pre_kernel<!INV, INV>), gM, dim3(256), 0, st, x, s->chirp, s->fa, s->T, s->M);
    KCHK("admm_fft_pre_kernel");
    double2 *a = s->fa, *b = s->fb;
    CMFTRY(stockham(st, &a, &b, s->M, K, -1.0));
    hipLaunchKernelGGL(admm_fft_mul_kernel, gM, dim3(256), 0, st, a, s->bh, s->M);
    KCHK("admm_fft_mul_kernel");
    CMFTRY(stockham(st, &a, &b, s->M, K, 1.0));
    hipLaunchKernelGGL((admm_fft_post_kernel<INV>), gT, dim3(256), 0, st, a, s->chirp, out, s->T, s->M, scale);
    KCHK("admm_fft_post_kernel");
    return CMF_OK;
}

static int admm_state(cmf_handle h, AdmmState **out)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    CMFTRY(fp64_single_gpu(h, RULE, false));
    if (!h->admm) return fail(CMF_ERR_STATE, "call cmf_admm_prepare before the ADMM rule entries");
    *out = h->admm;
    HIPCHK(hipSetDevice(h->device));
    return CMF_OK;
}

int cmf_admm_prepare(cmf_handle h, const double *data)
{
    if (!h || !data) return fail(CMF_ERR_ARG, "NULL argument");
    CMFTRY(fp64_single_gpu(h, RULE, true));
    const int64_t N = h->d.N, T = h->d.Tl, K = h->d.K, L = h->d.L;
    if (L * K > 8192) return fail(CMF_ERR_UNSUPPORTED, "ADMM: L*K = %lld > 8192 (the stacked solve keeps a column of L*K in LDS)", (long long)(L * K));
    if (T > (int64_t)65535 * TP) return fail(CMF_ERR_UNSUPPORTED, "ADMM: T = %lld > %lld", (long long)T, (long long)65535 * TP);
    HIPCHK(hipSetDevice(h->device));
    admm_free(h);
    auto *s = new AdmmState();
    h->admm = s;
    auto bail = [&](int rc) { admm_free(h); return rc; };
    int rc = fp64_prepare_common(h, s, data);
    if (rc != CMF_OK) return bail(rc);
    s->F = T / 2 + 1;
    while (s->M < 2 * T - 1) s->M <<= 1;
    const size_t NT = (size_t)N * T, KT = (size_t)K * T, LKN = (size_t)s->LK * N;
    for (double **p : {&s->Z1, &s->D1, &s->est})
        if (rc == CMF_OK) rc = fp64_alloc(s, p, NT);
    for (double **p : {&s->Wstk, &s->Z2w, &s->Z3w[0], &s->Z3w[1], &s->U2, &s->U3})
        if (rc == CMF_OK) rc = fp64_alloc(s, p, LKN);
    for (double **p : {&s->Hh, &s->Z2h, &s->Z3h[0], &s->Z3h[1], &s->Q2, &s->Q3, &s->yr})
        if (rc == CMF_OK) rc = fp64_alloc(s, p, KT);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->G, (size_t)s->LK * s->LK);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->Gt, (size_t)s->LK * s->LK);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->Y, KT);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->fa, (size_t)K * s->M);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->fb, (size_t)K * s->M);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->chirp, (size_t)T);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->bh, (size_t)s->M);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->Alag, (size_t)(2 * L - 1) * K * K);
    if (rc == CMF_OK && K <= 64) rc = fp64_alloc(s, &s->Lf, (size_t)K * K * s->F);
    if (rc != CMF_OK) return bail(rc);
    if (hipHostMalloc(&s->hsum, sizeof(double)) != hipSuccess) return bail(fail(CMF_ERR_HIP, "hipHostMalloc failed"));
    // Bluestein chirp and the transform of its conjugate (depend on T only)
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(admm_chirp_kernel, dim3((unsigned)blocks(s->M, 256)), dim3(256), 0, st, s->chirp, s->bh, T, s->M);
    if (hipGetLastError() != hipSuccess) return bail(fail(CMF_ERR_HIP, "launch of admm_chirp_kernel failed"));
    double2 *a = s->bh, *b = s->fa;
    if ((rc = stockham(st, &a, &b, s->M, 1, -1.0)) != CMF_OK) return bail(rc);
    if (a != s->bh && hipMemcpyAsync(s->bh, a, (size_t)s->M * sizeof(double2), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return bail(fail(CMF_ERR_HIP, "copy of the chirp transform failed"));
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(CMF_ERR_HIP, "cmf_admm_prepare: the device failed"));
    return CMF_OK;
}

// reverts per call: cmf_get_counter "admm_W_reverts" / "admm_H_reverts"
int admm_counter(const cmf_handle_s *h, const char *name, int64_t *value)
{
    if (std::strcmp(name, "admm_W_reverts") == 0) { *value = h->admm ? h->admm->w_reverts : 0; return 1; }
    if (std::strcmp(name, "admm_H_reverts") == 0) { *value = h->admm ? h->admm->h_reverts : 0; return 1; }
    return 0;
}

// the revert-and-break rule of admm.jl:99-107 / :203-211 on the call's own loss history; returns true to break
static bool admm_decide(std::vector<double> &hist, double loss, double tol, int64_t *reverts, bool *revert)
{
    hist.push_back(loss);
    *revert = false;
    if (hist.size() < 2) return false;
    const double diff = hist[hist.size() - 2] - hist.back();
    if (diff < 0) {
        *revert = true;
        hist.pop_back();
        ++*reverts;
    }
    return diff < tol;
}

int cmf_admm_update_motifs(cmf_handle h, const double *H, double *W, double rhow, int64_t maxiter, double tol, int nonnegW, int64_t *iters)
{
    AdmmState *s = nullptr;
    CMFTRY(admm_state(h, &s));
    if (!H || !W) return fail(CMF_ERR_ARG, "NULL argument");
    if (maxiter < 0) return fail(CMF_ERR_ARG, "admm_W_maxiter < 0");
    const int64_t N = s->N, T = s->T, K = s->K, L = s->L, LK = s->LK;
    hipStream_t st = h->stream;
    std::vector<double> Hr;
    CMFTRY(fp64_upload_H_rows(s, st, H, Hr));
    const size_t NT = (size_t)N * T, LKN = (size_t)LK * N;
    for (double *p : {s->Z1, s->D1}) HIPCHK(hipMemsetAsync(p, 0, NT * sizeof(double), st)); // admm.jl:36-48: everything starts at zero
    for (double *p : {s->Wstk, s->Z2w, s->Z3w[0], s->Z3w[1], s->U2, s->U3}) HIPCHK(hipMemsetAsync(p, 0, LKN * sizeof(double), st));
    // G = Hstk*Hstk' + 2I, factorised once per call (:51-53)
    const HstkRT hs{s->Hd, (int)K, (int)T};
    const HstkTR hst{s->Hd, (int)K, (int)T};
    CMFTRY((fp64_gemm<false, false>(s, st, RULE, hs, hst, EpiStore{s->G, LK, 2.0}, LK, LK, T, false)));
    hipLaunchKernelGGL(admm_chol_kernel, dim3(1), dim3(1024), 0, st, s->G, s->Gt, (int)LK);
    KCHK("admm_chol_kernel");
    const double c1 = 1.0 / (1.0 + 1.0 / rhow), c2 = 1.0 / rhow;
    int cur = 0; // Z3 = Z3w[cur]; Z3_last = Z3w[cur ^ 1]
    std::vector<double> hist;
    int64_t it = 0, reverts = 0;
    while (it < maxiter) {
        ++it;
        // 1. Wstk = G \ (Hstk*(Z1-U1) + Z2-U2 + Z3-U3)   (:63-65)
        CMFTRY((fp64_gemm<false, true>(s, st, RULE, hs, RowMajorDiff{s->Z1, s->D1, N}, EpiRhsW{s->Wstk, s->Z2w, s->U2, s->Z3w[cur], s->U3, N}, LK, N, T, false)));
        hipLaunchKernelGGL(admm_trsm_kernel, dim3((unsigned)N), dim3(64), LK * sizeof(double), st, s->G, s->Gt, s->Wstk, (int)LK, N);
        KCHK("admm_trsm_kernel");
        // 2-3. estT = Hstk'*Wstk; Z1 = c1*((estT+U1) + c2*data'); U1 += estT - Z1   (:68-69, 89)
        CMFTRY((fp64_gemm<true, true>(s, st, RULE, hst, RowMajor{s->Wstk, N}, EpiZ1W{s->Z1, s->D1, s->data, N, c1, c2}, T, N, LK, false)));
        // 4-6. column norms with the w[n] >= 1 rule, Z3 = max(0, Wstk+U3) into Z3_last's buffer, U2, U3   (:72-91)
        hipLaunchKernelGGL(admm_w_cols_kernel, dim3((unsigned)blocks(N, 256)), dim3(256), 0, st, s->Wstk, s->Z2w, s->U2, s->Z3w[cur ^ 1], s->U3,
                           (int)LK, N, nonnegW ? 1 : 0);
        KCHK("admm_w_cols_kernel");
        cur ^= 1;
        // 7. loss = norm(data' - Hstk'*Z3) / norm(data)   (:93-96)
        CMFTRY((fp64_gemm<true, true>(s, st, RULE, hst, RowMajor{s->Z3w[cur], N}, EpiLossT{s->data, N}, T, N, LK, true)));
        double loss = 0.0;
        CMFTRY(read_loss(s, st, &loss));
        bool revert = false;
        const bool stop = admm_decide(hist, loss, tol, &reverts, &revert); // 8. (:99-107)
        if (revert) cur ^= 1;
        if (stop) break;
    }
    // fold: W[k, n, l] = Z3[l*K + k, n]   (:114-120)
    std::vector<double> Z((size_t)LK * N);
    HIPCHK(hipMemcpyAsync(Z.data(), s->Z3w[cur], Z.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    fp64_fold_W(Z.data(), W, K, N, L);
    s->w_reverts = reverts;
    if (iters) *iters = it;
    return CMF_OK;
}

int cmf_admm_update_feature_maps(cmf_handle h, const double *W, double *H, double rhoh, int64_t maxiter, double l1H, double tol, int nonnegH,
                                 double *loss, int64_t *iters)
{
    AdmmState *s = nullptr;
    CMFTRY(admm_state(h, &s));
    if (!H || !W) return fail(CMF_ERR_ARG, "NULL argument");
    if (maxiter < 0) return fail(CMF_ERR_ARG, "admm_H_maxiter < 0");
    const int64_t N = s->N, T = s->T, K = s->K, L = s->L;
    if (T < L) return fail(CMF_ERR_ARG, "ADMM: update_feature_maps! needs T >= L (admm.jl:233 indexes wh[:, :, 1:L]); T = %lld, L = %lld", (long long)T, (long long)L);
    if (K > 64) return fail(CMF_ERR_UNSUPPORTED, "ADMM: update_feature_maps! factorises a K x K Gram per frequency for K <= 64 (K = %lld)", (long long)K);
    hipStream_t st = h->stream;
    const size_t NT = (size_t)N * T, KT = (size_t)K * T;
    HIPCHK(hipMemcpyAsync(s->Wd, W, (size_t)K * N * L * sizeof(double), hipMemcpyHostToDevice, st));
    for (double *p : {s->Z1, s->D1}) HIPCHK(hipMemsetAsync(p, 0, NT * sizeof(double), st)); // admm.jl:152-163
    for (double *p : {s->Z2h, s->Z3h[0], s->Z3h[1], s->Q2, s->Q3}) HIPCHK(hipMemsetAsync(p, 0, KT * sizeof(double), st));
    // precompute_solveH(W, 1, T) (:167, :229-247) as 2L-1 lag matrices and one factorisation per frequency 0..T/2
    const int64_t nA = (2 * L - 1) * K * K;
    hipLaunchKernelGGL(admm_lag_gram_kernel, dim3((unsigned)blocks(nA, 256)), dim3(256), 0, st, s->Wd, s->Alag, (int)K, N, (int)L);
    KCHK("admm_lag_gram_kernel");
    hipLaunchKernelGGL(admm_freq_chol_kernel, dim3((unsigned)blocks(s->F, 64)), dim3(64), 0, st, s->Alag, s->Lf, (int)K, (int)L, T, s->F);
    KCHK("admm_freq_chol_kernel");
    const double c1 = 1.0 / (1.0 + 1.0 / rhoh), c2 = 1.0 / rhoh, lam = l1H / rhoh;
    const WkR wk{s->Wd, (int)K};
    const WnR wn{s->Wd, (int)K, (int)N};
    int cur = 0;
    std::vector<double> hist;
    int64_t it = 0, reverts = 0;
    while (it < maxiter) {
        ++it;
        // 1. H = real(ifft(Gram_f \ fft(circtransconv(W, Z1-Q1) + Z2-Q2 + Z3-Q3)))   (:180-182, fastsolveH! :249-272 with rho = 1)
        CMFTRY((fp64_gemm<true, false>(s, st, RULE, wk, ShiftColsDiff{s->Z1, s->D1, (int)N, (int)T},
                                  EpiRhsH{s->yr, s->Z2h, s->Q2, s->Z3h[cur], s->Q3, T}, K, T, N * L, false)));
        CMFTRY(dft_rows<false>(s, st, s->yr, s->Y, 1.0));
        hipLaunchKernelGGL(admm_freq_solve_kernel, dim3((unsigned)blocks(s->F, 64)), dim3(64), 0, st, s->Lf, s->Y, (int)K, T, s->F);
        KCHK("admm_freq_solve_kernel");
        CMFTRY(dft_rows<true>(s, st, s->Y, s->Hh, 1.0 / (double)T));
        // 2. est = circular conv(W, H); Z1 = c1*((est+Q1) + c2*data)   (:185-186)
        CMFTRY((fp64_gemm<false, true>(s, st, RULE, wn, LagH<true>{s->Hh, (int)K, (int)T}, EpiZ1H{s->est, s->Z1, s->D1, s->data, N, c1, c2}, N, T, K * L, false)));
        // 3-4. Z2 = shrink(H+Q2), Z3 = max(0, H+Q3) into Z3_last's buffer   (:189-197)
        hipLaunchKernelGGL(admm_h_aux_kernel, dim3((unsigned)blocks(KT, 256)), dim3(256), 0, st, s->Hh, s->Q2, s->Q3, s->Z2h, s->Z3h[cur ^ 1], (int64_t)KT,
                           lam, nonnegH ? 1 : 0);
        KCHK("admm_h_aux_kernel");
        cur ^= 1;
        // 5. loss of the linear conv(W, Z3), then revert / break BEFORE the dual update   (:199-211)
        CMFTRY((fp64_gemm<false, true>(s, st, RULE, wn, LagH<false>{s->Z3h[cur], (int)K, (int)T}, EpiLossN{s->data, N}, N, T, K * L, true)));
        double l = 0.0;
        CMFTRY(read_loss(s, st, &l));
        bool revert = false;
        const bool stop = admm_decide(hist, l, tol, &reverts, &revert);
        if (revert) cur ^= 1;
        if (stop) break;
        // 6. Q1 += est - Z1, Q2 += H - Z2, Q3 += H - Z3   (:214-216)
        hipLaunchKernelGGL(admm_h_dual_kernel, dim3((unsigned)blocks((int64_t)std::max(NT, KT), 256)), dim3(256), 0, st, s->D1, s->est, s->Z1, (int64_t)NT,
                           s->Q2, s->Q3, s->Hh, s->Z2h, s->Z3h[cur], (int64_t)KT);
        KCHK("admm_h_dual_kernel");
    }
    // H .= Z3 (:219); the call returns norm(conv(W, H) - data) / norm(data) (:225)
    CMFTRY((fp64_gemm<false, true>(s, st, RULE, wn, LagH<false>{s->Z3h[cur], (int)K, (int)T}, EpiLossN{s->data, N}, N, T, K * L, true)));
    double l = 0.0;
    CMFTRY(read_loss(s, st, &l));
    std::vector<double> Hr(KT);
    HIPCHK(hipMemcpyAsync(Hr.data(), s->Z3h[cur], KT * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t t = 0; t < T; ++t)
        for (int64_t k = 0; k < K; ++k) H[k + K * t] = Hr[(size_t)k * T + t];
    s->h_reverts = reverts;
    if (loss) *loss = l;
    if (iters) *iters = it;
    return CMF_OK;
}
