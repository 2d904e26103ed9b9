// cmf_sep.hip -- the separable fit (src/algs/separable.jl) on one device, in fp64 end to end, one entry per stage: cmf_sep_prepare,
// cmf_sep_gram, cmf_sep_spa, cmf_sep_nnls, cmf_sep_shift_table, cmf_sep_construct (include/cmf_hip.h).  The kernels are in
// cmf_sep.h, the NNLS solver in cmf_anls.h, the contraction and the shared part of the state in cmf_fp64.h; the rewritings are in
// DESIGN.md 6d.  The decisions on R x R numbers (grouping, sorting) are the host language's.
#include "cmf_internal.h"
#include "cmf_anls.h"
#include "cmf_nnls_large.h"
#include "cmf_sep.h"

using namespace fp64;
using namespace sep;

static const char RULE[] = "separable";
constexpr double SEP_NNLS_TOL = 1e-8; // the solver's threshold (the package's default is not known)

struct SepState : Fp64State { // data: [t][n]
    double *Xs = nullptr, *Y = nullptr;        // the scaled data (N x T as [t][n]) and its projection (R x T as [t][r], made on demand)
    int64_t y_rows = 0;
    double *col1 = nullptr, *col2 = nullptr, *norms = nullptr, *wbuf = nullptr; // T, T, T, MMAX + 1
    int *rec = nullptr;                        // T: the records of sep_select_kernel
    int64_t *vert = nullptr;                   // WMAX .. min(N, T) vertices of a call
    double *Vd = nullptr, *Gram = nullptr, *C = nullptr, *Gd = nullptr, *rowsum = nullptr; // step 2, made on demand for R rows
    double *P = nullptr, *part = nullptr, *head = nullptr;                                // shift table, made on demand
    int64_t nnls_rows = 0, table_rows = 0, table_L = 0, table_splits = 0;
    anls::LargeScratch large;                  // the slabs of nnls_large_kernel (option "nnls_large"), made by the first call that needs them
    unsigned long long *st = nullptr;          // anls::ST_N counters, then FL_N flags
    struct Host { unsigned long long st[anls::ST_N + FL_N]; } *host = nullptr; // pinned
    int64_t exchanges = 0;
    double scaled_thresh = NAN;                // the thresh Xs was made with (NaN: none)
};

void sep_free(cmf_handle_s *h)
{
    if (!h || !h->sep) return;
    fp64_release(h, h->sep);
    anls::large_release(&h->sep->large);
    if (h->sep->host) (void)hipHostFree(h->sep->host);
    delete h->sep;
    h->sep = nullptr;
}

int sep_counter(const cmf_handle_s *h, const char *name, int64_t *value)
{
    if (std::strcmp(name, "sep_nnls_exchanges") == 0) { *value = h->sep ? h->sep->exchanges : 0; return 1; }
    return 0;
}

static int sep_state(cmf_handle h, SepState **out)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    CMFTRY(fp64_single_gpu(h, RULE, false));
    if (!h->sep) return fail(CMF_ERR_STATE, "call cmf_sep_prepare before the entries of the separable fit");
    *out = h->sep;
    HIPCHK(hipSetDevice(h->device));
    return CMF_OK;
}

int cmf_sep_prepare(cmf_handle h, const double *data)
{
    if (!h || !data) return fail(CMF_ERR_ARG, "NULL argument");
    CMFTRY(fp64_single_gpu(h, RULE, true));
    const int64_t N = h->d.N, T = h->d.Tl;
    if (T > (int64_t)65535 * TP) return fail(CMF_ERR_UNSUPPORTED, "separable: T = %lld > %lld", (long long)T, (long long)65535 * TP);
    HIPCHK(hipSetDevice(h->device));
    sep_free(h);
    auto *s = new SepState();
    h->sep = s;
    auto bail = [&](int rc) { sep_free(h); return rc; };
    int rc = fp64_prepare_common(h, s, data);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->Xs, (size_t)N * T);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->col1, (size_t)T);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->col2, (size_t)T);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->norms, (size_t)T);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->wbuf, (size_t)MMAX + 1);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->rec, (size_t)T);
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->vert, (size_t)std::min(N, T));
    if (rc == CMF_OK) rc = fp64_alloc(s, &s->st, anls::ST_N + FL_N);
    if (rc != CMF_OK) return bail(rc);
    if (hipHostMalloc(&s->host, sizeof(SepState::Host)) != hipSuccess) return bail(fail(CMF_ERR_HIP, "hipHostMalloc failed"));
    return CMF_OK;
}

// lanes that share a column of M rows: the least power of two >= M in 8..64
static int lane_group(int64_t M)
{
    int g = 8;
    while (g < 64 && g < M) g <<= 1;
    return g;
}
static unsigned column_grid(int64_t T, int G) { return (unsigned)blocks(T, (int64_t)COLS_IT * 4 * (64 / G)); }

static int scale(SepState *s, hipStream_t st, double thresh)
{
    if (s->scaled_thresh == thresh) return CMF_OK; // (Xs is read-only once made: SPA without `pre` works on a copy)
    const int G = lane_group(s->N);
    hipLaunchKernelGGL(sep_scale_kernel, dim3(column_grid(s->T, G)), dim3(256), 0, st, s->data, s->Xs, s->col1, s->col2, (int)s->N, s->T, thresh, G);
    KCHK("sep_scale_kernel");
    s->scaled_thresh = thresh;
    return CMF_OK;
}

static int check_thresh(double thresh)
{
    if (!(thresh == thresh)) return fail(CMF_ERR_ARG, "separable: thresh is NaN");
    return CMF_OK;
}

int cmf_sep_gram(cmf_handle h, double thresh, double *XXt)
{
    SepState *s = nullptr;
    CMFTRY(sep_state(h, &s));
    if (!XXt) return fail(CMF_ERR_ARG, "NULL argument");
    CMFTRY(check_thresh(thresh));
    const int64_t N = s->N, T = s->T;
    hipStream_t st = h->stream;
    CMFTRY(scale(s, st, thresh));
    double *D = nullptr;
    HIPCHK(hipMalloc(&D, (size_t)N * N * sizeof(double)));
    int rc = fp64_gemm<true, true>(s, st, RULE, ColMajor{s->Xs, N}, RowMajor{s->Xs, N}, EpiStore{D, N, 0.0}, N, N, T, false);
    if (rc == CMF_OK && hipMemcpyAsync(XXt, D, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(CMF_ERR_HIP, "read-back of X X' failed");
    if (hipStreamSynchronize(st) != hipSuccess && rc == CMF_OK) rc = fail(CMF_ERR_HIP, "the contraction X X' failed");
    (void)hipFree(D);
    return rc;
}

int cmf_sep_spa(cmf_handle h, int64_t R, double thresh, int pre, const double *proj, int64_t *vertices)
{
    SepState *s = nullptr;
    CMFTRY(sep_state(h, &s));
    if (!vertices) return fail(CMF_ERR_ARG, "NULL argument");
    CMFTRY(check_thresh(thresh));
    const int64_t N = s->N, T = s->T;
    if (R < 1 || R > std::min(N, T)) return fail(CMF_ERR_ARG, "separable: SPA needs 1 <= R <= min(N, T) (R = %lld, N = %lld, T = %lld)", (long long)R, (long long)N, (long long)T);
    if (pre < 0 || pre > 2) return fail(CMF_ERR_ARG, "separable: pre must be 0 (none), 1 (:svd) or 2 (:svdcond), got %d", pre);
    if ((pre != 0) != (proj != nullptr)) return fail(CMF_ERR_ARG, "separable: `proj` (R x N) goes with pre = 1 or 2 and only with them");
    if (N > MMAX) return fail(CMF_ERR_UNSUPPORTED, "separable: SPA holds a column of the residual in LDS: N <= %d (N = %lld)", MMAX, (long long)N);
    hipStream_t st = h->stream;
    CMFTRY(scale(s, st, thresh));
    const int64_t M = pre ? R : N;
    if (s->y_rows < M) { // the residual SPA edits: a copy of Xs, or its projection
        CMFTRY(fp64_alloc(s, &s->Y, (size_t)M * T));
        s->y_rows = M;
    }
    double *projd = nullptr;
    if (pre) { // pre_svd / pre_svdcond (:323-333): Y = proj * Xs, proj from the eigen-decomposition of X X' (the caller's)
        HIPCHK(hipMalloc(&projd, (size_t)R * N * sizeof(double)));
        if (hipMemcpyAsync(projd, proj, (size_t)R * N * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) {
            (void)hipFree(projd);
            return fail(CMF_ERR_HIP, "upload of proj failed");
        }
        const int rc = fp64_gemm<false, false>(s, st, RULE, RowMajor{projd, N}, ColMajor{s->Xs, N}, anls::EpiStoreT{s->Y, R}, R, T, N, false);
        if (rc != CMF_OK) { (void)hipStreamSynchronize(st); (void)hipFree(projd); return rc; }
    } else {
        HIPCHK(hipMemcpyAsync(s->Y, s->Xs, (size_t)N * T * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    auto done = [&](int rc) { (void)hipStreamSynchronize(st); if (projd) (void)hipFree(projd); return rc; };
    if (hipMemsetAsync(s->st, 0, (anls::ST_N + FL_N) * sizeof(unsigned long long), st) != hipSuccess) return done(fail(CMF_ERR_HIP, "hipMemsetAsync failed"));
    const int G = lane_group(M);
    const dim3 grid(column_grid(T, G));
    const size_t lds = (size_t)M * sizeof(double);
    const double band = std::sqrt(DBL_EPS); // findsetmax's thresh (:403)
    for (int64_t r = 0; r < R; ++r) { // :303-316
        hipLaunchKernelGGL(sep_project_kernel, grid, dim3(256), lds, st, s->Y, (int)M, T, s->wbuf, s->norms, G, r > 0 ? 1 : 0);
        hipLaunchKernelGGL(sep_select_kernel, dim3(1), dim3(SEL), 0, st, s->norms, s->col2, T, s->Y, (int)M, band, (int)r, s->vert, s->wbuf, s->rec,
                           s->st + anls::ST_N);
    }
    if (hipGetLastError() != hipSuccess) return done(fail(CMF_ERR_HIP, "launch of the SPA kernels failed"));
    std::vector<int64_t> v((size_t)R);
    if (hipMemcpyAsync(v.data(), s->vert, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(s->host->st, s->st, sizeof(s->host->st), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return done(fail(CMF_ERR_HIP, "SPA failed on the device: %s", hipGetErrorString(hipGetLastError())));
    if (projd) (void)hipFree(projd);
    if (s->host->st[anls::ST_N + FL_ZERO_W])
        return fail(CMF_ERR_UNSUPPORTED, "separable: the SPA residual vanished in %llu round(s): the (thresholded) data has fewer than R = %lld independent columns",
                    s->host->st[anls::ST_N + FL_ZERO_W], (long long)R);
    std::sort(v.begin(), v.end()); // :318
    std::copy(v.begin(), v.end(), vertices);
    return CMF_OK;
}

// the buffers of step 2 for R rows (a state that has grown keeps its smaller buffers until it is released)
static int step2_buffers(SepState *s, int64_t R)
{
    if (s->nnls_rows >= R) return CMF_OK;
    CMFTRY(fp64_alloc(s, &s->Vd, (size_t)R * s->N));
    CMFTRY(fp64_alloc(s, &s->Gram, (size_t)R * R));
    CMFTRY(fp64_alloc(s, &s->C, (size_t)R * s->T));
    CMFTRY(fp64_alloc(s, &s->Gd, (size_t)R * s->T));
    CMFTRY(fp64_alloc(s, &s->rowsum, (size_t)R));
    s->nnls_rows = R;
    return CMF_OK;
}

int cmf_sep_nnls(cmf_handle h, int64_t *vertices, int64_t R, double *V, double *G)
{
    SepState *s = nullptr;
    CMFTRY(sep_state(h, &s));
    if (!vertices || !V || !G) return fail(CMF_ERR_ARG, "NULL argument");
    const int64_t N = s->N, T = s->T;
    if (R < 1) return fail(CMF_ERR_ARG, "separable: R = %lld", (long long)R);
    const bool large = R > anls::WMAX && h->nnls_large;
    if (R > anls::WMAX && !large)
        return fail(CMF_ERR_UNSUPPORTED, "separable: the NNLS step solves R = K*L <= %d unknowns per column in LDS (R = %lld)", anls::WMAX, (long long)R);
    if (R > anls::WLARGE)
        return fail(CMF_ERR_UNSUPPORTED, "separable: the NNLS step solves R = K*L <= %d unknowns per column (option \"nnls_large\"; R = %lld)", anls::WLARGE, (long long)R);
    for (int64_t r = 0; r < R; ++r)
        if (vertices[r] < 0 || vertices[r] >= T) return fail(CMF_ERR_ARG, "separable: vertex %lld is not a column of the data (T = %lld)", (long long)vertices[r], (long long)T);
    hipStream_t st = h->stream;
    CMFTRY(step2_buffers(s, R));
    int64_t *vd = nullptr;
    HIPCHK(hipMalloc(&vd, (size_t)R * sizeof(int64_t)));
    auto done = [&](int rc) { (void)hipStreamSynchronize(st); (void)hipFree(vd); return rc; };
    auto step = [&]() -> int {
        HIPCHK(hipMemcpyAsync(vd, vertices, (size_t)R * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(s->st, 0, (anls::ST_N + FL_N) * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(sep_gather_kernel, dim3((unsigned)R), dim3(256), 0, st, s->data, vd, s->Vd, (int)N); // V = data[:, vertices] (:23)
        KCHK("sep_gather_kernel");
        // G = nonneg_lsq(V, data) (:26) on the normal equations V'V g = V'data[:, t], all T columns sharing the Gram
        CMFTRY((fp64_gemm<false, false>(s, st, RULE, RowMajor{s->Vd, N}, ColMajor{s->Vd, N}, EpiStore{s->Gram, R, 0.0}, R, R, N, false)));
        CMFTRY((fp64_gemm<false, false>(s, st, RULE, RowMajor{s->Vd, N}, ColMajor{s->data, N}, EpiStore{s->C, T, 0.0}, R, T, N, false)));
        if (large) {
            CMFTRY(anls::nnls_large(&s->large, st, RULE, s->Gram, s->C, s->Gd, (int)R, T, SEP_NNLS_TOL, 0, s->st));
        } else {
            hipLaunchKernelGGL(anls::anls_nnls_w_kernel, dim3((unsigned)T), dim3(256), 0, st, s->Gram, s->C, s->Gd, (int)R, T, SEP_NNLS_TOL,
                               anls::anls_round_cap((int)R, 0), 0, s->st);
            KCHK("anls_nnls_w_kernel");
        }
        HIPCHK(hipMemcpyAsync(s->host->st, s->st, sizeof(s->host->st), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return CMF_OK;
    };
    int rc = step();
    if (rc != CMF_OK) return done(rc);
    s->exchanges = (int64_t)s->host->st[anls::ST_ROUNDS];
    if (s->host->st[anls::ST_BADPIVOT])
        return done(fail(CMF_ERR_UNSUPPORTED, "separable NNLS: the Gram of a passive set is not positive definite in %llu problem(s) (dependent vertices or non-finite "
                                              "input); V and G are left as they were", s->host->st[anls::ST_BADPIVOT]));
    if (s->host->st[anls::ST_CAPPED])
        return done(fail(CMF_ERR_UNSUPPORTED, "separable NNLS: %llu problem(s) hit the cap on pivoting rounds; V and G are left as they were", s->host->st[anls::ST_CAPPED]));
    std::vector<double> Vh((size_t)R * N), Gh((size_t)R * T);
    auto finish = [&]() -> int { // renormalize! (:340-348)
        hipLaunchKernelGGL(sep_rowsum_kernel, dim3((unsigned)R), dim3(256), 0, st, s->Gd, T, 0, 0, s->rowsum);
        KCHK("sep_rowsum_kernel");
        hipLaunchKernelGGL(sep_rescale_kernel, dim3((unsigned)R), dim3(256), 0, st, s->Gd, T, s->Vd, (int)N, s->rowsum);
        KCHK("sep_rescale_kernel");
        HIPCHK(hipMemcpyAsync(Vh.data(), s->Vd, Vh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(Gh.data(), s->Gd, Gh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return CMF_OK;
    };
    rc = finish();
    if (rc != CMF_OK) return done(rc);
    (void)hipFree(vd);
    std::memcpy(V, Vh.data(), Vh.size() * sizeof(double)); // [r][n] is Julia's N x R
    for (int64_t r = 0; r < R; ++r)
        for (int64_t t = 0; t < T; ++t) G[r + R * t] = Gh[(size_t)r * T + t];
    return CMF_OK;
}

int cmf_sep_shift_table(cmf_handle h, const double *G, int64_t R, int64_t L, double *P, double *head)
{
    SepState *s = nullptr;
    CMFTRY(sep_state(h, &s));
    if (!G || !P || !head) return fail(CMF_ERR_ARG, "NULL argument");
    const int64_t T = s->T;
    if (R < 1 || L < 1 || L > T) return fail(CMF_ERR_ARG, "separable: the shift table needs R >= 1 and 1 <= L <= T (R = %lld, L = %lld, T = %lld)", (long long)R, (long long)L, (long long)T);
    if (R > (1 << 14) || L > (1 << 14)) return fail(CMF_ERR_UNSUPPORTED, "separable: shift table of R = %lld, L = %lld", (long long)R, (long long)L);
    std::vector<double> Gr((size_t)R * T); // [r][t]
    for (int64_t r = 0; r < R; ++r) {
        bool any = false;
        for (int64_t t = 0; t < T; ++t) { const double v = G[r + R * t]; Gr[(size_t)r * T + t] = v; any = any || v != 0.0; }
        if (!any) return fail(CMF_ERR_UNSUPPORTED, "separable: row %lld of G is zero: its shift cosines are 0/0 (:378-380)", (long long)r);
    }
    const int64_t chunk = std::max<int64_t>(2048, rup(blocks(T, 16), TR)), splits = blocks(T, chunk), PL = R * L;
    if (s->table_rows < R || s->table_L < L || s->table_splits < splits) {
        CMFTRY(fp64_alloc(s, &s->P, (size_t)R * PL));
        CMFTRY(fp64_alloc(s, &s->part, (size_t)splits * R * PL));
        CMFTRY(fp64_alloc(s, &s->head, (size_t)PL));
        s->table_rows = R; s->table_L = L; s->table_splits = splits;
    }
    CMFTRY(step2_buffers(s, R));
    hipStream_t st = h->stream;
    std::vector<double> Ph((size_t)R * PL), hh((size_t)PL);
    auto run = [&]() -> int {
        HIPCHK(hipMemcpyAsync(s->Gd, Gr.data(), Gr.size() * sizeof(double), hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)blocks(R, TM), (unsigned)blocks(PL, TP), (unsigned)splits);
        hipLaunchKernelGGL(sep_lag_kernel, grid, dim3(256), 0, st, s->Gd, (int)R, (int)L, T, chunk, s->part);
        KCHK("sep_lag_kernel");
        hipLaunchKernelGGL(sep_lag_sum_kernel, dim3((unsigned)blocks(R * PL, 256)), dim3(256), 0, st, s->part, R * PL, (int)splits, s->P);
        KCHK("sep_lag_sum_kernel");
        hipLaunchKernelGGL(sep_rowsum_kernel, dim3((unsigned)PL), dim3(256), 0, st, s->Gd, T, (int)L, 1, s->head);
        KCHK("sep_rowsum_kernel");
        HIPCHK(hipMemcpyAsync(Ph.data(), s->P, Ph.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hh.data(), s->head, hh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return CMF_OK;
    };
    const int rc = run();
    if (rc != CMF_OK) { (void)hipStreamSynchronize(st); return rc; }
    // the device's [a][b][l] and [a][l] to Julia's P[a + R*(b + R*l)] and head[a + R*l]
    for (int64_t a = 0; a < R; ++a)
        for (int64_t b = 0; b < R; ++b)
            for (int64_t l = 0; l < L; ++l) P[a + R * (b + R * l)] = Ph[(size_t)(a * R + b) * L + l];
    for (int64_t a = 0; a < R; ++a)
        for (int64_t l = 0; l < L; ++l) head[a + R * l] = hh[(size_t)a * L + l];
    return CMF_OK;
}

int cmf_sep_construct(cmf_handle h, const double *V, const double *G, int64_t *groups, double *W, double *H)
{
    SepState *s = nullptr;
    CMFTRY(sep_state(h, &s));
    if (!V || !G || !groups || !W || !H) return fail(CMF_ERR_ARG, "NULL argument");
    const int64_t N = s->N, T = s->T, K = s->K, L = s->L, R = K * L;
    for (int64_t i = 0; i < R; ++i)
        if (groups[i] < 0 || groups[i] >= R) return fail(CMF_ERR_ARG, "separable: groups[%lld] = %lld is not a row of G (R = %lld)", (long long)i, (long long)groups[i], (long long)R);
    // construct_WH (:59-87, average_H=true): K*T*L additions, done where the arrays are.  groups is Julia's K x L: groups[k + K*l]
    for (int64_t l = 0; l < L; ++l)
        for (int64_t n = 0; n < N; ++n)
            for (int64_t k = 0; k < K; ++k) W[k + K * (n + N * l)] = V[n + N * groups[k + K * l]]; // :66-68
    for (int64_t t = 0; t < T; ++t)
        for (int64_t k = 0; k < K; ++k) {
            double sum = 0.0;
            for (int64_t l = 0; l < L && t + l < T; ++l) sum += G[groups[k + K * l] + R * (t + l)]; // :74-76
            H[k + K * t] = sum / (double)(std::min(T, t + L + 1) - t);                             // :77: min(T, t+L) - t + 1 in 1-based t
        }
    return CMF_OK;
}
