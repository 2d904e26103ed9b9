// cmf_signif.hip -- the host side of cmf_null_shifts / cmf_null_moments (include/cmf_hip.h): seqNMF's significance test of components
// on held-out data (test_significance.m).  The kernels and the definition of the shifts are in cmf_signif.h.  Nothing here touches the
// state of a rule: the entries read the handle's raw data (XT) and its resident W (Wn) and write scratch of their own.
#include "cmf_internal.h"
#include "cmf_signif.h"

struct SignifState {
    float *tab = nullptr;      // [Lp][Np][C32 of a full batch]: the null motifs of the batch in flight
    double *partial = nullptr; // [TB][C32][3]
    double *sums = nullptr;    // [cap_draws][K][3]: what a call returns
    float *tsum = nullptr;     // [Tl][K32]: the slab sum of the timing comparison (cmf_time_kernel "transconv1_sum")
    int64_t batch = 0;         // draws the tables above are sized for
    int64_t cap_draws = 0;
};

void signif_free(cmf_handle_s *h)
{
    if (!h->signif) return;
    SignifState *s = h->signif;
    if (s->tab) (void)hipFree(s->tab);
    if (s->partial) (void)hipFree(s->partial);
    if (s->sums) (void)hipFree(s->sums);
    if (s->tsum) (void)hipFree(s->tsum);
    delete s;
    h->signif = nullptr;
}

// draws per batch: option "signif_batch", else cmf_signif.h's default; never more than the 32-bit offsets of the operand loads take
// (the 32 lags of a lag block of the table stay below 2 GB).  0: not even one draw fits.
static int64_t signif_batch(const cmf_handle_s *h)
{
    const CmfDims &d = h->d;
    int64_t B = h->signif_batch > 0 ? h->signif_batch : cmfsig::default_batch(d.K);
    const int64_t lt = std::min<int64_t>(d.Lp, 32);
    const int64_t max_c32 = (((int64_t)1 << 31) - 1) / (lt * d.Np * 4) / 32 * 32;
    return std::min<int64_t>(B, max_c32 / d.K);
}

static int signif_ensure(cmf_handle_s *h, int64_t B, int64_t n_draws)
{
    const CmfDims &d = h->d;
    if (!h->signif) h->signif = new SignifState();
    SignifState *s = h->signif;
    if (s->batch < B) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (s->tab) (void)hipFree(s->tab);
        if (s->partial) (void)hipFree(s->partial);
        s->tab = nullptr; s->partial = nullptr; s->batch = 0;
        const size_t C32 = (size_t)rup(B * d.K, 32), TB = (size_t)(d.Tl + 127) / 128;
        CMFTRY(dalloc_zero(&s->tab, (size_t)d.Lp * d.Np * C32));
        CMFTRY(dalloc_zero(&s->partial, TB * C32 * 3));
        s->batch = B;
    }
    if (s->cap_draws < n_draws) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (s->sums) (void)hipFree(s->sums);
        s->sums = nullptr; s->cap_draws = 0;
        CMFTRY(dalloc_zero(&s->sums, (size_t)n_draws * d.K * 3));
        s->cap_draws = n_draws;
    }
    return CMF_OK;
}

// draws [d0, d0 + B) of the resident W against the raw data: shift table, contraction with the moments epilogue, sum over the t blocks
// into sums[(col0 + dl K + k) * 3 + .]
static int signif_run_batch(cmf_handle_s *h, uint64_t seed, int64_t d0, int64_t B, int64_t col0)
{
    const CmfDims &d = h->d;
    SignifState *s = h->signif;
    const int C32 = (int)rup(B * d.K, 32), TB = (d.Tl + 127) / 128;
    hipLaunchKernelGGL(signif_shift_kernel, dim3((C32 + 255) / 256, d.Np), dim3(256), 0, h->stream, s->tab, h->Wn, cmfsig::base(seed, CMF_SIGNIF_STREAM),
                       (long long)d0, (int)B, d.K, d.N, d.L, d.Lp, d.Np, d.K32, C32);
    KCHK("signif_shift_kernel");
    SgParams p;
    p.tab = s->tab; p.XT = h->XT; p.partial = s->partial;
    p.Np = d.Np; p.TP = d.TP; p.PADL = d.PADL; p.C32 = C32; p.CB = C32 / 32; p.L = d.L; p.Tl = d.Tl;
    p.C = (int)(rup(d.N, 8) / 8);
    p.pairs = TB * p.CB;
    p.W = (int)std::min<int64_t>(8LL * h->n_cu, p.pairs); // 2 workgroups of 4 waves per CU (transconv_kernel's residency)
    dim3 grid((p.W + 3) / 4), block(256);
    switch (h->tc_LT) {
#define CASE(LT_) case LT_: hipLaunchKernelGGL((signif_moments_kernel<LT_>), grid, block, 0, h->stream, p); break;
        CASE(4) CASE(8) CASE(12) CASE(16) CASE(20) CASE(24) CASE(28) CASE(32)
#undef CASE
    default: return fail(CMF_ERR_STATE, "internal: bad transconv LT %d", h->tc_LT);
    }
    KCHK("signif_moments_kernel");
    const int ncols = (int)(B * d.K);
    hipLaunchKernelGGL(signif_reduce_kernel, dim3((ncols + 255) / 256), dim3(256), 0, h->stream, s->partial, s->sums, ncols, C32, TB, (long long)col0);
    KCHK("signif_reduce_kernel");
    h->signif_launches += 3;
    return CMF_OK;
}

// what both entries ask of the handle, before any device work
static int signif_ready(cmf_handle_s *h, const char *what)
{
    if (h->group || h->root_only || h->sharded) return fail(CMF_ERR_UNSUPPORTED, "%s: single-GPU handles only", what);
    if (!h->factors_set) return fail(CMF_ERR_STATE, "factors not set: call cmf_set_factors first");
    if (!h->have_data) return fail(CMF_ERR_STATE, "handle was created without data");
    if (h->mu_mask || h->M)
        return fail(CMF_ERR_STATE, "%s: a mask is installed (held-out entries of the data may hold NaN); the test runs on a handle made of the held-out columns alone", what);
    const CmfDims &d = h->d;
    if (d.L > CMF_SIGNIF_MAX_L) return fail(CMF_ERR_UNSUPPORTED, "%s: L = %d is beyond %d", what, d.L, CMF_SIGNIF_MAX_L);
    // the last lag block's window of the last t block ends 32 ceil(L / 32) - 256 columns beyond a row of XT at most: that lands in the zero left
    // padding of the next row, which the last row of the allocation does not have
    const int64_t over = rup(d.Tl, 128) + 32LL * ((d.L + 31) / 32) - (rup(d.Tl, 512) + 256);
    if (over > 0 && rup(d.N, 8) >= d.Np) return fail(CMF_ERR_UNSUPPORTED, "%s: L = %d with N = %d (a multiple of 128 up to 7) is not supported", what, d.L, d.N);
    if (signif_batch(h) < 1) return fail(CMF_ERR_UNSUPPORTED, "%s: the null motifs of one draw (K = %d, N = %d) exceed the 2 GB a lag block may take", what, d.K, d.N);
    return CMF_OK;
}

int cmf_null_shifts(uint64_t seed, int64_t first_draw, int64_t n_draws, int64_t K, int64_t N, int64_t L, int32_t *shifts)
{
    if (cmfsig::null_shifts(seed, first_draw, n_draws, K, N, L, shifts))
        return fail(CMF_ERR_ARG, "cmf_null_shifts: shifts must not be NULL, n_draws, K, N >= 1, first_draw >= 0 and 1 <= L <= %d", CMF_SIGNIF_MAX_L);
    return CMF_OK;
}

int cmf_null_moments(cmf_handle h, uint64_t seed, int64_t first_draw, int64_t n_draws, double *sums)
{
    if (!h || !sums) return fail(CMF_ERR_ARG, "NULL argument");
    if (n_draws < 1 || first_draw < 0) return fail(CMF_ERR_ARG, "cmf_null_moments: n_draws must be at least 1 and first_draw at least 0");
    CMFTRY(signif_ready(h, "cmf_null_moments"));
    HIPCHK(hipSetDevice(h->device));
    const CmfDims &d = h->d;
    const int64_t B = signif_batch(h);
    CMFTRY(signif_ensure(h, std::min(B, n_draws), n_draws));
    for (int64_t j = 0; j < n_draws; j += B)
        CMFTRY(signif_run_batch(h, seed, first_draw + j, std::min(B, n_draws - j), j * d.K));
    HIPCHK(hipMemcpyAsync(sums, h->signif->sums, (size_t)n_draws * d.K * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CMF_OK;
}

// cmf_time_kernel "signif_draw": one default batch of null draws (shift table, contraction + moments, reduction), per DRAW;
// "transconv1_sum": the one-source C3 contraction of the rule plus its slab sum -- what one draw would cost through the rule's kernels.
int signif_time(cmf_handle_s *h, bool draws, int reps, double *avg_ms, double *flops)
{
    CMFTRY(signif_ready(h, "cmf_time_kernel"));
    const CmfDims &d = h->d;
    const int64_t B = signif_batch(h);
    CMFTRY(signif_ensure(h, B, B));
    SignifState *s = h->signif;
    if (!draws && !s->tsum) CMFTRY(dalloc_zero(&s->tsum, (size_t)d.Tl * d.K32));
    auto run = [&]() -> int {
        if (draws) return signif_run_batch(h, 0, 1, B, 0);
        CMFTRY(launch_transconv(h, 1, h->XT));
        return launch_slab_sum(h, s->tsum, h->hslabs, h->tc_S1, (size_t)d.Tl * d.K32);
    };
    CMFTRY(timed_reps(h->stream, h->ev0, h->ev1, reps, run, avg_ms));
    if (draws) *avg_ms /= (double)B;
    const double S = (double)d.L * d.Tl - 0.5 * (double)d.L * (d.L - 1);
    *flops = 2.0 * d.K * d.N * S;
    return CMF_OK;
}
