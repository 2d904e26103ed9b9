// cmf_recentre.hip -- seqNMF's re-centring of motifs on the resident factors (cmf_recentre.h has the definition and the decision):
// the kernels, the step the MU entries enqueue between the element-wise update of H and the loss conv (mult.jl:42-58: behind :51-52,
// in front of :55-57), and the entries cmf_recentre_shifts / cmf_recentre / cmf_mu_set_recentre / cmf_mu_recentre_info.
//
// One step is four launches on the handle's stream and nothing else -- no synchronisation, no copy to the host, no atomics:
//   recentre_mass_kernel    c_l[k] = sum_n Wn[l][n][k] in fp64, n ascending, one thread per (lag, component), 32 components side by side
//                           (a 128-byte line of Wn per step of n), and whether the lag holds an entry above the clamp floor
//   recentre_decide_kernel  m0, m1 over the lags in order, the decision of cmf_recentre.h -> the table of K shifts (it stays until the
//                           next step), |s_k| added to the running totals, and one word behind the table: is any shift non-zero
//   recentre_move_kernel    W in both layouts in place (a thread owns the lag column of one (k, n) and walks it away from the shift), H and
//                           Ht by column k's own shift into the step's scratch; vacated entries take the clamp floor
//   recentre_back_kernel    the moved columns of H and Ht from the scratch back into the handle's buffers (the parameter blocks, the
//                           write-back record and hals_snap hold those pointers: nothing is swapped)
// The last two read the table themselves and return at once while the word behind it is 0: a step whose shifts are all zero moves no
// data and leaves W and H bitwise untouched.  Only live entries are written (k < K, n < N, l < L, 0 <= t < Tl): every padding element keeps
// the exact zero the contraction kernels rely on.
#include "cmf_internal.h"
#include "cmf_recentre.h"

struct RecentreState {
    double *cl = nullptr;     // [K32][Lp]: the sums over n per (component, lag)
    int *live = nullptr;      // [K32][Lp]: the lag holds an entry above the floor
    int32_t *shifts = nullptr; // [K32 + 1]: s_k of the last step | any of them non-zero
    long long *moved = nullptr; // [K32]: sum of |s_k| since the handle was made
    float *sH = nullptr, *sHt = nullptr; // [Tl][K32], [K32][Tl]
};

void recentre_free(cmf_handle_s *h)
{
    if (!h->rc) return;
    RecentreState *r = h->rc;
    for (void *p : {(void *)r->cl, (void *)r->live, (void *)r->shifts, (void *)r->moved, (void *)r->sH, (void *)r->sHt})
        if (p) (void)hipFree(p);
    delete r;
    h->rc = nullptr;
}

static int recentre_ensure(cmf_handle_s *h)
{
    if (h->rc) return CMF_OK;
    const CmfDims &d = h->d;
    RecentreState *r = h->rc = new RecentreState();
    CMFTRY(dalloc_zero(&r->cl, (size_t)d.K32 * d.Lp));
    CMFTRY(dalloc_zero(&r->live, (size_t)d.K32 * d.Lp));
    CMFTRY(dalloc_zero(&r->shifts, (size_t)d.K32 + 1));
    CMFTRY(dalloc_zero(&r->moved, (size_t)d.K32));
    CMFTRY(dalloc_zero(&r->sH, (size_t)d.Tl * d.K32));
    CMFTRY(dalloc_zero(&r->sHt, (size_t)d.K32 * d.Tl));
    return CMF_OK;
}

static __global__ __launch_bounds__(256) void recentre_mass_kernel(const float *__restrict__ Wn, double *__restrict__ cl, int *__restrict__ live, int N, int K, int L,
                                                                   int Lp, int Np, int K32)
{
    const int k = blockIdx.x * 32 + threadIdx.x, l = blockIdx.y * 8 + threadIdx.y;
    if (k >= K || l >= L) return;
    const float *p = Wn + (size_t)l * Np * K32 + k;
    double c = 0.0;
    float top = 0.f;
#pragma unroll 8
    for (int n = 0; n < N; ++n) {
        const float w = p[(size_t)n * K32];
        c += (double)w;
        top = fmaxf(top, w);
    }
    cl[(size_t)k * Lp + l] = c;
    live[(size_t)k * Lp + l] = top > CMF_EPS_F ? 1 : 0;
}

static __global__ __launch_bounds__(256) void recentre_decide_kernel(const double *__restrict__ cl, const int *__restrict__ live, int32_t *__restrict__ shifts,
                                                                     long long *__restrict__ moved, int K, int L, int Lp, int K32)
{
    int any = 0;
    for (int k = threadIdx.x; k < K32; k += 256) {
        int32_t s = 0;
        if (k < K) {
            cmfrc::Mass m;
            for (int l = 0; l < L; ++l) cmfrc::add_lag(m, l, cl[(size_t)k * Lp + l], live[(size_t)k * Lp + l] != 0);
            s = cmfrc::decide(m, L);
            moved[k] += s < 0 ? -(long long)s : (long long)s;
        }
        shifts[k] = s;
        any |= s != 0;
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) shifts[K32] = any;
}

// blockIdx.y: 0 H -> sH, 1 Ht -> sHt, 2 Wt in place, 3 Wn in place
static __global__ __launch_bounds__(256) void recentre_move_kernel(float *__restrict__ H, float *__restrict__ Ht, float *__restrict__ Wt, float *__restrict__ Wn,
                                                                   float *__restrict__ sH, float *__restrict__ sHt, const int32_t *__restrict__ shifts, int N, int Tl,
                                                                   int K, int L, int Np, int K32, int TP, int PADL)
{
    if (!shifts[K32]) return;
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int job = blockIdx.y;
    if (job == 0) {
        for (size_t i = first; i < (size_t)Tl * K32; i += stride) {
            const int t = (int)(i / K32), k = (int)(i - (size_t)t * K32);
            const long long s = k < K ? shifts[k] : 0, src = t + s;
            if (s) sH[i] = (src >= 0 && src < Tl) ? H[(size_t)(PADL + src) * K32 + k] : CMF_EPS_F;
        }
    } else if (job == 1) {
        for (size_t i = first; i < (size_t)K * Tl; i += stride) {
            const int k = (int)(i / Tl), t = (int)(i - (size_t)k * Tl);
            const long long s = shifts[k], src = t + s;
            if (s) sHt[i] = (src >= 0 && src < Tl) ? Ht[(size_t)k * TP + PADL + src] : CMF_EPS_F;
        }
    } else {
        const bool wt = job == 2; // Wt[l][k][n]: n along the threads; Wn[l][n][k]: k along the threads
        const size_t lag = (size_t)Np * K32, count = wt ? (size_t)K * Np : (size_t)Np * K32;
        for (size_t i = first; i < count; i += stride) {
            const int k = wt ? (int)(i / Np) : (int)(i % K32), n = wt ? (int)(i % Np) : (int)(i / K32);
            if (k >= K || n >= N) continue;
            const long long s = shifts[k];
            if (!s) continue;
            float *p = (wt ? Wt : Wn) + (wt ? (size_t)k * Np + n : (size_t)n * K32 + k);
            if (s > 0)
                for (long long l = L - 1; l >= 0; --l) p[l * lag] = l - s >= 0 ? p[(l - s) * lag] : CMF_EPS_F;
            else
                for (long long l = 0; l < L; ++l) p[l * lag] = l - s < L ? p[(l - s) * lag] : CMF_EPS_F;
        }
    }
}

// blockIdx.y: 0 sH -> H, 1 sHt -> Ht
static __global__ __launch_bounds__(256) void recentre_back_kernel(float *__restrict__ H, float *__restrict__ Ht, const float *__restrict__ sH, const float *__restrict__ sHt,
                                                                   const int32_t *__restrict__ shifts, int Tl, int K, int K32, int TP, int PADL)
{
    if (!shifts[K32]) return;
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.y == 0) {
        for (size_t i = first; i < (size_t)Tl * K32; i += stride) {
            const int t = (int)(i / K32), k = (int)(i - (size_t)t * K32);
            if (k < K && shifts[k]) H[(size_t)(PADL + t) * K32 + k] = sH[i];
        }
    } else {
        for (size_t i = first; i < (size_t)K * Tl; i += stride) {
            const int k = (int)(i / Tl), t = (int)(i - (size_t)k * Tl);
            if (shifts[k]) Ht[(size_t)k * TP + PADL + t] = sHt[i];
        }
    }
}

// One step on the resident factors, enqueued on the handle's stream.  Every writer of the factors passes through set_est: the
// few-component pack sk_Wj and the x-ortho table G are stale behind it, est is void.
int recentre_step(cmf_handle_s *h)
{
    CMFTRY(recentre_ensure(h));
    RecentreState *r = h->rc;
    const CmfDims &d = h->d;
    hipLaunchKernelGGL(recentre_mass_kernel, dim3(d.KB, (d.L + 7) / 8), dim3(32, 8), 0, h->stream, h->Wn, r->cl, r->live, d.N, d.K, d.L, d.Lp, d.Np, d.K32);
    KCHK("recentre_mass_kernel");
    hipLaunchKernelGGL(recentre_decide_kernel, dim3(1), dim3(256), 0, h->stream, r->cl, r->live, r->shifts, r->moved, d.K, d.L, d.Lp, d.K32);
    KCHK("recentre_decide_kernel");
    const size_t most = std::max((size_t)d.Tl, (size_t)d.Np) * d.K32;
    const unsigned gx = (unsigned)std::min<size_t>(2048, (most + 255) / 256);
    hipLaunchKernelGGL(recentre_move_kernel, dim3(gx, 4), dim3(256), 0, h->stream, h->H, h->Ht, h->Wt, h->Wn, r->sH, r->sHt, r->shifts, d.N, d.Tl, d.K, d.L, d.Np,
                       d.K32, d.TP, d.PADL);
    KCHK("recentre_move_kernel");
    hipLaunchKernelGGL(recentre_back_kernel, dim3(gx, 2), dim3(256), 0, h->stream, h->H, h->Ht, r->sH, r->sHt, r->shifts, d.Tl, d.K, d.K32, d.TP, d.PADL);
    KCHK("recentre_back_kernel");
    h->recentre_launches += 4;
    set_est(h, EST_NONE);
    return CMF_OK;
}

// what the handle entries ask, before any device work
static int recentre_single(const cmf_handle_s *h, const char *what)
{
    if (h->group || h->root_only || h->sharded)
        return fail(CMF_ERR_UNSUPPORTED, "%s: single-GPU handles only (a shift of H crosses the borders of the shards of a T-sharded group)", what);
    return CMF_OK;
}

int cmf_recentre_shifts(const double *W, int64_t K, int64_t N, int64_t L, int32_t *shifts)
{
    if (cmfrc::shifts(W, K, N, L, shifts)) return fail(CMF_ERR_ARG, "cmf_recentre_shifts: W and shifts must not be NULL, K, N, L >= 1");
    return CMF_OK;
}

int cmf_recentre(cmf_handle h, int32_t *shifts)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    CMFTRY(recentre_single(h, "cmf_recentre"));
    if (!h->factors_set) return fail(CMF_ERR_STATE, "factors not set: call cmf_set_factors first");
    HIPCHK(hipSetDevice(h->device));
    if (h->wb && h->wb->armed) wb_disarm(h); // (a W copy in flight would deliver the factor this call moves)
    h->carry = CmfLossCarry{};
    CMFTRY(recentre_step(h));
    if (!shifts) return CMF_OK;
    HIPCHK(hipMemcpyAsync(shifts, h->rc->shifts, (size_t)h->d.K * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CMF_OK;
}

int cmf_mu_set_recentre(cmf_handle h, int on)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    if (on != 0 && on != 1) return fail(CMF_ERR_ARG, "cmf_mu_set_recentre: on must be 0 or 1");
    CMFTRY(recentre_single(h, "cmf_mu_set_recentre"));
    if (on && h->gram)
        return fail(CMF_ERR_UNSUPPORTED, "the Gram forms (option \"gram\") keep tables of W across the H phase that a shift of W would leave stale: set gram = 0 first");
    h->mu_recentre = on;
    return CMF_OK;
}

int cmf_mu_recentre_info(cmf_handle h, int32_t *last_shifts, int64_t *moved)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    CMFTRY(recentre_single(h, "cmf_mu_recentre_info"));
    const size_t K = (size_t)h->d.K;
    if (!h->rc) { // no step yet
        if (last_shifts) std::memset(last_shifts, 0, K * sizeof(int32_t));
        if (moved) std::memset(moved, 0, K * sizeof(int64_t));
        return CMF_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    static_assert(sizeof(long long) == sizeof(int64_t), "moved is copied as it lies");
    if (last_shifts) HIPCHK(hipMemcpyAsync(last_shifts, h->rc->shifts, K * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (moved) HIPCHK(hipMemcpyAsync(moved, h->rc->moved, K * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CMF_OK;
}
