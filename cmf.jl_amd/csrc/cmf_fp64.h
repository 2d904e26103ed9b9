#pragma once
// cmf_fp64.h -- what the fp64 rules (ADMM: cmf_admm.h / cmf_admm.hip, ANLS: cmf_anls.h / cmf_anls.hip) share: the contraction
// kernel with the loaders and epilogues both of them use, the fixed-order sum of its loss partials, and the host side of a rule's
// state (dimensions, the data, the factor a call reads, the loss buffers).  Included after cmf_internal.h.
//
//   fp64_gemm_kernel     the contractions: C[m, p] = sum_r A(m, r) B(r, p) for element loaders A, B that address the factors in
//                        place (the stacked Hstk of common.jl:133-142, the lagged H and data columns), with a fused element-wise
//                        epilogue (a store, the updates of a rule, squared residuals of the loss).  64 x 64 tiles, 4 x 4 per thread.
//   fp64_sum_kernel      the loss partials of a contraction, summed in a fixed order
// A loader or epilogue that one rule alone uses is in that rule's header.
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fp64 {

constexpr int TM = 64, TP = 64, TR = 16;

// ---- element loaders (A: m x r, B: r x p) --------------------------------------------------------------------------------------
// Hstk[i, t] = H[k, t - l] (i = l*K + k, zero for t < l); H is row-major [k][t] on the device
struct HstkRT { // A(i, t): m = stacked row, r = time
    const double *H; int K, T;
    __device__ double operator()(int64_t i, int64_t t) const { int l = (int)(i / K), k = (int)(i % K); return t >= l ? H[(int64_t)k * T + t - l] : 0.0; }
};
struct HstkTR { // A(t, i) or B(t, j) with the stacked row as the second index
    const double *H; int K, T;
    __device__ double operator()(int64_t t, int64_t i) const { int l = (int)(i / K), k = (int)(i % K); return t >= l ? H[(int64_t)k * T + t - l] : 0.0; }
};
struct RowMajor { // M[r][p] with row stride ld
    const double *X; int64_t ld;
    __device__ double operator()(int64_t r, int64_t p) const { return X[r * ld + p]; }
};
// W in Julia's layout W[k + K*(n + N*l)]
struct WkR { // A(k, r) with r = n + N*l
    const double *W; int K;
    __device__ double operator()(int64_t k, int64_t r) const { return W[k + (int64_t)K * r]; }
};
struct WnR { // A(n, r) with r = k + K*l
    const double *W; int K, N;
    __device__ double operator()(int64_t n, int64_t r) const { int l = (int)(r / K), k = (int)(r % K); return W[k + (int64_t)K * (n + (int64_t)N * l)]; }
};

// ---- epilogues: called once per output element; the return value is added to the loss partial ---------------------------------
struct EpiStore { // C[m][p] (row stride ld) = acc + (diag ? add_diag : 0)
    double *C; int64_t ld; double add_diag;
    __device__ double operator()(int64_t m, int64_t p, double acc) const { C[m * ld + p] = acc + (m == p ? add_diag : 0.0); return 0.0; }
};
struct EpiLossN { // (acc - data[n, t])^2   (admm.jl:199-200, 225; anls.jl:35)
    const double *data; int64_t N;
    __device__ double operator()(int64_t n, int64_t t, double acc) const { double r = acc - data[t * N + n]; return r * r; }
};

// A_MFAST / B_PFAST: which index of the loader is contiguous in memory, so that a wave's tile loads run along it
template <class AL, class BL, class EP, bool A_MFAST, bool B_PFAST>
static __global__ __launch_bounds__(256) void fp64_gemm_kernel(AL A, BL B, EP E, int64_t M, int64_t P, int64_t R, double *partial)
{
    __shared__ double As[TR][TM + 1];
    __shared__ double Bs[TR][TP + 1];
    __shared__ double red[256];
    const int tid = threadIdx.x, tm = tid % 16, tp = tid / 16;
    const int64_t m0 = (int64_t)blockIdx.x * TM, p0 = (int64_t)blockIdx.y * TP;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int64_t r0 = 0; r0 < R; r0 += TR) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q;
            const int mm = A_MFAST ? idx % TM : idx / TR, ra = A_MFAST ? idx / TM : idx % TR;
            As[ra][mm] = (m0 + mm < M && r0 + ra < R) ? A(m0 + mm, r0 + ra) : 0.0;
            const int pp = B_PFAST ? idx % TP : idx / TR, rb = B_PFAST ? idx / TP : idx % TR;
            Bs[rb][pp] = (p0 + pp < P && r0 + rb < R) ? B(r0 + rb, p0 + pp) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < TR; ++rr) {
            double av[4], bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { av[q] = As[rr][tm + 16 * q]; bv[q] = Bs[rr][tp + 16 * q]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }
    double part = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t m = m0 + tm + 16 * a, p = p0 + tp + 16 * b;
            if (m < M && p < P) part += E(m, p, acc[a][b]);
        }
    if (partial) {
        red[tid] = part;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
    }
}

// sum of n partials into out[0], one workgroup, fixed order (deterministic)
static __global__ __launch_bounds__(256) void fp64_sum_kernel(const double *partial, int64_t n, double *out)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// `rule` is "ADMM" or "ANLS": the word a message names the calling rule by.
struct Fp64State { // AdmmState and AnlsState derive from it
    int64_t N = 0, T = 0, K = 0, L = 0, LK = 0;
    double datanorm = 0.0;
    double *data = nullptr;                      // N x T, data[n + N*t] (= data' row-major)
    double *Hd = nullptr;                        // K x T: the H a call reads (or, in the ANLS H step, updates in place)
    double *Wd = nullptr;                        // K x N x L, Julia's layout: the W the H call reads
    double *partial = nullptr, *dsum = nullptr;  // the loss partials of a contraction (npartial of them) and their sum
    int64_t npartial = 0;
    std::vector<void *> owned;                   // everything fp64_alloc handed out
};

template <typename T>
static int fp64_alloc(Fp64State *s, T **p, size_t n)
{
    HIPCHK(hipMalloc(p, std::max<size_t>(n, 1) * sizeof(T)));
    s->owned.push_back(*p);
    return CMF_OK;
}

// frees what fp64_alloc handed out, after the handle's stream has drained (a rule's pinned host memory is its own to free)
static void fp64_release(cmf_handle_s *h, Fp64State *s)
{
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (void *p : s->owned) (void)hipFree(p);
}

static int64_t blocks(int64_t n, int64_t b) { return (n + b - 1) / b; }

// loss: the squared residuals the epilogue returns are summed into s->dsum
template <bool AMF, bool BPF, class AL, class BL, class EP>
static int fp64_gemm(Fp64State *s, hipStream_t st, const char *rule, AL a, BL b, EP e, int64_t M, int64_t P, int64_t R, bool loss)
{
    const dim3 grid((unsigned)blocks(M, TM), (unsigned)blocks(P, TP));
    if (grid.y > 65535) return fail(CMF_ERR_UNSUPPORTED, "%s: a contraction of %lld columns is beyond one launch", rule, (long long)P);
    if (loss && (int64_t)grid.x * grid.y > s->npartial) return fail(CMF_ERR_STATE, "internal: %s loss partial buffer too small", rule);
    hipLaunchKernelGGL((fp64_gemm_kernel<AL, BL, EP, AMF, BPF>), grid, dim3(256), 0, st, a, b, e, M, P, R, loss ? s->partial : nullptr);
    KCHK("fp64_gemm_kernel");
    if (loss) {
        hipLaunchKernelGGL(fp64_sum_kernel, dim3(1), dim3(256), 0, st, s->partial, (int64_t)grid.x * grid.y, s->dsum);
        KCHK("fp64_sum_kernel");
    }
    return CMF_OK;
}

// the refusal of a handle that fronts a T-sharded group, in the words of cmf_*_prepare (which names the limit) or of an update entry
static int fp64_single_gpu(const cmf_handle_s *h, const char *rule, bool prepare)
{
    if (!h->group && !h->root_only && !h->sharded) return CMF_OK;
    if (prepare)
        return fail(CMF_ERR_UNSUPPORTED, "the %s rule runs on a single-GPU handle of at most %lld columns only (this one fronts a T-sharded "
                                         "group: cmf_create_multi / cmf_create_shard, or cmf_create of a longer recording)", rule, (long long)65535 * TP);
    return fail(CMF_ERR_UNSUPPORTED, "the %s rule runs on a single-GPU handle only (this one fronts a T-sharded group)", rule);
}

// cmf_*_prepare on a fresh state, after the rule's refusals: the dimensions, the buffers above, norm(data) and the upload of data
// (admm.jl:13-21, anls.jl:10-14: the constructor keeps norm(data))
static int fp64_prepare_common(const cmf_handle_s *h, Fp64State *s, const double *data)
{
    s->N = h->d.N; s->T = h->d.Tl; s->K = h->d.K; s->L = h->d.L; s->LK = s->L * s->K;
    s->npartial = blocks(s->T, 64) * blocks(s->N, 64);
    const size_t NT = (size_t)s->N * s->T;
    CMFTRY(fp64_alloc(s, &s->data, NT));
    CMFTRY(fp64_alloc(s, &s->Hd, (size_t)s->K * s->T));
    CMFTRY(fp64_alloc(s, &s->Wd, (size_t)s->K * s->N * s->L));
    CMFTRY(fp64_alloc(s, &s->partial, (size_t)s->npartial));
    CMFTRY(fp64_alloc(s, &s->dsum, 1));
    double ss = 0.0;
    for (size_t i = 0; i < NT; ++i) ss += data[i] * data[i];
    s->datanorm = std::sqrt(ss);
    if (hipMemcpy(s->data, data, NT * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(CMF_ERR_HIP, "data upload failed");
    return CMF_OK;
}

// H (K x T, Julia's layout H[k + K*t]) -> s->Hd as [k][t]; Hr is the staging copy and outlives the call's stream work
static int fp64_upload_H_rows(Fp64State *s, hipStream_t st, const double *H, std::vector<double> &Hr)
{
    const int64_t K = s->K, T = s->T;
    Hr.resize((size_t)K * T);
    for (int64_t t = 0; t < T; ++t)
        for (int64_t k = 0; k < K; ++k) Hr[(size_t)k * T + t] = H[k + K * t];
    HIPCHK(hipMemcpyAsync(s->Hd, Hr.data(), Hr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    return CMF_OK;
}

// fold (admm.jl:114-120; anls.jl:56, :150-157): W[k, n, l] = X[l*K + k, n], X as [i][n]
static void fp64_fold_W(const double *X, double *W, int64_t K, int64_t N, int64_t L)
{
    for (int64_t l = 0; l < L; ++l)
        for (int64_t n = 0; n < N; ++n)
            for (int64_t k = 0; k < K; ++k) W[k + K * (n + N * l)] = X[(size_t)(l * K + k) * N + n];
}

} // namespace fp64
