// cmf_xortho.h -- the small kernels of seqNMF's cross-orthogonality penalties on the MU rule (cmf_mu_set_xortho).
//
//   S(A)[k][t]   = sum of A[k][t'] over |t' - t| <= L - 1, 0 <= t' < T        (box of width 2L - 1, cut at both ends of the recording)
//   off(A)[k][.] = sum of A[k'][.] over k' != k                               (the OTHER components)
//   G = off(S(H));  xH = off(S(numH));  oW[k][n] = off(Wflat)[k][n],  Wflat[k][n] = sum_l W[k][n][l]
//
// Every sum here adds non-negative terms only, in a fixed order: no difference of running sums (total - own, a sliding window, prefix
// differences) -- beside a component of order 1 a dead one at eps would get rounding noise of either sign where the true value is
// 1e-15, and a negative denominator term with it.  S is a direct window sum out of LDS, off an exclusive prefix plus an exclusive suffix.
// The tables are [rows][K32] with k fastest (the layout of H without its row padding); the weights are wave-uniform arguments.
#pragma once
#include <hip/hip_runtime.h>

#define XO_WIN_T 64    // columns of a window workgroup
#define XO_WIN_CH 128  // rows staged per pass
#define XO_OFF_T 256   // columns of an off workgroup
#define XO_NPART 1024  // fp64 partials of a cost sum

// out[t][k] = S(in)[t][k] for t in [0, Tl): grid (ceil(Tl / 64), KB), block 256 = 32 k x 8 groups of 8 adjacent columns.  The rows
// [t0 - (L-1), t0 + 63 + (L-1)] pass through LDS 128 at a time (rows outside the recording as zeros); a thread adds the rows of its
// window in ascending order.
static __global__ __launch_bounds__(256) void xo_window_kernel(const float *in, float *out, int Tl, int K32, int L)
{
    __shared__ float tile[XO_WIN_CH][33];
    const int tid = threadIdx.x, kk = tid & 31, tq = tid >> 5;
    const int t0 = blockIdx.x * XO_WIN_T, kb = blockIdx.y;
    const int hw = L - 1;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const int r_first = t0 - hw, r_last = t0 + XO_WIN_T - 1 + hw;
    for (int c0 = r_first; c0 <= r_last; c0 += XO_WIN_CH) {
#pragma unroll
        for (int q = 0; q < XO_WIN_CH / 8; ++q) {
            const int row = c0 + tq + 8 * q;
            tile[tq + 8 * q][kk] = (row >= 0 && row < Tl) ? in[(size_t)row * K32 + kb * 32 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = t0 + 8 * tq + j;
            const int lo = max(c0, t - hw), hi = min(c0 + XO_WIN_CH - 1, t + hw);
            float a = acc[j];
            for (int r = lo; r <= hi; ++r) a += tile[r - c0][kk];
            acc[j] = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int t = t0 + 8 * tq + j;
        if (t < Tl) out[(size_t)t * K32 + kb * 32 + kk] = acc[j];
    }
}

// off over ALL K components (across the 32-wide k blocks) of the rows of in: grid ceil(Tl / 256), block 256, a thread per row.
//   base == NULL:  out[t][k] = off(in)[t][k]
//   base != NULL:  out[t][k] = base[t][k] + (lam * off(in)[t][k] + lam2 * g[t][k])       (the finished denominator of H)
// Columns k >= K get an exact 0.  outT (may be NULL): the transposed copy outT[k * TP + t] as well (G in the layout of Ht).
// First pass, k blocks ascending: the exclusive prefix into out.  Second pass, descending: the exclusive suffix is added.
static __global__ __launch_bounds__(256) void xo_off_kernel(const float *in, float *out, float *outT, int TP, int Tl, int K, int K32, const float *base,
                                                            const float *g, float lam, float lam2)
{
    __shared__ float tile[XO_OFF_T][33];
    const int tid = threadIdx.x, kk = tid & 31, tq = tid >> 5;
    const int t0 = blockIdx.x * XO_OFF_T;
    const int KB = K32 / 32;
    float run = 0.f;
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll 4
        for (int q = 0; q < XO_OFF_T / 8; ++q) {
            const int t = t0 + tq + 8 * q;
            tile[tq + 8 * q][kk] = (t < Tl && kb * 32 + kk < K) ? in[(size_t)t * K32 + kb * 32 + kk] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < 32; ++c) {
            const float v = tile[tid][c];
            tile[tid][c] = run;
            run += v;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < XO_OFF_T / 8; ++q) {
            const int t = t0 + tq + 8 * q;
            if (t < Tl) out[(size_t)t * K32 + kb * 32 + kk] = tile[tq + 8 * q][kk];
        }
        __syncthreads();
    }
    run = 0.f;
    for (int kb = KB - 1; kb >= 0; --kb) {
#pragma unroll 4
        for (int q = 0; q < XO_OFF_T / 8; ++q) {
            const int t = t0 + tq + 8 * q;
            tile[tq + 8 * q][kk] = (t < Tl && kb * 32 + kk < K) ? in[(size_t)t * K32 + kb * 32 + kk] : 0.f;
        }
        __syncthreads();
        for (int c = 31; c >= 0; --c) {
            const float v = tile[tid][c];
            tile[tid][c] = run;
            run += v;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < XO_OFF_T / 8; ++q) {
            const int t = t0 + tq + 8 * q, k = kb * 32 + kk;
            if (t < Tl) {
                const size_t idx = (size_t)t * K32 + k;
                float o = out[idx] + tile[tq + 8 * q][kk]; // prefix + suffix
                if (base) o = base[idx] + (lam * o + lam2 * g[idx]);
                if (k >= K) o = 0.f;
                out[idx] = o;
                tile[tq + 8 * q][kk] = o;
            }
        }
        if (outT) {
            __syncthreads();
            if (t0 + tid < Tl)
                for (int c = 0; c < 32; ++c) outT[(size_t)(kb * 32 + c) * TP + t0 + tid] = tile[tid][c];
        }
        __syncthreads();
    }
}

// Wf[k][n] = sum_l Wt[l][k][n]: grid (Np / 128, K), block 128.  Lags in ascending order.
static __global__ __launch_bounds__(128) void xo_wflat_kernel(const float *Wt, float *Wf, int L, int K32, int Np)
{
    const int n = blockIdx.x * 128 + threadIdx.x, k = blockIdx.y;
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += Wt[((size_t)l * K32 + k) * Np + n];
    Wf[(size_t)k * Np + n] = s;
}

// oW[k][n] = off(Wf)[k][n] over k < K (rows k >= K and columns n >= N stay the zeros they were allocated as: W is zero there):
// grid Np / 128, block 128, a thread per n; exclusive prefix ascending, exclusive suffix descending.
static __global__ __launch_bounds__(128) void xo_off_w_kernel(const float *Wf, float *oW, int K, int Np)
{
    const int n = blockIdx.x * 128 + threadIdx.x;
    float run = 0.f;
    for (int k = 0; k < K; ++k) {
        oW[(size_t)k * Np + n] = run;
        run += Wf[(size_t)k * Np + n];
    }
    run = 0.f;
    for (int k = K - 1; k >= 0; --k) {
        oW[(size_t)k * Np + n] += run;
        run += Wf[(size_t)k * Np + n];
    }
}

// denomW[l][k][n] += lam * xW[l][k][n] + lamW * oW[k][n]   (float4 lanes; KN4 = K32 * Np / 4, n4 = L * KN4)
static __global__ __launch_bounds__(256) void xo_fold_w_kernel(float *den, const float *xW, const float *oW, size_t n4, size_t KN4, float lam, float lamW)
{
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < n4; idx += (size_t)gridDim.x * blockDim.x) {
        float4 d = reinterpret_cast<float4 *>(den)[idx];
        const float4 x = reinterpret_cast<const float4 *>(xW)[idx];
        const float4 o = reinterpret_cast<const float4 *>(oW)[idx % KN4];
        d.x += lam * x.x + lamW * o.x; d.y += lam * x.y + lamW * o.y;
        d.z += lam * x.z + lamW * o.z; d.w += lam * x.w + lamW * o.w;
        reinterpret_cast<float4 *>(den)[idx] = d;
    }
}

// partial[b] = sum over block b's share of a[i] * b[i] in fp64 (grid XO_NPART or fewer; the host adds the partials in order)
static __global__ __launch_bounds__(256) void xo_dot_kernel(const float *a, const float *b, size_t n, double *partial)
{
    __shared__ double red[256];
    double s = 0.0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += (double)a[i] * (double)b[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
