#pragma once
// cmf_sep.h -- gfx950 kernels of the separable fit (src/algs/separable.jl), all in fp64.
//
// Successive projection (SPA, separable.jl:280-319).  The residual is kept column by column, X[t*M + m] (M = N, or R after
// `pre`), and a round is two kernels on one stream; the host reads nothing until the R vertices are found:
//   sep_select_kernel    findsetmax (:403-419) and the col2 tie-break (:306-311) of one round, ONE workgroup.  The sequential
//                        scan is replaced by its exact parallel form: the anchor can only move at a strict prefix-maximum
//                        record (the running maximum never exceeds anchor + thresh), so the records are listed by a chunked
//                        prefix-max scan, one lane walks that short list to the final anchor (a, i_a), the set is
//                        {i_a} u {i > i_a : x[i] > a - thresh} and the vertex is the first maximum of col2 over it.  Leaves
//                        the vertex, w = resid[:, j] and norm(w)^2 in device memory for the next kernel.
//   sep_project_kernel   resid[:, t] -= w (w' resid[:, t] / |w|^2) (:315 without the N x N projector) fused with the column norm
//                        of the result, which is recomputed, never downdated.  A group of G = 8..64 lanes owns a column (a
//                        wave holds 64/G consecutive columns, so the loads of a wave are contiguous), w sits in LDS, the two
//                        sums of a column run in a fixed order (strided partial sums, then a butterfly): bit-repeatable.
//   sep_scale_kernel     :281-291: col1, col2, X = data * inv(DX), the columns below `thresh` zeroed
// Step 2 (:26-27) is anls_nnls_w_kernel of cmf_anls.h on V'V and V'data, then sep_rowsum_kernel / sep_rescale_kernel
// (renormalize!, :340-348).  The shift cosines (:364-385) come from
//   sep_lag_kernel       P[a, b, l] = sum_t G[a, t] G[b, t+l] as one 64 x 64-tiled contraction over (a, (b, l)) whose T range is
//                        split over blockIdx.z; sep_lag_sum_kernel adds the splits in the order of z (fixed)
//   sep_rowsum_kernel    head[a, l] = |G[a, 0 : T-l]|, summed directly over its T - l entries (and the row sums of renormalize!)
#include <hip/hip_runtime.h>
#include <cstdint>
#include "cmf_fp64.h"

namespace sep {

constexpr int MMAX = 4096;    // rows of the SPA residual: w is held in LDS (32 KB)
constexpr int SEL = 1024;     // threads of sep_select_kernel (one workgroup)
constexpr int COLS_IT = 4;    // columns a lane group walks in sep_project_kernel / sep_scale_kernel
constexpr double DBL_EPS = 2.220446049250313e-16;
enum { FL_ZERO_W = 0, FL_N = 1 }; // flags of a SPA call in device memory: rounds whose residual had vanished

// X[p*ld + r] as a loader of fp64_gemm_kernel: A(m, r) = X[r*ld + m], B(r, p) = X[p*ld + r]
struct ColMajor {
    const double *X; int64_t ld;
    __device__ double operator()(int64_t r, int64_t p) const { return X[p * ld + r]; }
};

// sum over the G lanes of a group (G a power of two <= 64), the same value in all of them, in a fixed order
__device__ inline double group_sum(double v, int G)
{
    for (int s = G >> 1; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// the column a lane group works on in iteration `it`: consecutive groups of consecutive waves take consecutive columns
__device__ inline int64_t group_column(int G, int it)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cpw = 64 / G;
    return (((int64_t)blockIdx.x * COLS_IT + it) * 4 + wave) * cpw + lane / G;
}

static __global__ __launch_bounds__(256) void sep_scale_kernel(const double *data, double *X, double *col1, double *col2, int N, int64_t T, double thresh, int G)
{
    const int sl = (threadIdx.x & 63) % G;
    for (int it = 0; it < COLS_IT; ++it) {
        const int64_t t = group_column(G, it);
        const bool live = t < T;
        const double *x = data + (live ? t : 0) * N;
        double s1 = 0.0, s2 = 0.0;
        if (live)
            for (int n = sl; n < N; n += G) { const double v = x[n]; s1 += fabs(v); s2 = fma(v, v, s2); }
        s1 = group_sum(s1, G);
        s2 = group_sum(s2, G);
        if (!live) continue;
        const double inv = 1.0 / (s1 + (s1 < DBL_EPS ? 1.0 : 0.0)); // inv(diagscale(col1)), :283-284, :389-391
        const bool drop = s1 < thresh;                               // :287-291
        for (int n = sl; n < N; n += G) X[t * N + n] = drop ? 0.0 : x[n] * inv;
        if (sl == 0) { col1[t] = s1; col2[t] = sqrt(s2); }
    }
}

// wbuf: w (M doubles), then norm(w)^2.  project = 0: the norms only (the first round).
static __global__ __launch_bounds__(256) void sep_project_kernel(double *X, int M, int64_t T, const double *wbuf, double *norms, int G, int project)
{
    extern __shared__ double ws[];
    if (project)
        for (int m = threadIdx.x; m < M; m += 256) ws[m] = wbuf[m];
    __syncthreads();
    const double wn2 = project ? wbuf[M] : 1.0;
    const int sl = (threadIdx.x & 63) % G;
    for (int it = 0; it < COLS_IT; ++it) {
        const int64_t t = group_column(G, it);
        const bool live = t < T;
        double *x = X + (live ? t : 0) * M;
        double c = 0.0;
        if (project) {
            double dot = 0.0;
            if (live)
                for (int m = sl; m < M; m += G) dot = fma(ws[m], x[m], dot);
            c = group_sum(dot, G) / wn2;
        }
        double ss = 0.0;
        if (live)
            for (int m = sl; m < M; m += G) {
                double v = x[m]; // (a second read of the column: it has just passed through the cache)
                if (project) { v = fma(-ws[m], c, v); x[m] = v; }
                ss = fma(v, v, ss);
            }
        ss = group_sum(ss, G);
        if (live && sl == 0) norms[t] = sqrt(ss);
    }
}

// better(a, b): candidate a = (col2, index) comes before b in "the first maximum of col2"
__device__ inline bool first_max(double va, int64_t ia, double vb, int64_t ib) { return ib < 0 || (ia >= 0 && (va > vb || (va == vb && ia < ib))); }

// One round's choice (see the head of the file).  x: T column norms; rec: T ints of scratch; vertices[round] receives j.
static __global__ __launch_bounds__(SEL) void sep_select_kernel(const double *x, const double *col2, int64_t T, const double *X, int M, double thresh, int round,
                                                               int64_t *vertices, double *wbuf, int *rec, unsigned long long *flags)
{
    __shared__ double cmax[SEL], bval[SEL], s_a;
    __shared__ int cnt[SEL];
    __shared__ int64_t bidx[SEL], s_ia;
    const int tid = threadIdx.x;
    const int64_t len = (T + SEL - 1) / SEL, lo = tid * len, hi = lo + len < T ? lo + len : T;
    // records: x[i] > max(x[0..i-1]); element 0 is the scan's first anchor
    double m = -INFINITY;
    for (int64_t i = lo; i < hi; ++i) m = fmax(m, x[i]);
    cmax[tid] = m;
    __syncthreads();
    double before = -INFINITY;
    for (int c = 0; c < tid; ++c) before = fmax(before, cmax[c]);
    int n = 0;
    double run = before;
    for (int64_t i = lo; i < hi; ++i)
        if (i == 0 || x[i] > run) { ++n; run = x[i]; }
    cnt[tid] = n;
    __syncthreads();
    int off = 0;
    for (int c = 0; c < tid; ++c) off += cnt[c];
    run = before;
    for (int64_t i = lo; i < hi; ++i)
        if (i == 0 || x[i] > run) { rec[off++] = (int)i; run = x[i]; }
    __syncthreads();
    if (tid == 0) { // the walk: the anchor moves at a record above anchor + thresh
        int total = 0;
        for (int c = 0; c < SEL; ++c) total += cnt[c];
        double a = x[0];
        int64_t ia = 0;
        for (int q = 1; q < total; ++q) {
            const double v = x[rec[q]];
            if (v > a + thresh) { a = v; ia = rec[q]; }
        }
        s_a = a;
        s_ia = ia;
    }
    __syncthreads();
    const double a = s_a;
    const int64_t ia = s_ia;
    double bv = 0.0;
    int64_t bi = -1;
    for (int64_t i = ia + tid; i < T; i += SEL) // increasing i per thread: the first maximum of its own candidates
        if ((i == ia || x[i] > a - thresh) && first_max(col2[i], i, bv, bi)) { bv = col2[i]; bi = i; }
    bval[tid] = bv;
    bidx[tid] = bi;
    __syncthreads();
    for (int s = SEL / 2; s > 0; s >>= 1) {
        if (tid < s && first_max(bval[tid + s], bidx[tid + s], bval[tid], bidx[tid])) { bval[tid] = bval[tid + s]; bidx[tid] = bidx[tid + s]; }
        __syncthreads();
    }
    const int64_t j = bidx[0];
    // w = resid[:, j] and norm(w)^2 (:314-315), summed in a fixed order
    double ss = 0.0;
    for (int q = tid; q < M; q += SEL) { const double v = X[j * M + q]; wbuf[q] = v; ss = fma(v, v, ss); }
    __syncthreads();
    bval[tid] = ss;
    __syncthreads();
    for (int s = SEL / 2; s > 0; s >>= 1) {
        if (tid < s) bval[tid] += bval[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const double nw = sqrt(bval[0]);
        wbuf[M] = nw * nw;
        vertices[round] = j;
        if (!(nw > 0.0)) atomicAdd(&flags[FL_ZERO_W], 1ull);
    }
}

// V[r][n] = data[n, vertices[r]] (:23); data is [t][n]
static __global__ __launch_bounds__(256) void sep_gather_kernel(const double *data, const int64_t *vertices, double *V, int N)
{
    const int64_t t = vertices[blockIdx.x];
    for (int n = threadIdx.x; n < N; n += 256) V[(int64_t)blockIdx.x * N + n] = data[t * N + n];
}

// out[row] = sum_t |X[row][t]| (square = 0) or sqrt(sum_{t < len(row)} X[row][t]^2) (square = 1) with len = T - (row % L) when L > 0: one
// workgroup per row, strided partial sums and a tree, a fixed order.  With L > 0 the rows are (a, l) pairs of head[a, l] and X row a.
static __global__ __launch_bounds__(256) void sep_rowsum_kernel(const double *X, int64_t T, int L, int square, double *out)
{
    __shared__ double red[256];
    const int64_t row = L > 0 ? blockIdx.x / L : blockIdx.x, n = L > 0 ? T - blockIdx.x % L : T;
    const double *x = X + row * T;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < n; t += 256) { const double v = x[t]; s = square ? fma(v, v, s) : s + fabs(v); }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = square ? sqrt(red[0]) : red[0];
}

// renormalize! (:340-348): G[r, :] *= 1 / d[r], V[:, r] *= d[r] with d = diagscale(rowsum); one workgroup per row
static __global__ __launch_bounds__(256) void sep_rescale_kernel(double *G, int64_t T, double *V, int N, const double *rowsum)
{
    const double s = rowsum[blockIdx.x], d = s + (s < DBL_EPS ? 1.0 : 0.0), inv = 1.0 / d;
    double *g = G + (int64_t)blockIdx.x * T, *v = V + (int64_t)blockIdx.x * N;
    for (int64_t t = threadIdx.x; t < T; t += 256) g[t] *= inv;
    for (int n = threadIdx.x; n < N; n += 256) v[n] *= d;
}

// part[z][a][p] = sum_{t in split z} G[a, t] G[b, t+l], p = b*L + l; G is [r][t].  The tiling of fp64_gemm_kernel with the T range of a
// workgroup given by blockIdx.z (chunk is a multiple of TR).
static __global__ __launch_bounds__(256) void sep_lag_kernel(const double *G, int R, int L, int64_t T, int64_t chunk, double *part)
{
    using namespace fp64;
    __shared__ double As[TR][TM + 1];
    __shared__ double Bs[TR][TP + 1];
    const int tid = threadIdx.x, tm = tid % 16, tp = tid / 16;
    const int64_t m0 = (int64_t)blockIdx.x * TM, p0 = (int64_t)blockIdx.y * TP, PL = (int64_t)R * L;
    const int64_t t_lo = (int64_t)blockIdx.z * chunk, t_hi = t_lo + chunk < T ? t_lo + chunk : T;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int64_t t0 = t_lo; t0 < t_hi; t0 += TR) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, row = idx / TR;
            const int64_t t = t0 + idx % TR, a = m0 + row, p = p0 + row;
            As[idx % TR][row] = (a < R && t < t_hi) ? G[a * T + t] : 0.0;
            const int64_t b = p / L, l = p % L;
            Bs[idx % TR][row] = (p < PL && t < t_hi && t + l < T) ? G[b * T + t + l] : 0.0;
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
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t m = m0 + tm + 16 * a, p = p0 + tp + 16 * b;
            if (m < R && p < PL) part[((int64_t)blockIdx.z * R + m) * PL + p] = acc[a][b];
        }
}

static __global__ __launch_bounds__(256) void sep_lag_sum_kernel(const double *part, int64_t n, int splits, double *P)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int z = 0; z < splits; ++z) s += part[(int64_t)z * n + i];
    P[i] = s;
}

} // namespace sep
