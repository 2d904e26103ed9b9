// cmf_signif.h -- seqNMF's significance test of components on held-out data (Mackevicius et al., eLife 2019: test_significance.m).
//
// For every component k the overlap of its motif with the held-out data, v[k][t] = tensor_transconv(W, X)[k, t] (common.jl:71-81), is
// strongly right-skewed when the motif is a real sequence.  The null distribution of that skewness comes from motifs whose rows are
// circularly shifted along the lag axis, every (component, unit) by an amount of its own: draw 0 is the identity, draw d >= 1 shifts
// row (k, n) by
//     s(d, k, n) = ((bits(base(seed, 0x5157), ((d - 1) K + k) N + n) >> 32) * L) >> 32      (64-bit integer arithmetic, exact for L <= 4096)
// with base / bits of cmf_rng.h, and  Wnull_d[k, n, l] = W[k, n, (l - s) mod L].  The device returns, per draw and component, the three
// raw power sums S1 = sum_t v, S2 = sum_t v^2, S3 = sum_t v^3 over the T' held-out columns, v being the fp32 contraction widened to fp64
// before it is squared and cubed; the skewness, the p-values and the decision are host arithmetic in fp64 (host.py: evaluate_significance).
//
// The first part of this file is free of HIP (the shift table: cmf_null_shifts), so that a stand-alone CPU program can drive it; the
// kernels follow under __HIPCC__:
//   signif_shift_kernel    the null motifs of a batch of B draws as ONE table in the layout of Wn, [Lp][Np][C32]: column c = d_local K + k,
//                          draws packed without padding (a draw may straddle a 32-wide block), C32 = roundup(B K, 32); lags >= L,
//                          rows >= N and columns >= B K are written as exact zeros
//   signif_moments_kernel  the C3 contraction of transconv_kernel (cmf_kernels.h: tc_pair, tc_load_w, cmf_glds16, the 8 x 160 LDS-DMA
//                          chunk ring, the loop over 32-lag blocks) with the moments as its epilogue: a wave owns WHOLE pairs
//                          (128 columns t x 32 columns c, all n chunks), so nothing K x T is ever stored
//   signif_reduce_kernel   the partial sums of a column over the t blocks, added in ascending order
// No atomics; every sum has a fixed order, and a column's result depends on nothing but (W, X, seed, d): not on the batch size, on how
// a range of draws is cut into calls, or on the CU count the handle is planned for.
#pragma once
#include <cstdint>

#define CMF_SIGNIF_STREAM 0x5157ULL // the stream of base(seed, .) the shifts are drawn from
#define CMF_SIGNIF_MAX_L 4096       // (bits >> 32) * L stays below 2^44

#if defined(__HIPCC__)
#define CMF_SIGNIF_HD __host__ __device__
#else
#define CMF_SIGNIF_HD
#endif

namespace cmfsig {

// the integer mix of cmf_rng.h (cmfrng::mix / base / bits), restated so that the device computes the same counters
CMF_SIGNIF_HD inline uint64_t mix(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
CMF_SIGNIF_HD inline uint64_t base(uint64_t seed, uint64_t stream) { return mix(seed + 0x632BE59BD9B4E019ULL * (stream + 1)); }
CMF_SIGNIF_HD inline uint64_t bits(uint64_t b, uint64_t i) { return mix(b + (i + 1) * 0x9E3779B97F4A7C15ULL); }

// s(d, k, n) for draw d >= 0 given b = base(seed, CMF_SIGNIF_STREAM)
CMF_SIGNIF_HD inline int32_t shift(uint64_t b, int64_t d, int64_t k, int64_t n, int64_t K, int64_t N, int64_t L)
{
    if (d <= 0) return 0;
    const uint64_t ctr = ((uint64_t)(d - 1) * (uint64_t)K + (uint64_t)k) * (uint64_t)N + (uint64_t)n;
    return (int32_t)(((bits(b, ctr) >> 32) * (uint64_t)L) >> 32);
}

// The table of cmf_null_shifts: shifts[(j K + k) N + n] = s(first_draw + j, k, n).  0: written; 1: the arguments are refused (CMF_ERR_ARG).
inline int null_shifts(uint64_t seed, int64_t first_draw, int64_t n_draws, int64_t K, int64_t N, int64_t L, int32_t *shifts)
{
    if (!shifts || n_draws < 1 || first_draw < 0 || K < 1 || N < 1 || L < 1 || L > CMF_SIGNIF_MAX_L) return 1;
    const uint64_t b = base(seed, CMF_SIGNIF_STREAM);
    for (int64_t j = 0; j < n_draws; ++j)
        for (int64_t k = 0; k < K; ++k)
            for (int64_t n = 0; n < N; ++n) shifts[(j * K + k) * N + n] = shift(b, first_draw + j, k, n, K, N, L);
    return 0;
}

static inline int64_t gcd64(int64_t a, int64_t b)
{
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}
// draws per batch by default: the smallest multiple of 32 / gcd(K, 32) draws (whole 32-wide column blocks) that fills at least 8 blocks
inline int64_t default_batch(int64_t K)
{
    const int64_t m = 32 / gcd64(K, 32);
    return m * ((256 + K * m - 1) / (K * m));
}

} // namespace cmfsig

#if defined(__HIPCC__)
#include "cmf_kernels.h"

// tab[l][n][c] = Wn[(l - s) mod L][n][k], c = dl K + k, draw d0 + dl; exact zeros outside l < L, n < N, c < B K.
// One thread per (c, n): the shift is computed once and the Lp lags are walked with it.
static __global__ __launch_bounds__(256) void signif_shift_kernel(float *tab, const float *Wn, uint64_t b, long long d0, int B, int K, int N, int L, int Lp,
                                                                  int Np, int K32, int C32)
{
    const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (c >= C32) return;
    const bool live = c < B * K && n < N;
    const int dl = c / K, k = c - dl * K;
    int ls = 0; // source lag of l = 0: (0 - s) mod L
    if (live) {
        const int s = cmfsig::shift(b, d0 + dl, k, n, K, N, L);
        ls = s ? L - s : 0;
    }
    const size_t lag_w = (size_t)Np * K32, lag_t = (size_t)Np * C32;
    const float *src = Wn + (size_t)n * K32 + k;
    float *dst = tab + (size_t)n * C32 + c;
    for (int l = 0; l < Lp; ++l) {
        float v = 0.f;
        if (live && l < L) {
            v = src[(size_t)ls * lag_w];
            ls = (ls + 1 == L) ? 0 : ls + 1;
        }
        dst[(size_t)l * lag_t] = v;
    }
}

struct SgParams {
    const float *tab;  // [Lp][Np][C32]  the null motifs (the layout of Wn with C32 in K32's place)
    const float *XT;   // [Np][TP]       held-out data, transposed
    double *partial;   // [TB][C32][3]
    int Np, TP, PADL, C32, CB, L, Tl;
    int C;             // chunks (8 rows of n) = roundup(N, 8) / 8
    int pairs;         // TB * CB
    int W;             // waves the pairs are dealt to (grid = ceil(W / 4) workgroups): wave w takes pairs w, w + W, ...
};

template <int LT>
__global__ __launch_bounds__(256, 2) void signif_moments_kernel(SgParams p)
{
    __shared__ __attribute__((aligned(16))) float smem[4 * 2 * TC_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    float *S = smem + wave * (2 * TC_CHUNK);
    const int Np = p.Np, TP = p.TP, C32 = p.C32;
    const int gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (gw >= p.W) return;
    const int LB = (p.L + 31) >> 5;
    const size_t lagstride = (size_t)Np * C32;
    const int lagbytes = (int)(lagstride * 4);
    const unsigned lds_S = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float *)S);
    unsigned xoff[5]; // byte offset of this lane's float4 of an 8 x 160 chunk (transconv_kernel)
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        int idx = lane + 64 * q, row = idx / 40, c4 = idx - row * 40;
        xoff[q] = (unsigned)(row * TP + c4 * 4) * 4u;
    }

    for (int pr = gw; pr < p.pairs; pr += p.W) {
        // pair index -> (t block, column block); the column block is the fastest index
        const int cb = pr % p.CB, tblk = pr / p.CB;
        const int t0 = tblk * 128;

        f32x16 acc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

        for (int lb = 0; lb < LB; ++lb) {
            const float *xsrc = p.XT + (p.PADL + t0 + 32 * lb);
            __builtin_amdgcn_wave_barrier(); // the previous block's (or pair's) LDS reads are done
#pragma unroll
            for (int q = 0; q < 5; ++q) cmf_glds16(reinterpret_cast<const char *>(xsrc) + xoff[q], lds_S + q * 1024);
            // operand for n pair `it`: tab[lb*32 + l][2*it + h][cb*32 + i]  (descriptor base: lag lb*32)
            const __amdgpu_buffer_rsrc_t wr = cmf_rsrc(p.tab + (size_t)(lb * 32) * lagstride, (size_t)LT * lagstride * 4);
            const int woff = (h * C32 + cb * 32 + i) * 4;
            float b0[LT], b1[LT];
            tc_load_w<LT>(b0, wr, woff, 0, C32, lagbytes);
            int buf = 0;
            for (int c = 0; c < p.C; ++c) {
                float *Sb = S + buf * TC_CHUNK;
                // chunk c was issued one iteration ago; only the operand prefetch (LT loads) is younger
                __builtin_amdgcn_s_waitcnt(0x0F70 | (LT & 15) | ((LT >> 4) << 14)); // vmcnt(LT)
                __builtin_amdgcn_wave_barrier();
                if (c + 1 < p.C) {
                    const float *xs2 = xsrc + (size_t)(8 * (c + 1)) * TP;
                    const unsigned Sn = lds_S + (buf ^ 1) * (TC_CHUNK * 4);
#pragma unroll
                    for (int q = 0; q < 5; ++q) cmf_glds16(reinterpret_cast<const char *>(xs2) + xoff[q], Sn + q * 1024);
                }
                const int nrow = 8 * c;
                const float *sa = Sb + h * TC_ROW + i;
                tc_load_w<LT>(b1, wr, woff, nrow + 2, C32, lagbytes);
                __builtin_amdgcn_sched_barrier(0);
                tc_pair<LT>(acc, sa, b0);
                tc_load_w<LT>(b0, wr, woff, nrow + 4, C32, lagbytes);
                __builtin_amdgcn_sched_barrier(0);
                tc_pair<LT>(acc, sa + 2 * TC_ROW, b1);
                tc_load_w<LT>(b1, wr, woff, nrow + 6, C32, lagbytes);
                __builtin_amdgcn_sched_barrier(0);
                tc_pair<LT>(acc, sa + 4 * TC_ROW, b0);
                tc_load_w<LT>(b0, wr, woff, nrow + ((c + 1 < p.C) ? 8 : 0), C32, lagbytes);
                __builtin_amdgcn_sched_barrier(0);
                tc_pair<LT>(acc, sa + 6 * TC_ROW, b1);
                buf ^= 1;
            }
        }
        // moments of this lane's 64 values of column cb*32 + i (rows t0 + 32 tb + cmf_crow(r, h)), tb ascending, r ascending; rows beyond the
        // data add an exact 0.  Products and sums are separate roundings (no fused multiply-add).
        double s1 = 0.0, s2 = 0.0, s3 = 0.0;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int tb = 0; tb < 4; ++tb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int t = t0 + tb * 32 + cmf_crow(r, h);
                    const double v = (t < p.Tl) ? (double)acc[tb][r] : 0.0;
                    const double v2 = v * v;
                    const double v3 = v2 * v;
                    s1 = s1 + v;
                    s2 = s2 + v2;
                    s3 = s3 + v3;
                }
            // the two half-waves: h = 0 first
            const double o1 = __shfl_down(s1, 32, 64), o2 = __shfl_down(s2, 32, 64), o3 = __shfl_down(s3, 32, 64);
            if (h == 0) {
                double *q = p.partial + ((size_t)tblk * C32 + cb * 32 + i) * 3;
                q[0] = s1 + o1;
                q[1] = s2 + o2;
                q[2] = s3 + o3;
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): the stores are not among what the next pair's counted waits count
    }
}

// sums[(col0 + c) * 3 + s] = sum over the TB t blocks, ascending, of partial[tb][c][s]   (c < ncols = B K: column c is (draw, component))
static __global__ __launch_bounds__(256) void signif_reduce_kernel(const double *partial, double *sums, int ncols, int C32, int TB, long long col0)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int tb = 0; tb < TB; ++tb) {
        const double *q = partial + ((size_t)tb * C32 + c) * 3;
        a1 += q[0];
        a2 += q[1];
        a3 += q[2];
    }
    double *o = sums + (size_t)(col0 + c) * 3;
    o[0] = a1;
    o[1] = a2;
    o[2] = a3;
}
#endif // __HIPCC__
