#pragma once
// cmf_nnls_large.h -- the shared-Gram NNLS solver for 129 .. 1024 unknowns ("More than 128 unknowns"): the same
// block principal pivoting as anls_nnls_w_kernel (cmf_anls.h) with the same decisions -- pivot_single, anls_round_cap, tol, the
// ST_* counters, exact zeros off the passive set, passive entries clipped at zero, a bad pivot or a capped problem leaves its
// column of X unwritten -- but the factor of the passive submatrix lives in device memory, not in LDS.
//
//   nnls_large_kernel   persistent workgroups of 256: workgroup b owns slab b of the scratch ((n + 1) rows of `ld` doubles) and
//                       walks the problems b, b + gridDim.x, ...  A round gathers G_PP (lower triangle) into rows 0..m-1 of the
//                       slab and c_P into row m, then factorises by panels of NB = 32 columns: the diagonal block in LDS, the
//                       panel below it solved against that block (a row per thread, eight columns at a time in registers), the trailing submatrix
//                       updated by 64 x 64 tiles (4 x 4 per thread, the panel staged in LDS).  Row m rides along, so that it ends
//                       as w = L^-1 c_P and no forward substitution is left; the backward substitution goes block by block from
//                       the last one.  c, v (x on the passive set, y off it), z, idx, inP stay in LDS (29 KB at n = 1024).
//                       No inter-workgroup waits; every sum has a fixed order, so a call is bit-repeatable.
// Included after cmf_anls.h by cmf_anls.hip and cmf_sep.hip.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "cmf_anls.h"

namespace anls {

constexpr int WLARGE = 1024;  // unknowns of a problem of nnls_large_kernel (option "nnls_large"); up to WMAX the LDS kernel runs
constexpr int NB = 32;        // columns of a panel
constexpr int LT = 64;        // rows / columns of a tile of the trailing update
constexpr int LC = 16;        // panel columns staged per step of the trailing update

// row stride of a slab: whole 128-byte lines, an odd number of them (rows a power of two apart would meet in one L2 channel)
__host__ __device__ inline int large_ld(int n) { return 16 * (((n + 15) / 16) | 1); }
__host__ __device__ inline size_t large_slab(int n) { return (size_t)(n + 1) * large_ld(n); }

// Cholesky of the jb x jb diagonal block at (j0, j0) of the slab, in LDS; Ds is padded to NB x NB by the identity and stays
// behind for the panel solve with dinv = 1 / diagonal.  False (in every thread): a non-positive or non-finite pivot.
__device__ inline bool large_factor_diag(double *A, int ld, int j0, int jb, double (*Ds)[NB + 1], double *dinv)
{
    const int tid = threadIdx.x;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, q = e % NB;
        Ds[r][q] = (r < jb && q <= r) ? A[(size_t)(j0 + r) * ld + j0 + q] : (r == q ? 1.0 : 0.0);
    }
    if (tid < NB) dinv[tid] = 1.0;
    __syncthreads();
    for (int j = 0; j < jb; ++j) {
        double d = Ds[j][j];
        if (!(d > 0.0) || !(d <= 1.7e308)) return false; // (the same value in every thread)
        d = sqrt(d);
        if (tid > j && tid < jb) Ds[tid][j] /= d;
        __syncthreads();
        if (tid == 0) { Ds[j][j] = d; dinv[j] = 1.0 / d; } // (nobody reads the diagonal entry in this phase)
        for (int e = tid; e < NB * NB; e += 256) {
            const int a = e / NB, b = e % NB;
            if (b > j && b <= a && a < jb) Ds[a][b] -= Ds[a][j] * Ds[b][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, q = e % NB;
        if (r < jb && q <= r) A[(size_t)(j0 + r) * ld + j0 + q] = Ds[r][q];
    }
    return true;
}

// rows j1..m of the panel (j0, jb): row <- row * L_D^-T, a row per thread, eight columns at a time in registers (the columns
// already solved are read back: the thread's own stores)
__device__ inline void large_panel_solve(double *A, int ld, int j0, int jb, int j1, int m, const double (*Ds)[NB + 1], const double *dinv)
{
    for (int i = j1 + (int)threadIdx.x; i <= m; i += 256) {
        double *row = A + (size_t)i * ld + j0;
#pragma unroll 1
        for (int sb = 0; sb < jb; sb += 8) {
            double r[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) r[t] = sb + t < jb ? row[sb + t] : 0.0;
#pragma unroll 1
            for (int q = 0; q < sb; ++q) {
                const double rq = row[q];
#pragma unroll
                for (int t = 0; t < 8; ++t) r[t] -= rq * Ds[sb + t][q];
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                double s = r[t];
#pragma unroll
                for (int u = 0; u < t; ++u) s -= r[u] * Ds[sb + t][sb + u];
                r[t] = s * dinv[sb + t];
            }
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (sb + t < jb) row[sb + t] = r[t];
        }
    }
}

// A[i, k] -= sum_{j < jb} A[i, j0 + j] A[k, j0 + j] for j1 <= k <= i <= m, k < m, tile by tile
__device__ inline void large_trailing(double *A, int ld, int j0, int jb, int j1, int m, double (*Pi)[LT + 1], double (*Pk)[LT + 1])
{
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    for (int i0 = j1; i0 <= m; i0 += LT)
        for (int k0 = j1; k0 <= i0 && k0 < m; k0 += LT) {
            double acc[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
            for (int r0 = 0; r0 < jb; r0 += LC) {
#pragma unroll
                for (int q = 0; q < LT * LC / 256; ++q) {
                    const int e = tid + 256 * q, r = e % LC, row = e / LC;
                    const bool in = r0 + r < jb;
                    Pi[r][row] = (in && i0 + row <= m) ? A[(size_t)(i0 + row) * ld + j0 + r0 + r] : 0.0;
                    Pk[r][row] = (in && k0 + row < m) ? A[(size_t)(k0 + row) * ld + j0 + r0 + r] : 0.0;
                }
                __syncthreads();
#pragma unroll
                for (int rr = 0; rr < LC; ++rr) {
                    double av[4], bv[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { av[q] = Pi[rr][ty + 16 * q]; bv[q] = Pk[rr][tx + 16 * q]; }
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
                    const int i = i0 + ty + 16 * a, k = k0 + tx + 16 * b;
                    if (i <= m && k < m && k <= i) A[(size_t)i * ld + k] -= acc[a][b];
                }
        }
}

// G: n x n row-major, symmetric bit for bit; C, X: [i][col] with row stride N (N problems); slabs: gridDim.x * large_slab(n)
// doubles.  X[:, col] is written only when the problem ends regularly.
static __global__ __launch_bounds__(256) void nnls_large_kernel(const double *G, const double *C, double *X, double *slabs, int n, int64_t N, double tol, int cap,
                                                                int backup_only, unsigned long long *st)
{
    __shared__ double c[WLARGE], v[WLARGE], z[WLARGE]; // v: x on the passive set, y off it; z: the compact right-hand side / solution
    __shared__ int idx[WLARGE];
    __shared__ unsigned char inP[WLARGE];
    __shared__ double Ds[NB][NB + 1], dinv[NB];
    __shared__ double Pi[LC][LT + 1], Pk[LC][LT + 1];
    __shared__ int s_nv, s_vmax, s_wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = large_ld(n);
    double *A = slabs + (size_t)blockIdx.x * large_slab(n);
    const int per = (n + 255) / 256, i_lo = tid * per, i_hi = i_lo + per < n ? i_lo + per : n; // this thread's unknowns (in order)
    unsigned long long rounds_sum = 0, backups = 0, n_capped = 0, n_bad = 0;
    for (int64_t col = blockIdx.x; col < N; col += gridDim.x) {
        __syncthreads(); // (the previous problem's LDS is done with)
        for (int i = tid; i < n; i += 256) {
            const double ci = C[(int64_t)i * N + col];
            c[i] = ci;
            v[i] = -ci;
            inP[i] = 0;
        }
        int ninf = n + 1, p = 3, rounds = 0;
        bool used_backup = false, capped = false, bad = false;
        for (;;) {
            if (tid == 0) { s_nv = 0; s_vmax = -1; }
            __syncthreads();
            int mine = 0, top = -1;
            for (int i = i_lo; i < i_hi; ++i)
                if (v[i] < -tol) { ++mine; top = i; }
            if (mine) { atomicAdd(&s_nv, mine); atomicMax(&s_vmax, top); }
            __syncthreads();
            const int nv = s_nv, vmax = s_vmax;
            if (nv == 0) break;
            if (rounds >= cap) { capped = true; break; }
            ++rounds;
            const bool single = pivot_single(nv, ninf, p, backup_only, used_backup);
            int cnt = 0;
            for (int i = i_lo; i < i_hi; ++i) {
                if (v[i] < -tol && (!single || i == vmax)) inP[i] ^= 1;
                cnt += inP[i];
            }
            // the passive indices in increasing order: a scan of the per-thread counts
            int incl = cnt;
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d, 64);
                if (lane >= d) incl += t;
            }
            if (lane == 63) s_wsum[wave] = incl;
            __syncthreads();
            int off = incl - cnt, m = 0;
            for (int w = 0; w < 4; ++w) {
                if (w < wave) off += s_wsum[w];
                m += s_wsum[w];
            }
            for (int i = i_lo; i < i_hi; ++i)
                if (inP[i]) idx[off++] = i;
            __syncthreads();
            // rows 0..m-1: the lower triangle of G_PP; row m: c_P
            for (int a = tid >> 5; a <= m; a += 8) {
                double *row = A + (size_t)a * ld;
                if (a < m) {
                    const double *g = G + (int64_t)idx[a] * n;
                    for (int b = tid & 31; b <= a; b += 32) row[b] = g[idx[b]];
                } else {
                    for (int b = tid & 31; b < m; b += 32) row[b] = c[idx[b]];
                }
            }
            __syncthreads();
            for (int j0 = 0; j0 < m; j0 += NB) {
                const int jb = m - j0 < NB ? m - j0 : NB, j1 = j0 + jb;
                if (!large_factor_diag(A, ld, j0, jb, Ds, dinv)) { bad = true; break; }
                large_panel_solve(A, ld, j0, jb, j1, m, Ds, dinv);
                __syncthreads();
                if (j1 < m) large_trailing(A, ld, j0, jb, j1, m, Pi, Pk);
                __syncthreads();
            }
            if (bad) break;
            for (int a = tid; a < m; a += 256) z[a] = A[(size_t)m * ld + a]; // w = L^-1 c_P
            __syncthreads();
            for (int j0 = (m - 1) / NB * NB; j0 >= 0; j0 -= NB) { // L' x_P = w
                const int jb = m - j0 < NB ? m - j0 : NB;
                for (int e = tid; e < NB * NB; e += 256) {
                    const int r = e / NB, q = e % NB;
                    if (r < jb && q <= r) Ds[r][q] = A[(size_t)(j0 + r) * ld + j0 + q];
                }
                __syncthreads();
                if (wave == 0) {
                    double zz = lane < jb ? z[j0 + lane] : 0.0;
                    for (int j = jb - 1; j >= 0; --j) {
                        const double xj = __shfl(zz, j, 64) / Ds[j][j];
                        if (lane == j) zz = xj;
                        else if (lane < j) zz -= Ds[j][lane] * xj;
                    }
                    if (lane < jb) z[j0 + lane] = zz;
                }
                __syncthreads();
                for (int i = tid; i < j0; i += 256) {
                    double s = z[i];
                    for (int j = 0; j < jb; ++j) s -= A[(size_t)(j0 + j) * ld + i] * z[j0 + j];
                    z[i] = s;
                }
                __syncthreads();
            }
            // x on the passive set, y = G x - c off it (column i of the symmetric G: the reads of a wave are contiguous)
            for (int i = tid; i < n; i += 256)
                if (!inP[i]) {
                    double s = 0.0;
                    for (int a = 0; a < m; ++a) s += G[(int64_t)idx[a] * n + i] * z[a];
                    v[i] = s - c[i];
                }
            for (int a = tid; a < m; a += 256) v[idx[a]] = z[a];
        }
        rounds_sum += rounds;
        backups += used_backup;
        n_capped += capped;
        n_bad += bad;
        if (!capped && !bad)
            for (int i = tid; i < n; i += 256) X[(int64_t)i * N + col] = inP[i] ? fmax(v[i], 0.0) : 0.0;
    }
    if (tid == 0) {
        atomicAdd(&st[ST_ROUNDS], rounds_sum);
        if (backups) atomicAdd(&st[ST_BACKUP], backups);
        if (n_capped) atomicAdd(&st[ST_CAPPED], n_capped);
        if (n_bad) atomicAdd(&st[ST_BADPIVOT], n_bad);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// The scratch of a handle's state: made on first use, grown when a call needs more, freed by large_release (the state's *_free).
struct LargeScratch {
    double *slabs = nullptr;
    size_t doubles = 0;
};
constexpr size_t LARGE_BUDGET = (size_t)1 << 30; // bytes of scratch a state may hold
constexpr unsigned LARGE_WGS = 512;              // workgroups of a launch (two per compute unit)

static void large_release(LargeScratch *ls)
{
    if (ls->slabs) (void)hipFree(ls->slabs);
    ls->slabs = nullptr;
    ls->doubles = 0;
}

// enqueues the solve of `count` problems of n unknowns (WMAX < n <= WLARGE)
static int nnls_large(LargeScratch *ls, hipStream_t st, const char *rule, const double *G, const double *C, double *X, int n, int64_t count, double tol,
                      int backup_only, unsigned long long *counters)
{
    const size_t slab = large_slab(n);
    unsigned wgs = (unsigned)std::min<int64_t>(count, LARGE_WGS);
    wgs = (unsigned)std::max<size_t>(1, std::min<size_t>(wgs, LARGE_BUDGET / (slab * sizeof(double))));
    if (ls->doubles < slab * wgs) {
        HIPCHK(hipStreamSynchronize(st)); // (nothing may still run on the old scratch)
        large_release(ls);
        if (hipMalloc(&ls->slabs, slab * wgs * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            ls->slabs = nullptr;
            return fail(CMF_ERR_HIP, "%s: no device memory for the scratch of the NNLS solver (%u slabs of %zu bytes for %d unknowns)", rule, wgs,
                        slab * sizeof(double), n);
        }
        ls->doubles = slab * wgs;
    }
    hipLaunchKernelGGL(nnls_large_kernel, dim3(wgs), dim3(256), 0, st, G, C, X, ls->slabs, n, count, tol, anls_round_cap(n, backup_only), backup_only, counters);
    KCHK("nnls_large_kernel");
    return CMF_OK;
}

} // namespace anls
