#pragma once
// cmf_anls.h -- gfx950 kernels of the ANLS rule (src/algs/anls.jl), all in fp64 ("The ANLS rule").
//
// The solver is block principal pivoting (Kim & Park, SIAM J. Sci. Comput. 33(6), 2011) on the normal equations G x = c: a
// passive set P, x_P = G_PP^{-1} c_P by Cholesky, y = G x - c off P, infeasible i: x_i < -tol (in P) or y_i < -tol (off P).
// With p = 3 and ninf = n + 1 at the start: fewer infeasible indices than ninf -> ninf = that count, p = 3, exchange all;
// else p >= 1 -> p -= 1, exchange all; else exchange only the infeasible index of largest number (the backup rule).
// Every loop is bounded: a problem of n unknowns runs at most `cap` rounds (anls_round_cap) and reports it when it gets there.
//
//   anls_nnls_w_kernel   W step: one workgroup per unit n, n = K*L <= 128 unknowns, all problems share G = Hstk*Hstk'.  The
//                        passive-set submatrix of G is gathered into LDS as a packed lower triangle (66 KB at 128 unknowns),
//                        factorised and solved there; y is formed from G in global memory / L2.  Larger K*L is refused by the
//                        host (CMF_ERR_UNSUPPORTED), not run through global scratch.
//   nnls_wave            K <= 64 unknowns on one wave: lane k owns unknown k, the passive set is a 64-bit ballot, the compact
//                        Gram lives in LDS (one row per lane), the triangular solves run in registers through __shfl.
//   anls_h_sweep_kernel  basic H step: ONE one-wave workgroup walks t = t0..t1-1; c = B[:, t] - sum_{e != 0} A_Lt(e) H[:, t+e]
//                        with the already updated columns (e < 0) in an LDS ring, the old ones (e > 0) from global memory.
//                        A one-wave workgroup needs no hardware barrier: __syncthreads() is an LDS fence there.
//   anls_h_block_kernel  block H step: one wave per column of a phase l, l+L, l+2L, ... (their windows are disjoint).
//   anls_lag_gram_kernel A_Lt(e) for Lt = 1..L: the full lag-Grams (Lt = L) and the truncated ones of the last L-1 columns
// The contractions (G, C = Hstk*data', B = transconv(W, data), the loss of conv(W, H)) are fp64_gemm_kernel of cmf_fp64.h
// with its loaders and the ones below.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "cmf_fp64.h"

namespace anls {

constexpr int WMAX = 128;    // unknowns of a W-step problem (K*L)
constexpr int KMAX = 64;     // unknowns of an H-step problem (K)
constexpr int KS = KMAX + 1; // row stride of the compact Gram of nnls_wave in LDS
// counters of a call in device memory: rounds summed over problems, problems that took the backup rule, problems that
// hit the cap, problems whose factorisation met a non-positive or non-finite pivot
enum { ST_ROUNDS = 0, ST_BACKUP = 1, ST_CAPPED = 2, ST_BADPIVOT = 3, ST_N = 4 };

__host__ __device__ inline int anls_round_cap(int n, int backup_only) { return backup_only ? 50 * n + 50 : 5 * n + 10; }

// ---- loaders / epilogues for fp64_gemm_kernel ---------------------------------------------------------------------------------
// B(r, s) = data[n, s + l] (r = n + N*l), zero past the end: the linear transconv of the H step; data is [t][n]
struct ShiftColsLin {
    const double *X; int N; int64_t T;
    __device__ double operator()(int64_t r, int64_t s) const {
        const int l = (int)(r / N), n = (int)(r % N);
        const int64_t t = s + l;
        return t < T ? X[t * N + n] : 0.0;
    }
};
// B(r, t) = H[k, t - l] (r = k + K*l), zero for t < l; H in Julia's layout H[k + K*t]
struct LagHT {
    const double *H; int K;
    __device__ double operator()(int64_t r, int64_t t) const {
        const int l = (int)(r / K), k = (int)(r % K);
        return t >= l ? H[(t - l) * K + k] : 0.0;
    }
};
struct EpiStoreT { // C[p][m] (row stride ld) = acc
    double *C; int64_t ld;
    __device__ double operator()(int64_t m, int64_t p, double acc) const { C[p * ld + m] = acc; return 0.0; }
};

// A[((Lt-1)*(2L-1) + e + L-1)*K*K + k*K + k'] = sum_{l < Lt, 0 <= l-e < L} sum_n W[k, n, l] W[k', n, l-e]; one thread per (e, k, k')
// walks l upwards and leaves the running sum behind after every l.  W in Julia's layout W[k + K*(n + N*l)].
static __global__ __launch_bounds__(256) void anls_lag_gram_kernel(const double *W, double *A, int K, int64_t N, int L)
{
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (int64_t)(2 * L - 1) * K * K;
    if (id >= per) return;
    const int e = (int)(id / ((int64_t)K * K)) - (L - 1), k = (int)((id / K) % K), kp = (int)(id % K);
    double s = 0.0;
    for (int l = 0; l < L; ++l) {
        const int lp = l - e;
        if (lp >= 0 && lp < L) {
            const double *a = W + (int64_t)K * N * l, *b = W + (int64_t)K * N * lp;
            for (int64_t n = 0; n < N; ++n) s += a[k + K * n] * b[kp + K * n];
        }
        A[(int64_t)l * per + id] = s;
    }
}

// the exchange rule; true: only the infeasible index of largest number changes sides
__device__ inline bool pivot_single(int nv, int &ninf, int &p, int backup_only, bool &used_backup)
{
    if (!backup_only) {
        if (nv < ninf) { ninf = nv; p = 3; return false; }
        if (p >= 1) { --p; return false; }
    }
    used_backup = true;
    return true;
}

// ---- W step ---------------------------------------------------------------------------------------------------------------------
__device__ inline int tri(int a, int b) { return a * (a + 1) / 2 + b; } // packed lower triangle, b <= a

// G: n x n row-major, symmetric bit for bit (both triangles come from the same sums); C, X: [i][col] with row stride N.
// X[:, col] is written only when the problem ends regularly.
static __global__ __launch_bounds__(256) void anls_nnls_w_kernel(const double *G, const double *C, double *X, int n, int64_t N, double tol, int cap,
                                                                 int backup_only, unsigned long long *st)
{
    __shared__ double A[WMAX * (WMAX + 1) / 2];
    __shared__ double c[WMAX], x[WMAX], z[WMAX];
    __shared__ int idx[WMAX];
    __shared__ unsigned char inP[WMAX];
    __shared__ int s_vmax;
    const int tid = threadIdx.x, ta = tid >> 4, tb = tid & 15;
    const int64_t col = blockIdx.x;
    if (tid < n) {
        c[tid] = C[(int64_t)tid * N + col];
        x[tid] = 0.0;
        inP[tid] = 0;
    }
    __syncthreads();
    double y = tid < n ? -c[tid] : 0.0;
    int ninf = n + 1, p = 3, rounds = 0;
    bool used_backup = false, capped = false, bad = false;
    for (;;) {
        const bool inf = tid < n && (inP[tid] ? x[tid] < -tol : y < -tol);
        if (tid == 0) s_vmax = -1;
        const int nv = __syncthreads_count(inf);
        if (nv == 0) break;
        if (rounds >= cap) { capped = true; break; }
        ++rounds;
        if (inf) atomicMax(&s_vmax, tid);
        __syncthreads();
        const bool single = pivot_single(nv, ninf, p, backup_only, used_backup);
        if (inf && (!single || tid == s_vmax)) inP[tid] ^= 1;
        __syncthreads();
        // the passive indices in increasing order
        bool mine = false;
        if (tid < n && inP[tid]) {
            mine = true;
            int r = 0;
            for (int j = 0; j < tid; ++j) r += inP[j];
            idx[r] = tid;
        }
        const int m = __syncthreads_count(mine);
        for (int a = ta; a < m; a += 16) {
            const double *row = G + (int64_t)idx[a] * n;
            for (int b = tb; b <= a; b += 16) A[tri(a, b)] = row[idx[b]];
        }
        if (tid < m) z[tid] = c[idx[tid]];
        __syncthreads();
        // Cholesky of the packed triangle, right-looking
        for (int j = 0; j < m; ++j) {
            double d = A[tri(j, j)];
            if (!(d > 0.0) || !(d <= 1.7e308)) { bad = true; break; } // (the same value in every thread)
            d = sqrt(d);
            __syncthreads();
            if (tid == 0) A[tri(j, j)] = d;
            for (int i = j + 1 + tid; i < m; i += 256) A[tri(i, j)] /= d;
            __syncthreads();
            for (int a = j + 1 + ta; a < m; a += 16) {
                const double la = A[tri(a, j)];
                for (int b = j + 1 + tb; b <= a; b += 16) A[tri(a, b)] -= la * A[tri(b, j)];
            }
            __syncthreads();
        }
        if (bad) break;
        for (int j = 0; j < m; ++j) { // L w = c_P
            if (tid == 0) z[j] /= A[tri(j, j)];
            __syncthreads();
            const double zj = z[j];
            for (int i = j + 1 + tid; i < m; i += 256) z[i] -= A[tri(i, j)] * zj;
            __syncthreads();
        }
        for (int j = m - 1; j >= 0; --j) { // L' x_P = w
            if (tid == 0) z[j] /= A[tri(j, j)];
            __syncthreads();
            const double xj = z[j];
            for (int i = tid; i < j; i += 256) z[i] -= A[tri(j, i)] * xj;
            __syncthreads();
        }
        if (tid < n) x[tid] = 0.0;
        __syncthreads();
        if (tid < m) x[idx[tid]] = z[tid];
        if (tid < n && !inP[tid]) { // y = G x - c off P (column tid of the symmetric G: the reads of a wave are contiguous)
            double s = 0.0;
            for (int a = 0; a < m; ++a) s += G[(int64_t)idx[a] * n + tid] * z[a];
            y = s - c[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        atomicAdd(&st[ST_ROUNDS], (unsigned long long)rounds);
        if (used_backup) atomicAdd(&st[ST_BACKUP], 1ull);
        if (capped) atomicAdd(&st[ST_CAPPED], 1ull);
        if (bad) atomicAdd(&st[ST_BADPIVOT], 1ull);
    }
    if (!capped && !bad && tid < n) X[(int64_t)tid * N + col] = inP[tid] ? fmax(x[tid], 0.0) : 0.0;
}

// ---- H step ---------------------------------------------------------------------------------------------------------------------
// One wave solves min_{x >= 0} over K <= 64 unknowns: lane k passes c_k and gets x_k back.  G: K x K row-major (any address
// space).  Ls: KMAX*KS doubles of LDS, xs / xf: 64 doubles of LDS each.  fail: 0, ST_CAPPED or ST_BADPIVOT.  Called by all 64
// lanes of a one-wave workgroup.
__device__ inline double nnls_wave(const double *G, int K, double c, double tol, int cap, int backup_only, double *Ls, double *xs, double *xf,
                                   int &rounds, bool &used_backup, int &fail)
{
    const int lane = threadIdx.x;
    const bool live = lane < K;
    bool inP = false;
    double x = 0.0, y = -c;
    int ninf = K + 1, p = 3;
    rounds = 0;
    fail = 0;
    for (;;) {
        const bool inf = live && (inP ? x < -tol : y < -tol);
        const unsigned long long V = __ballot(inf);
        if (!V) break;
        if (rounds >= cap) { fail = ST_CAPPED; break; }
        ++rounds;
        const bool single = pivot_single(__popcll(V), ninf, p, backup_only, used_backup);
        const int vmax = 63 - __clzll((long long)V);
        if (inf && (!single || lane == vmax)) inP = !inP;
        const unsigned long long Pm = __ballot(inP);
        const int m = __popcll(Pm);
        const int a = __popcll(Pm & ((1ull << lane) - 1ull)); // this lane's row of the compact system when it is passive
        {
            unsigned long long q = Pm;
            for (int b = 0; q; ++b) {
                const int j = __ffsll((long long)q) - 1;
                q &= q - 1;
                if (inP && b <= a) Ls[a * KS + b] = G[lane * K + j];
            }
        }
        if (inP) xs[a] = c;
        __syncthreads();
        double z = lane < m ? xs[lane] : 0.0; // from here on lane r < m owns row r of the compact system
        for (int j = 0; j < m; ++j) { // Cholesky, left-looking, a row per lane
            double s = 0.0;
            if (lane >= j && lane < m) {
                s = Ls[lane * KS + j];
                for (int q = 0; q < j; ++q) s -= Ls[lane * KS + q] * Ls[j * KS + q];
            }
            double d = __shfl(s, j, 64);
            if (!(d > 0.0) || !(d <= 1.7e308)) { fail = ST_BADPIVOT; break; }
            d = sqrt(d);
            if (lane >= j && lane < m) Ls[lane * KS + j] = lane == j ? d : s / d;
            __syncthreads();
        }
        if (fail) break;
        for (int j = 0; j < m; ++j) { // L w = c_P
            const double zj = __shfl(z, j, 64) / Ls[j * KS + j];
            if (lane == j) z = zj;
            else if (lane > j && lane < m) z -= Ls[lane * KS + j] * zj;
        }
        for (int j = m - 1; j >= 0; --j) { // L' x_P = w
            const double xj = __shfl(z, j, 64) / Ls[j * KS + j];
            if (lane == j) z = xj;
            else if (lane < j) z -= Ls[j * KS + lane] * xj;
        }
        __syncthreads();
        if (lane < m) xs[lane] = z;
        __syncthreads();
        x = inP ? xs[a] : 0.0;
        xf[lane] = live ? x : 0.0;
        __syncthreads();
        if (live && !inP) {
            double s = 0.0;
            for (int j = 0; j < K; ++j) s += G[lane * K + j] * xf[j];
            y = s - c;
        }
        __syncthreads();
    }
    return inP ? fmax(x, 0.0) : 0.0;
}

// sum_{e != 0, 0 <= t+e < T} A(e)[k, :] H[:, t+e] spread over the wave: lane = g*K + k takes the lags e = -(L-1) + g, + ng, ...
// and lane k < K adds the ng partial sums up in a fixed order.  At: (2L-1) x K x K.  RING: columns before t come from `ring`
// (slot s mod (L-1)), else from H.
template <bool RING>
__device__ inline double column_rhs(const double *At, const double *Bt, const double *H, const double *ring, double *part, int K, int L, int64_t T, int64_t t)
{
    const int lane = threadIdx.x, ng = 64 / K, g = lane / K, k = lane % K;
    double s = 0.0;
    if (g < ng)
        for (int e = -(L - 1) + g; e <= L - 1; e += ng) {
            const int64_t ts = t + e;
            if (e == 0 || ts < 0 || ts >= T) continue;
            const double *hc = (RING && e < 0) ? ring + (ts % (L - 1)) * K : H + ts * K;
            const double *Ae = At + ((int64_t)(e + L - 1) * K + k) * K;
            for (int j = 0; j < K; ++j) s += Ae[j] * hc[j];
        }
    part[lane] = s;
    __syncthreads();
    double tot = 0.0;
    if (lane < K) {
        for (int q = 0; q < ng; ++q) tot += part[q * K + lane];
        tot = Bt[t * K + lane] - tot;
    }
    __syncthreads();
    return tot;
}

// Basic H step (anls.jl:63-94 in Gram form) for the columns t0..t1-1, in order.  A: L x (2L-1) x K x K (anls_lag_gram_kernel),
// Bt: [t][k], H: [t][k] (Julia's layout), updated in place.  Dynamic LDS: (L-1)*K doubles of ring, then (2L-1)*K*K doubles
// for the full lag-Grams when a_lds is set.  Launch: one workgroup of 64.
static __global__ __launch_bounds__(64) void anls_h_sweep_kernel(const double *A, const double *Bt, double *H, int K, int L, int64_t T, int64_t t0, int64_t t1,
                                                                 double tol, int cap, int backup_only, int a_lds, unsigned long long *st)
{
    __shared__ double Ls[KMAX * KS];
    __shared__ double xs[64], xf[64], part[64];
    extern __shared__ double dyn[];
    const int lane = threadIdx.x;
    const int R = L - 1;
    const int64_t per = (int64_t)(2 * L - 1) * K * K;
    double *ring = dyn;
    const double *Afull = A + (int64_t)(L - 1) * per;
    if (a_lds) {
        double *Al = dyn + (int64_t)R * K;
        for (int64_t i = lane; i < per; i += 64) Al[i] = Afull[i];
        Afull = Al;
    }
    for (int64_t s = (t0 - R > 0 ? t0 - R : 0); s < t0; ++s)
        if (lane < K) ring[(s % R) * K + lane] = H[s * K + lane];
    __syncthreads();
    unsigned long long rounds_sum = 0, backups = 0;
    int fail = 0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t left = T - t;
        const int Lt = left < L ? (int)left : L;
        const double *At = Lt == L ? Afull : A + (int64_t)(Lt - 1) * per;
        const double c = column_rhs<true>(At, Bt, H, ring, part, K, L, T, t);
        int rounds;
        bool used_backup = false;
        const double x = nnls_wave(At + (int64_t)(L - 1) * K * K, K, c, tol, cap, backup_only, Ls, xs, xf, rounds, used_backup, fail);
        rounds_sum += rounds;
        backups += used_backup;
        if (fail) break;
        if (lane < K) {
            H[t * K + lane] = x;
            if (R > 0) ring[(t % R) * K + lane] = x;
        }
        __syncthreads();
    }
    if (lane == 0) {
        atomicAdd(&st[ST_ROUNDS], rounds_sum);
        atomicAdd(&st[ST_BACKUP], backups);
        if (fail) atomicAdd(&st[fail], 1ull);
    }
}

// Block H step (anls.jl:101-134 in Gram form), one phase: the columns first, first + L, ... (ncols of them, all with a full
// window: first + (ncols-1)*L <= T - L), one one-wave workgroup per column.  Afull: (2L-1) x K x K.
static __global__ __launch_bounds__(64) void anls_h_block_kernel(const double *Afull, const double *Bt, double *H, int K, int L, int64_t T, int64_t first,
                                                                 int64_t ncols, double tol, int cap, int backup_only, unsigned long long *st)
{
    __shared__ double Ls[KMAX * KS];
    __shared__ double xs[64], xf[64], part[64];
    if ((int64_t)blockIdx.x >= ncols) return;
    const int lane = threadIdx.x;
    const int64_t t = first + (int64_t)blockIdx.x * L;
    const double c = column_rhs<false>(Afull, Bt, H, nullptr, part, K, L, T, t);
    int rounds, fail;
    bool used_backup = false;
    const double x = nnls_wave(Afull + (int64_t)(L - 1) * K * K, K, c, tol, cap, backup_only, Ls, xs, xf, rounds, used_backup, fail);
    if (!fail && lane < K) H[t * K + lane] = x;
    if (lane == 0) {
        atomicAdd(&st[ST_ROUNDS], (unsigned long long)rounds);
        if (used_backup) atomicAdd(&st[ST_BACKUP], 1ull);
        if (fail) atomicAdd(&st[fail], 1ull);
    }
}

} // namespace anls
