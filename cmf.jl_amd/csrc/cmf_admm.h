#pragma once
// cmf_admm.h -- gfx950 kernels of the ADMM rule (src/algs/admm.jl), all in fp64 ("The ADMM rule").
//
//   admm_chol_kernel     the LK x LK Cholesky of G = Hstk*Hstk' + 2I (one workgroup, right-looking, in place; once per W call)
//   admm_trsm_kernel     G \ rhs against N right-hand sides: one wave per column, the column in LDS, no explicit inverse
//   admm_lag_gram_kernel the 2L-1 lag matrices A(d) of the H solve
//   admm_freq_chol_kernel  Gram_f = sum_d A(d) exp(+2 pi i f d / T) + 2I and its Hermitian Cholesky, one thread per frequency 0..T/2
//   admm_freq_solve_kernel the two triangular solves per frequency, and the Hermitian partner T-f
//   admm_fft_*           Bluestein over a radix-2 Stockham FFT of power-of-two length: one path for every T
//   admm_w_cols_kernel   W side steps 4-6 on the stacked columns (norm rule w[n] >= 1, projection, duals U2 / U3)
//   admm_h_aux_kernel    H side steps 3-4 (soft threshold, projection); admm_h_dual_kernel the duals Q2 / Q3
// The contractions are fp64_gemm_kernel of cmf_fp64.h, with its loaders and epilogues and the ones below (the differences of
// two arrays, the circularly wrapped H and data columns, the Z / dual updates).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "cmf_fp64.h"

namespace admm {

// ---- element loaders for fp64_gemm_kernel (A: m x r, B: r x p) -------------------------------------------------------------------
struct RowMajorDiff { // X[r][p] - Y[r][p]
    const double *X, *Y; int64_t ld;
    __device__ double operator()(int64_t r, int64_t p) const { return X[r * ld + p] - Y[r * ld + p]; }
};
// B(r, s) = X[n, (s + l) mod T] - Y[n, ...] with r = n + N*l, X / Y in data's layout [t][n]
struct ShiftColsDiff {
    const double *X, *Y; int N, T;
    __device__ double operator()(int64_t r, int64_t s) const {
        int l = (int)(r / N), n = (int)(r % N);
        int64_t t = s + l;
        if (t >= T) t -= T;
        int64_t o = t * N + n;
        return X[o] - Y[o];
    }
};
// B(r, t) = H[k, t - l] (r = k + K*l): linear (zero for t < l) or circular ((t - l) mod T)
template <bool CIRC>
struct LagH {
    const double *H; int K, T;
    __device__ double operator()(int64_t r, int64_t t) const {
        int l = (int)(r / K), k = (int)(r % K);
        int64_t s = t - l;
        if (s < 0) { if (!CIRC) return 0.0; s += T; }
        return H[(int64_t)k * T + s];
    }
};

// ---- epilogues: called once per output element; the return value is added to the loss partial ---------------------------------
struct EpiRhsW { // rhs[i][n] = acc + Z2 - U2 + Z3 - U3   (admm.jl:63-65)
    double *out; const double *Z2, *U2, *Z3, *U3; int64_t ld;
    __device__ double operator()(int64_t i, int64_t n, double acc) const {
        int64_t o = i * ld + n;
        out[o] = acc + Z2[o] - U2[o] + Z3[o] - U3[o];
        return 0.0;
    }
};
struct EpiZ1W { // estT[t][n] = acc; Z1 = c1*((estT+U1) + c2*data'); U1 += estT - Z1   (admm.jl:68-69, 89)
    double *Z1, *U1; const double *data; int64_t N; double c1, c2;
    __device__ double operator()(int64_t t, int64_t n, double est) const {
        int64_t o = t * N + n;
        double u = U1[o];
        double z = c1 * ((est + u) + c2 * data[o]);
        Z1[o] = z;
        U1[o] = u + (est - z);
        return 0.0;
    }
};
struct EpiLossT { // (data'[t][n] - acc)^2   (admm.jl:93-96)
    const double *data; int64_t N;
    __device__ double operator()(int64_t t, int64_t n, double acc) const { double r = data[t * N + n] - acc; return r * r; }
};
struct EpiRhsH { // y[k][s] = acc + (Z2 - Q2) + (Z3 - Q3): the real input of the forward FFT (admm.jl:180-182, by linearity)
    double *y; const double *Z2, *Q2, *Z3, *Q3; int64_t T;
    __device__ double operator()(int64_t k, int64_t s, double acc) const {
        int64_t o = k * T + s;
        y[o] = acc + (Z2[o] - Q2[o]) + (Z3[o] - Q3[o]);
        return 0.0;
    }
};
struct EpiZ1H { // est[n, t] = acc (kept for the dual update); Z1 = c1*((est+Q1) + c2*data)   (admm.jl:185-186)
    double *est, *Z1; const double *Q1, *data; int64_t N; double c1, c2;
    __device__ double operator()(int64_t n, int64_t t, double e) const {
        int64_t o = t * N + n;
        est[o] = e;
        Z1[o] = c1 * ((e + Q1[o]) + c2 * data[o]);
        return 0.0;
    }
};

// ---- W side: Cholesky of the LK x LK Gram and the triangular solves ------------------------------------------------------------
// In place on G (row-major, lower triangle used); writes the factor's transpose to Lt for the backward solve.
static __global__ __launch_bounds__(1024) void admm_chol_kernel(double *G, double *Lt, int n)
{
    const int tid = threadIdx.x;
    for (int j = 0; j < n; ++j) {
        __syncthreads();
        const double d = sqrt(G[(int64_t)j * n + j]);
        __syncthreads();
        if (tid == 0) G[(int64_t)j * n + j] = d;
        for (int i = j + 1 + tid; i < n; i += 1024) G[(int64_t)i * n + j] /= d;
        __syncthreads();
        // trailing update of the lower triangle: G[i][c] -= G[i][j] G[c][j] for j < c <= i
        const int64_t m = n - j - 1;
        for (int64_t e = tid; e < m * (m + 1) / 2; e += 1024) {
            int64_t i = (int64_t)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
            while (i * (i + 1) / 2 > e) --i;
            while ((i + 1) * (i + 2) / 2 <= e) ++i;
            const int64_t c = e - i * (i + 1) / 2;
            const int64_t ii = j + 1 + i, cc = j + 1 + c;
            G[ii * n + cc] -= G[ii * n + j] * G[cc * n + j];
        }
    }
    __syncthreads();
    for (int64_t e = tid; e < (int64_t)n * n; e += 1024) {
        const int64_t i = e / n, c = e % n;
        Lt[c * n + i] = (c <= i) ? G[i * n + c] : 0.0;
    }
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// X[:, n] = (L L')^{-1} X[:, n] for the columns of X ([i][n], row stride N): one wave per column, the column in LDS (LK doubles)
static __global__ __launch_bounds__(64) void admm_trsm_kernel(const double *Lf, const double *Lt, double *X, int n, int64_t N)
{
    extern __shared__ double y[];
    const int64_t col = blockIdx.x;
    const int lane = threadIdx.x;
    for (int i = lane; i < n; i += 64) y[i] = X[(int64_t)i * N + col];
    __syncthreads();
    for (int i = 0; i < n; ++i) { // L y = b
        double s = 0.0;
        for (int j = lane; j < i; j += 64) s += Lf[(int64_t)i * n + j] * y[j];
        s = wave_sum(s);
        if (lane == 0) y[i] = (y[i] - s) / Lf[(int64_t)i * n + i];
        __syncthreads();
    }
    for (int i = n - 1; i >= 0; --i) { // L' x = y
        double s = 0.0;
        for (int j = i + 1 + lane; j < n; j += 64) s += Lt[(int64_t)i * n + j] * y[j];
        s = wave_sum(s);
        if (lane == 0) y[i] = (y[i] - s) / Lt[(int64_t)i * n + i];
        __syncthreads();
    }
    for (int i = lane; i < n; i += 64) X[(int64_t)i * N + col] = y[i];
}

// W side steps 4-6 (admm.jl:72-91, U1 is in the estT epilogue) on the stacked columns, one thread per column n:
// V2 = Wstk + U2, w = |V2|^2, Z2 = V2 / sqrt(w) where w >= 1 (else kept), Z3 = max(0, Wstk + U3) into Z3n, U2 += Wstk - Z2, U3 += Wstk - Z3
static __global__ __launch_bounds__(256) void admm_w_cols_kernel(const double *Wstk, double *Z2, double *U2, double *Z3n, double *U3, int LK, int64_t N, int nonneg)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double w = 0.0;
    for (int i = 0; i < LK; ++i) {
        const double v = Wstk[i * N + n] + U2[i * N + n];
        w += v * v;
    }
    const bool scale = w >= 1.0;
    const double rs = scale ? sqrt(w) : 1.0;
    for (int i = 0; i < LK; ++i) {
        const int64_t o = i * N + n;
        const double x = Wstk[o], u2 = U2[o], u3 = U3[o];
        double z2 = Z2[o];
        if (scale) { z2 = (x + u2) / rs; Z2[o] = z2; }
        const double z3 = nonneg ? fmax(0.0, x + u3) : x + u3;
        Z3n[o] = z3;
        U2[o] = u2 + (x - z2);
        U3[o] = u3 + (x - z3);
    }
}

// ---- H side ---------------------------------------------------------------------------------------------------------------------
// A[d + L-1][k][k'] = sum_n sum_{l - l' = d} W[k, n, l] W[k', n, l'] (k >= k' only: the Grams are Hermitian)
static __global__ __launch_bounds__(256) void admm_lag_gram_kernel(const double *W, double *A, int K, int64_t N, int L)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nd = 2 * L - 1;
    if (e >= nd * K * K) return;
    const int dd = (int)(e / ((int64_t)K * K)), k = (int)((e / K) % K), kp = (int)(e % K);
    if (kp > k) { A[e] = 0.0; return; }
    const int d = dd - (L - 1);
    double s = 0.0;
    for (int l = (d > 0 ? d : 0); l < L && l - d < L; ++l) {
        const int lp = l - d;
        const double *a = W + (int64_t)K * N * l, *b = W + (int64_t)K * N * lp;
        for (int64_t n = 0; n < N; ++n) s += a[k + K * n] * b[kp + K * n];
    }
    A[e] = s;
}

// Gram_f (lower triangle) and its Cholesky for f = 0..F-1, in place in Lf[(i*K + j)*F + f] (complex as double2)
static __global__ __launch_bounds__(64) void admm_freq_chol_kernel(const double *A, double2 *Lf, int K, int L, int64_t T, int64_t F)
{
    const int64_t f = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) {
            double re = (i == j) ? 2.0 : 0.0, im = 0.0;
            for (int dd = 0; dd < 2 * L - 1; ++dd) {
                const int64_t d = dd - (L - 1);
                int64_t m = (f * d) % T;
                if (m < 0) m += T;
                double sn, cs;
                sincospi(2.0 * (double)m / (double)T, &sn, &cs); // exp(+2 pi i f d / T), the angle from (f*d mod T) in integers
                const double a = A[((int64_t)dd * K + i) * K + j];
                re += a * cs;
                im += a * sn;
            }
            Lf[((int64_t)i * K + j) * F + f] = make_double2(re, im);
        }
    for (int j = 0; j < K; ++j) {
        double d = Lf[((int64_t)j * K + j) * F + f].x;
        for (int p = 0; p < j; ++p) {
            const double2 v = Lf[((int64_t)j * K + p) * F + f];
            d -= v.x * v.x + v.y * v.y;
        }
        d = sqrt(d);
        Lf[((int64_t)j * K + j) * F + f] = make_double2(d, 0.0);
        for (int i = j + 1; i < K; ++i) {
            double2 s = Lf[((int64_t)i * K + j) * F + f];
            for (int p = 0; p < j; ++p) { // s -= L[i][p] conj(L[j][p])
                const double2 a = Lf[((int64_t)i * K + p) * F + f], b = Lf[((int64_t)j * K + p) * F + f];
                s.x -= a.x * b.x + a.y * b.y;
                s.y -= a.y * b.x - a.x * b.y;
            }
            Lf[((int64_t)i * K + j) * F + f] = make_double2(s.x / d, s.y / d);
        }
    }
}

// Y[k][f] <- Gram_f^{-1} Y[k][f] for f = 0..F-1 (Y row-major K x T complex), and Y[k][T-f] = conj(Y[k][f])
static __global__ __launch_bounds__(64) void admm_freq_solve_kernel(const double2 *Lf, double2 *Y, int K, int64_t T, int64_t F)
{
    const int64_t f = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    for (int i = 0; i < K; ++i) { // L y = b
        double2 s = Y[(int64_t)i * T + f];
        for (int j = 0; j < i; ++j) {
            const double2 a = Lf[((int64_t)i * K + j) * F + f], y = Y[(int64_t)j * T + f];
            s.x -= a.x * y.x - a.y * y.y;
            s.y -= a.x * y.y + a.y * y.x;
        }
        const double d = Lf[((int64_t)i * K + i) * F + f].x;
        Y[(int64_t)i * T + f] = make_double2(s.x / d, s.y / d);
    }
    for (int i = K - 1; i >= 0; --i) { // L^H x = y
        double2 s = Y[(int64_t)i * T + f];
        for (int j = i + 1; j < K; ++j) { // s -= conj(L[j][i]) x[j]
            const double2 a = Lf[((int64_t)j * K + i) * F + f], x = Y[(int64_t)j * T + f];
            s.x -= a.x * x.x + a.y * x.y;
            s.y -= a.x * x.y - a.y * x.x;
        }
        const double d = Lf[((int64_t)i * K + i) * F + f].x;
        Y[(int64_t)i * T + f] = make_double2(s.x / d, s.y / d);
    }
    if (f >= 1 && T - f != f)
        for (int i = 0; i < K; ++i) {
            const double2 v = Y[(int64_t)i * T + f];
            Y[(int64_t)i * T + (T - f)] = make_double2(v.x, -v.y);
        }
}

// H side steps 3-4 (admm.jl:189-197): Z2 = sign(H+Q2) max(0, |H+Q2| - lam), Z3 = max(0, H+Q3) into Z3n
static __global__ __launch_bounds__(256) void admm_h_aux_kernel(const double *H, const double *Q2, const double *Q3, double *Z2, double *Z3n, int64_t n, double lam, int nonneg)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double h = H[e], v = h + Q2[e];
    const double mag = fmax(0.0, fabs(v) - lam);
    Z2[e] = v > 0 ? mag : (v < 0 ? -mag : 0.0);
    const double w = h + Q3[e];
    Z3n[e] = nonneg ? fmax(0.0, w) : w;
}

// admm.jl:214-216: Q1 += est - Z1 (n1 elements), Q2 += H - Z2, Q3 += H - Z3 (n2 elements)
static __global__ __launch_bounds__(256) void admm_h_dual_kernel(double *Q1, const double *est, const double *Z1, int64_t n1, double *Q2, double *Q3,
                                                          const double *H, const double *Z2, const double *Z3, int64_t n2)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n1) Q1[e] += est[e] - Z1[e];
    if (e < n2) {
        const double h = H[e];
        Q2[e] += h - Z2[e];
        Q3[e] += h - Z3[e];
    }
}

// ---- FFT along T: Bluestein over a radix-2 Stockham FFT of length M (a power of two >= 2T-1) -------------------------------------
// chirp w[m] = exp(-pi i m^2 / T), the angle from m^2 mod 2T in integers; b[m] = conj(w[|m|]) wrapped into length M
static __global__ __launch_bounds__(256) void admm_chirp_kernel(double2 *w, double2 *b, int64_t T, int64_t M)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    int64_t a = -1;
    if (m < T) a = m;
    else if (M - m < T) a = M - m;
    double sn = 0.0, cs = 0.0;
    if (a >= 0) {
        const int64_t q = (a * a) % (2 * T);
        sincospi((double)q / (double)T, &sn, &cs);
    }
    if (m < T) w[m] = make_double2(cs, -sn);
    b[m] = a >= 0 ? make_double2(cs, sn) : make_double2(0.0, 0.0);
}

// buf[row][m] = x[row][m] * w[m] for m < T, 0 up to M.  REAL: x is real (row stride T); else complex, conjugated when CONJ
template <bool REAL, bool CONJ>
static __global__ __launch_bounds__(256) void admm_fft_pre_kernel(const void *x, const double2 *w, double2 *buf, int64_t T, int64_t M)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (m >= M) return;
    double2 o = make_double2(0.0, 0.0);
    if (m < T) {
        double2 v;
        if (REAL) v = make_double2(static_cast<const double *>(x)[row * T + m], 0.0);
        else v = static_cast<const double2 *>(x)[row * T + m];
        if (CONJ) v.y = -v.y;
        const double2 c = w[m];
        o = make_double2(v.x * c.x - v.y * c.y, v.x * c.y + v.y * c.x);
    }
    buf[row * M + m] = o;
}

// one radix-2 Stockham stage (natural order in and out after log2(M) stages); sign -1 forward, +1 inverse (unnormalised)
static __global__ __launch_bounds__(256) void admm_fft_stage_kernel(const double2 *in, double2 *out, int64_t M, int64_t Ns, double sign)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    const int64_t half = M >> 1;
    if (j >= half) return;
    const double2 *src = in + row * M;
    double2 *dst = out + row * M;
    const int64_t k = j & (Ns - 1);
    const double2 a = src[j], b0 = src[j + half];
    double sn, cs;
    sincospi(sign * (double)k / (double)Ns, &sn, &cs);
    const double2 b = make_double2(b0.x * cs - b0.y * sn, b0.x * sn + b0.y * cs);
    const int64_t o = (j - k) * 2 + k;
    dst[o] = make_double2(a.x + b.x, a.y + b.y);
    dst[o + Ns] = make_double2(a.x - b.x, a.y - b.y);
}

// buf[row][m] *= bh[m]
static __global__ __launch_bounds__(256) void admm_fft_mul_kernel(double2 *buf, const double2 *bh, int64_t M)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (m >= M) return;
    const double2 a = buf[row * M + m], b = bh[m];
    buf[row * M + m] = make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// X[row][t] = w[t] * conv[row][t] / M.  REAL: write Re(X) * scale into a real row (the inverse transform's real part)
template <bool REAL>
static __global__ __launch_bounds__(256) void admm_fft_post_kernel(const double2 *buf, const double2 *w, void *X, int64_t T, int64_t M, double scale)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (t >= T) return;
    const double2 v = buf[row * M + t], c = w[t];
    const double re = (v.x * c.x - v.y * c.y) / (double)M, im = (v.x * c.y + v.y * c.x) / (double)M;
    if (REAL) static_cast<double *>(X)[row * T + t] = re * scale;
    else static_cast<double2 *>(X)[row * T + t] = make_double2(re, im);
}

} // namespace admm
