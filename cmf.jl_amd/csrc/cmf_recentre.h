// cmf_recentre.h -- seqNMF's re-centring of motifs (Mackevicius et al., eLife 2019: shiftFactors.m), the decision stated once and free of
// HIP (like cmf_signif.h, cmf_events.h), so that the host entry cmf_recentre_shifts, the kernels of cmf_recentre.hip and a stand-alone CPU
// program (tests/recentre_shift_driver.cpp) share it.
//
// A convolutive factorisation does not change when motif k moves by s lags and row k of H by -s columns, so an MU fit can drift until a
// motif straddles the edge of the L-lag window.  The step moves every motif's centre of mass back to the middle.  In 0-based lags, for
// component k of a K x N x L W:
//     c_l = sum_n W[k, n, l]                    n ascending, from 0.0, in fp64
//     m0  = sum_l c_l,  m1 = sum_l (l + 1) c_l  lags ascending, from 0.0, in fp64 (no fused multiply-add)
//     c   = max(floor(m1 / m0), 1),  centre = max(floor(L / 2), 1),  s_k = centre - c          (shiftFactors.m with its 1-based floor)
//     s_k = 0  where L == 1, where m0 is zero or m0, m1 are not finite, and where the component is dead: no entry of W[k] above the MU
//              clamp floor (without that rule a uniform dead motif at odd L walks one lag per step)
//     W'[k, n, l] = W[k, n, l - s_k] where 0 <= l - s_k < L,  H'[k, t] = H[k, t + s_k] where 0 <= t + s_k < T,  the floor elsewhere.
// c is capped at kCMax so that a W with entries of both signs (a rule without the non-negativity constraint) cannot overflow the int32.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CMF_RC_HD __host__ __device__
#else
#define CMF_RC_HD
#endif

namespace cmfrc {

constexpr double kFloor = 2.220446049250313e-16; // eps(Float64): what w_update_kernel / h_update_kernel clamp at; exact in fp32
constexpr int32_t kCMax = 1 << 30;

// running sums of one component over the lags, in the order of the definition
struct Mass {
    double m0 = 0.0, m1 = 0.0;
    bool live = false; // an entry above the floor has been seen
};
CMF_RC_HD inline void add_lag(Mass &m, int64_t l, double c_l, bool lag_live)
{
#if defined(__clang__)
#pragma clang fp contract(off) // (the device and the host must round (l + 1) c_l alike)
#endif
    m.m0 += c_l;
    const double term = (double)(l + 1) * c_l;
    m.m1 += term;
    m.live = m.live || lag_live;
}

// s_k of a component with these sums in an L-lag window
CMF_RC_HD inline int32_t decide(const Mass &m, int64_t L)
{
    if (L <= 1 || !m.live) return 0;
    if (m.m0 == 0.0 || !std::isfinite(m.m0) || !std::isfinite(m.m1)) return 0;
    const double ratio = std::floor(m.m1 / m.m0);
    const int32_t c = ratio >= (double)kCMax ? kCMax : ratio < 1.0 ? 1 : (int32_t)ratio;
    const int32_t centre = L / 2 >= 1 ? (int32_t)(L / 2) : 1;
    return centre - c;
}

// The table of cmf_recentre_shifts for a K x N x L fp64 W in Julia's order (k fastest).  0: written; 1: the arguments are refused.
inline int shifts(const double *W, int64_t K, int64_t N, int64_t L, int32_t *out)
{
    if (!W || !out || K < 1 || N < 1 || L < 1) return 1;
    for (int64_t k = 0; k < K; ++k) {
        Mass m;
        for (int64_t l = 0; l < L; ++l) {
            double c_l = 0.0;
            bool live = false;
            for (int64_t n = 0; n < N; ++n) {
                const double w = W[k + K * (n + N * l)];
                c_l += w;
                live = live || w > kFloor;
            }
            add_lag(m, l, c_l, live);
        }
        out[k] = decide(m, L);
    }
    return 0;
}

} // namespace cmfrc
