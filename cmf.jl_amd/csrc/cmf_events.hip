// cmf_events.hip -- the KL form of the MU rule on an event list (cmf_events_*, include/cmf_hip.h): the rule of cmf_mu_set_divergence(CMF_DIV_KL)
// with every sum over the data taken over its non-zero entries only.  R = data ./ (est + eps) is zero where data is zero, so numW and numH
// read est at the events; denomW and denomH never read data (kl_hsum / kl_den_w / kl_wsum / kl_den_h, launched as they are); the sum of
// est over ALL entries, which the loss needs, has a closed form in the sums of W over n and of H over t.  Nothing of size N x T exists.
// cmf_events.h holds the validation, the index and the work tables (free of HIP).
//
// W and H live in the layouts of the dense handle (Wn [Lp][Np][K32], Wt [Lp][K32][Np], H [TP][K32], Ht [K32][TP], PADL >= L - 1 zero rows in
// front of t = 0), so that w_update_kernel and h_update_kernel are launched as they are.  In those layouts the L rows H[t-L+1 .. t] that one
// event reads are ONE contiguous block of LK = L * K32 floats, and so is W[:, n, :] once its lags are reversed: est at an event is a dot
// product of two contiguous vectors, and numW of a unit is the r-weighted sum of such blocks.  No atomics: a long list is cut into chunks
// whose partial sums are added in chunk order.
#include "cmf_internal.h"
#include "cmf_events.h"

#define EV_EPS 2.220446049250313e-16 // eps(Float64): src/CMF.jl:20
#define EV_MAX_GRID (1 << 22)        // workgroups per launch (a longer work table goes out in several launches)

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// r_j = x_j / (est_j + eps) at the events of one work item of the unit table (grid: items; a wave per event, lanes along the reversed
// (lag, component) index).  LOSS: partial[item] = the fp64 sum of the item's log terms x_j log(r_j), wave by wave in a fixed order.
template <bool LOSS>
static __global__ __launch_bounds__(256) void ev_ratio_kernel(const CmfEventsItem *items, int item0, const int32_t *um_time, const float *um_count, const float *Wn,
                                                              const float *H, float *ratio, double *partial, int L, int LK, int K32, int Np, int PADL)
{
    __shared__ float w[CMF_EVENTS_MAX_LK];
    __shared__ double red[4];
    const CmfEventsItem it = items[item0 + blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (it.begin == it.end) { // (a unit without events)
        if (LOSS && tid == 0) partial[item0 + blockIdx.x] = 0.0;
        return;
    }
    for (int i = tid; i < LK; i += 256) { // w[(L-1-l) * K32 + k] = W[k, n, l]
        const int lr = i / K32, k = i - lr * K32;
        w[i] = Wn[((size_t)(L - 1 - lr) * Np + it.dest) * K32 + k];
    }
    __syncthreads();
    double s = 0.0;
    for (int j = it.begin + wave; j < it.end; j += 4) {
        const float *hb = H + (size_t)(PADL + um_time[j] - (L - 1)) * K32; // rows t-L+1 .. t (the rows in front of t = 0 are zero)
        float acc = 0.f;
        for (int i = lane; i < LK; i += 64) acc += w[i] * hb[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) {
            const float x = um_count[j];
            const float q = cmf_kl_ratio(x, acc);
            ratio[j] = q;
            if (LOSS) s += (double)cmf_kl_term(x, x, q); // (v = x: the log term alone; the sum of est - x over ALL entries is ev_loss_kernel's)
        }
    }
    if (LOSS) {
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (tid == 0) partial[item0 + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// numW of one work item of the unit table: acc[(L-1-l) * K32 + k] = sum over the item's events, in order, of r_j H[k, t_j - l].  Threads own
// Q of the LK accumulators each; U events are in flight together.  slot < 0: the finished numW[l][k][n]; else the item's slab.
template <int Q>
static __global__ __launch_bounds__(256) void ev_numw_kernel(const CmfEventsItem *items, int item0, const int32_t *um_time, const float *ratio, const float *H, float *numW,
                                                             float *slabs, int L, int LK, int K32, int Np, int PADL)
{
    constexpr int U = Q <= 4 ? 4 : 2;
    const CmfEventsItem it = items[item0 + blockIdx.x];
    const int tid = threadIdx.x;
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    int j = it.begin;
    for (; j + U <= it.end; j += U) {
        float r[U], v[U][Q];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            r[u] = ratio[j + u];
            const float *hb = H + (size_t)(PADL + um_time[j + u] - (L - 1)) * K32;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int i = tid + 256 * q;
                v[u][q] = hb[i < LK ? i : 0];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] += r[u] * v[u][q];
    }
    for (; j < it.end; ++j) {
        const float r = ratio[j];
        const float *hb = H + (size_t)(PADL + um_time[j] - (L - 1)) * K32;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = tid + 256 * q;
            acc[q] += r * hb[i < LK ? i : 0];
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = tid + 256 * q;
        if (i >= LK) continue;
        if (it.slot >= 0) {
            slabs[(size_t)it.slot * LK + i] = acc[q];
        } else {
            const int lr = i / K32, k = i - lr * K32;
            numW[((size_t)(L - 1 - lr) * K32 + k) * Np + it.dest] = acc[q];
        }
    }
}

// The units with several chunks: numW[l][k][n] = the sum of the unit's slabs in chunk order (grid: fixes)
static __global__ __launch_bounds__(256) void ev_numw_fix_kernel(const CmfEventsFix *fixes, int fix0, const float *slabs, float *numW, int L, int LK, int K32, int Np)
{
    const CmfEventsFix f = fixes[fix0 + blockIdx.x];
    for (int i = threadIdx.x; i < LK; i += 256) {
        float s = 0.f;
        for (int c = 0; c < f.n; ++c) s += slabs[(size_t)(f.first + c) * LK + i];
        const int lr = i / K32, k = i - lr * K32;
        numW[((size_t)(L - 1 - lr) * K32 + k) * Np + f.dest] = s;
    }
}

// numH of one work item of the column table: the item's events lie in columns [t, t + L) of the time-major order; lanes along k read
// Wn[t_p - t][n_p][k]; the G = 256 / K32 groups of lanes take every G-th event and are added in group order.  r_p comes through the
// permutation from the unit-major ratio.  slot < 0: the finished numH[t][k]; else the item's slab.
static __global__ __launch_bounds__(256) void ev_numh_kernel(const CmfEventsItem *items, int item0, const int32_t *tm_unit, const int32_t *tm_time, const int32_t *tm_src,
                                                             const float *ratio, const float *Wn, float *numH, float *slabs, int K32, int Np, int G)
{
    __shared__ float red[256];
    const CmfEventsItem it = items[item0 + blockIdx.x];
    const int tid = threadIdx.x, g = tid / K32, k = tid - g * K32;
    float acc = 0.f;
    if (g < G) {
#pragma unroll 4
        for (int p = it.begin + g; p < it.end; p += G) {
            const int l = tm_time[p] - it.dest;
            acc += Wn[((size_t)l * Np + tm_unit[p]) * K32 + k] * ratio[tm_src[p]];
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < K32) {
        float s = red[tid];
        for (int gg = 1; gg < G; ++gg) s += red[gg * K32 + tid];
        float *out = it.slot >= 0 ? slabs + (size_t)it.slot * K32 : numH + (size_t)it.dest * K32;
        out[tid] = s;
    }
}

// The columns with several chunks: numH[t][k] = the sum of the column's slabs in chunk order (grid: fixes; block K32 <= 256)
static __global__ __launch_bounds__(256) void ev_numh_fix_kernel(const CmfEventsFix *fixes, int fix0, const float *slabs, float *numH, int K32)
{
    const CmfEventsFix f = fixes[fix0 + blockIdx.x];
    const int k = threadIdx.x;
    if (k >= K32) return;
    float s = 0.f;
    for (int c = 0; c < f.n; ++c) s += slabs[(size_t)(f.first + c) * K32 + k];
    numH[(size_t)f.dest * K32 + k] = s;
}

// The loss, one workgroup, fp64 in a fixed order: (sum_j x_j log(x_j / e_j) - sum_j x_j + sum_all e) / sum_j x_j, with
//   sum_all e = sum_k sum_{l < min(L, T)} (sum_n W[k, n, l]) (sum_{t < T - l} H[k, t]) + N T eps
// from the tables of kl_wsum_kernel (wsums[l * K32 + k]) and kl_hsum_kernel (hsums[k * KL_HCHUNKS + c]; the last l entries of the row are
// taken off, as kl_den_w_kernel does).
static __global__ __launch_bounds__(256) void ev_loss_kernel(const double *partial, int n_items, const double *wsums, const double *hsums, const float *Ht, int TP, int PADL,
                                                             int T, int N, int K, int K32, int L, double count_sum, double *out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n_items; i += 256) s += partial[i];
    const double logsum = cmf_block_sum_f64(s, red);
    const int Lm = L < T ? L : T;
    double c = 0.0;
    for (int idx = tid; idx < Lm * K; idx += 256) {
        const int l = idx / K, k = idx - l * K;
        double hs = 0.0;
        for (int q = 0; q < KL_HCHUNKS; ++q) hs += hsums[k * KL_HCHUNKS + q];
        const float *row = Ht + (size_t)k * TP + PADL;
        for (int j = 0; j < l; ++j) hs -= (double)row[T - 1 - j];
        c += wsums[l * K32 + k] * hs;
    }
    const double all = cmf_block_sum_f64(c, red) + (double)N * (double)T * EV_EPS;
    if (tid == 0) *out = ((logsum - count_sum) + all) / count_sum;
}

// a table in W's transposed layout [L][K32][Np] -> Julia order (k fastest, then n, then l)
static __global__ void ev_unpack_wt_kernel(double *out, int N, int K, int L, const float *Wt, int Np, int K32)
{
    const size_t total = (size_t)L * N * K;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(idx % K);
        const size_t r = idx / K;
        const int n = (int)(r % N), l = (int)(r / N);
        out[idx] = (double)Wt[((size_t)l * K32 + k) * Np + n];
    }
}

static __global__ void ev_widen_kernel(double *out, const float *in, size_t n)
{
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) out[idx] = (double)in[idx];
}

// ------------------------------------------------------------------------------------------
// the handle
// ------------------------------------------------------------------------------------------
struct cmf_events_s {
    int device = 0;
    int N = 0, T = 0, K = 0, L = 0, Np = 0, KB = 0, K32 = 0, PADL = 0, TP = 0, Lp = 0, LK = 0;
    int64_t nnz = 0;
    double count_sum = 0.0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs; // everything hipMalloc'ed, in order
    int64_t device_bytes = 0, launches = 0, ratio_passes = 0;
    // the factors and the tables of the update kernels
    float *H = nullptr, *Ht = nullptr, *Wt = nullptr, *Wn = nullptr;
    float *numW = nullptr, *denW = nullptr; // [L][K32][Np]
    float *numH = nullptr, *denH = nullptr; // [T][K32]
    double *hsums = nullptr, *wsums = nullptr, *d_loss = nullptr, *stage = nullptr, *d_hist = nullptr;
    size_t stage_elems = 0, hist_elems = 0;
    // the events, both orders
    int32_t *um_time = nullptr, *tm_unit = nullptr, *tm_time = nullptr, *tm_src = nullptr;
    float *um_count = nullptr, *ratio = nullptr;
    std::vector<int32_t> unit_ptr, time_ptr; // (host: the work tables are rebuilt from them when a chunk option changes)
    // the work tables
    int unit_chunk = 128, time_chunk = 2048, keep_ratio = 1;
    CmfEventsItem *u_items = nullptr, *t_items = nullptr;
    CmfEventsFix *u_fixes = nullptr, *t_fixes = nullptr;
    float *u_slabs = nullptr, *t_slabs = nullptr;
    double *partial = nullptr; // [n_u_items]
    int64_t n_u_items = 0, n_u_fixes = 0, n_t_items = 0, n_t_fixes = 0, table_bytes = 0;
    bool factors_set = false, ratio_valid = false;
};

template <typename T>
static int ev_alloc(cmf_events_s *h, T **p, size_t n, bool tracked = true)
{
    n = std::max<size_t>(n, 1);
    HIPCHK(hipMalloc(p, n * sizeof(T)));
    HIPCHK(hipMemset(*p, 0, n * sizeof(T)));
    if (tracked) h->allocs.push_back(*p);
    h->device_bytes += (int64_t)(n * sizeof(T));
    return CMF_OK;
}

template <typename T>
static int ev_upload(cmf_events_s *h, T **p, const std::vector<T> &v, bool tracked = true)
{
    CMFTRY(ev_alloc(h, p, v.size(), tracked));
    if (!v.empty()) HIPCHK(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return CMF_OK;
}

static void ev_free_tables(cmf_events_s *h)
{
    for (void *p : {(void *)h->u_items, (void *)h->t_items, (void *)h->u_fixes, (void *)h->t_fixes, (void *)h->u_slabs, (void *)h->t_slabs, (void *)h->partial})
        if (p) (void)hipFree(p);
    h->u_items = h->t_items = nullptr;
    h->u_fixes = h->t_fixes = nullptr;
    h->u_slabs = h->t_slabs = nullptr;
    h->partial = nullptr;
    h->device_bytes -= h->table_bytes;
    h->table_bytes = 0;
}

// The work tables for the chunk sizes in force (cmf_events.h), on the device; the slabs of the destinations with several chunks.
static int ev_build_tables(cmf_events_s *h)
{
    std::vector<CmfEventsItem> ui, ti;
    std::vector<CmfEventsFix> uf, tf;
    const int64_t us = cmf_events_items(h->unit_ptr, h->N, 1, h->unit_chunk, &ui, &uf);
    const int64_t ts = cmf_events_items(h->time_ptr, h->T, h->L, h->time_chunk, &ti, &tf);
    if (ui.size() >= ((size_t)1 << 31) || ti.size() >= ((size_t)1 << 31))
        return fail(CMF_ERR_UNSUPPORTED, "unit_chunk=%d, time_chunk=%d: more than 2^31 work items", h->unit_chunk, h->time_chunk);
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
    ev_free_tables(h);
    const int64_t before = h->device_bytes;
    CMFTRY(ev_upload(h, &h->u_items, ui, false));
    CMFTRY(ev_upload(h, &h->t_items, ti, false));
    CMFTRY(ev_upload(h, &h->u_fixes, uf, false));
    CMFTRY(ev_upload(h, &h->t_fixes, tf, false));
    CMFTRY(ev_alloc(h, &h->u_slabs, (size_t)us * h->LK, false));
    CMFTRY(ev_alloc(h, &h->t_slabs, (size_t)ts * h->K32, false));
    CMFTRY(ev_alloc(h, &h->partial, ui.size(), false));
    h->table_bytes = h->device_bytes - before;
    h->n_u_items = (int64_t)ui.size(); h->n_u_fixes = (int64_t)uf.size();
    h->n_t_items = (int64_t)ti.size(); h->n_t_fixes = (int64_t)tf.size();
    return CMF_OK;
}

static int ev_destroy(cmf_events_s *h)
{
    if (!h) return CMF_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    ev_free_tables(h);
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->stage) (void)hipFree(h->stage);
    if (h->d_hist) (void)hipFree(h->d_hist);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CMF_OK;
}

static int ev_ensure_stage(cmf_events_s *h, size_t elems)
{
    if (h->stage_elems >= elems) return CMF_OK;
    if (h->stage) {
        HIPCHK(hipFree(h->stage));
        h->device_bytes -= (int64_t)(h->stage_elems * sizeof(double));
    }
    h->stage = nullptr;
    h->stage_elems = 0;
    HIPCHK(hipMalloc(&h->stage, elems * sizeof(double)));
    h->stage_elems = elems;
    h->device_bytes += (int64_t)(elems * sizeof(double));
    return CMF_OK;
}

static int ev_ready(cmf_events_s *h)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    if (!h->factors_set) return fail(CMF_ERR_STATE, "cmf_events_set_factors has not been called");
    HIPCHK(hipSetDevice(h->device));
    return CMF_OK;
}

// Launches `n` workgroups of a work table in pieces of at most EV_MAX_GRID: launch(first, count).
template <typename F>
static int ev_for_pieces(cmf_events_s *h, int64_t n, const char *name, F launch)
{
    for (int64_t first = 0; first < n; first += EV_MAX_GRID) {
        launch((int)first, (unsigned)std::min<int64_t>(EV_MAX_GRID, n - first));
        KCHK(name);
        h->launches += 1;
    }
    return CMF_OK;
}

// r_j at every event for the resident W, H (LOSS: the block sums of the log terms too)
static int ev_ratio(cmf_events_s *h, bool loss)
{
    CMFTRY(ev_for_pieces(h, h->n_u_items, "ev_ratio_kernel", [&](int first, unsigned n) {
        if (loss)
            hipLaunchKernelGGL(ev_ratio_kernel<true>, dim3(n), dim3(256), 0, h->stream, h->u_items, first, h->um_time, h->um_count, h->Wn, h->H, h->ratio, h->partial, h->L,
                               h->LK, h->K32, h->Np, h->PADL);
        else
            hipLaunchKernelGGL(ev_ratio_kernel<false>, dim3(n), dim3(256), 0, h->stream, h->u_items, first, h->um_time, h->um_count, h->Wn, h->H, h->ratio, h->partial, h->L,
                               h->LK, h->K32, h->Np, h->PADL);
    }));
    h->ratio_passes += 1;
    h->ratio_valid = true;
    return CMF_OK;
}

template <int Q>
static void ev_launch_numw(cmf_events_s *h, int first, unsigned n)
{
    hipLaunchKernelGGL(ev_numw_kernel<Q>, dim3(n), dim3(256), 0, h->stream, h->u_items, first, h->um_time, h->ratio, h->H, h->numW, h->u_slabs, h->L, h->LK, h->K32, h->Np,
                       h->PADL);
}

static int ev_num_w(cmf_events_s *h)
{
    const int Q = (h->LK + 255) / 256; // accumulators per thread: the next of 1, 2, 4, 8, 16
    auto launch = [&](int first, unsigned n) {
        if (Q <= 1) ev_launch_numw<1>(h, first, n);
        else if (Q <= 2) ev_launch_numw<2>(h, first, n);
        else if (Q <= 4) ev_launch_numw<4>(h, first, n);
        else if (Q <= 8) ev_launch_numw<8>(h, first, n);
        else ev_launch_numw<16>(h, first, n);
    };
    CMFTRY(ev_for_pieces(h, h->n_u_items, "ev_numw_kernel", launch));
    return ev_for_pieces(h, h->n_u_fixes, "ev_numw_fix_kernel", [&](int first, unsigned n) {
        hipLaunchKernelGGL(ev_numw_fix_kernel, dim3(n), dim3(256), 0, h->stream, h->u_fixes, first, h->u_slabs, h->numW, h->L, h->LK, h->K32, h->Np);
    });
}

static int ev_num_h(cmf_events_s *h)
{
    const int G = 256 / h->K32;
    CMFTRY(ev_for_pieces(h, h->n_t_items, "ev_numh_kernel", [&](int first, unsigned n) {
        hipLaunchKernelGGL(ev_numh_kernel, dim3(n), dim3(256), 0, h->stream, h->t_items, first, h->tm_unit, h->tm_time, h->tm_src, h->ratio, h->Wn, h->numH, h->t_slabs,
                           h->K32, h->Np, G);
    }));
    return ev_for_pieces(h, h->n_t_fixes, "ev_numh_fix_kernel", [&](int first, unsigned n) {
        hipLaunchKernelGGL(ev_numh_fix_kernel, dim3(n), dim3(256), 0, h->stream, h->t_fixes, first, h->t_slabs, h->numH, h->K32);
    });
}

// denomW[l][k][0 .. Np) = sum(H[k, 1:T-l]) (kl_hsum_kernel, kl_den_w_kernel: the dense rule's launches)
static int ev_den_w(cmf_events_s *h)
{
    hipLaunchKernelGGL(kl_hsum_kernel, dim3(h->K, KL_HCHUNKS), dim3(256), 0, h->stream, h->Ht, h->TP, h->PADL, h->T, h->hsums);
    KCHK("kl_hsum_kernel");
    hipLaunchKernelGGL(kl_den_w_kernel, dim3(h->L, h->K), dim3(256), 0, h->stream, h->Ht, h->hsums, h->denW, h->TP, h->PADL, h->T, h->K32, h->Np);
    KCHK("kl_den_w_kernel");
    h->launches += 2;
    return CMF_OK;
}

// denomH[t][k] from the sums of W over n (kl_wsum_kernel, kl_den_h_kernel)
static int ev_den_h(cmf_events_s *h)
{
    const size_t TK = (size_t)h->T * h->K32;
    hipLaunchKernelGGL(kl_wsum_kernel, dim3(h->L, h->K), dim3(256), 0, h->stream, h->Wt, h->K32, h->Np, h->wsums);
    KCHK("kl_wsum_kernel");
    hipLaunchKernelGGL(kl_den_h_kernel, dim3((unsigned)((TK + 255) / 256)), dim3(256), 0, h->stream, h->wsums, h->denH, h->T, h->K, h->K32, h->L);
    KCHK("kl_den_h_kernel");
    h->launches += 2;
    return CMF_OK;
}

// update_motifs! (mult.jl:23-39 with data -> R at the events): the ratio unless the loss pass left it, numW, denomW, mult.jl:37-38
static int ev_w_phase(cmf_events_s *h, double l1W, double l2W)
{
    if (!(h->keep_ratio && h->ratio_valid)) CMFTRY(ev_ratio(h, false));
    CMFTRY(ev_num_w(h));
    CMFTRY(ev_den_w(h));
    hipLaunchKernelGGL(w_update_kernel, dim3(h->Np / 64, h->KB, h->L), dim3(256), 0, h->stream, h->Wt, h->Wn, h->numW, h->denW, h->N, h->K, h->L, h->Np, h->K32,
                       (float)l1W, (float)(2.0 * l2W), (const float *)nullptr, (float *)nullptr, 0);
    KCHK("w_update_kernel");
    h->launches += 1;
    h->ratio_valid = false;
    return CMF_OK;
}

// the loss of the resident factors -> *dst (device); the ratio it leaves belongs to them
static int ev_loss(cmf_events_s *h, double *dst, bool wsums_current)
{
    CMFTRY(ev_ratio(h, true));
    hipLaunchKernelGGL(kl_hsum_kernel, dim3(h->K, KL_HCHUNKS), dim3(256), 0, h->stream, h->Ht, h->TP, h->PADL, h->T, h->hsums);
    KCHK("kl_hsum_kernel");
    h->launches += 1;
    if (!wsums_current) {
        hipLaunchKernelGGL(kl_wsum_kernel, dim3(h->L, h->K), dim3(256), 0, h->stream, h->Wt, h->K32, h->Np, h->wsums);
        KCHK("kl_wsum_kernel");
        h->launches += 1;
    }
    hipLaunchKernelGGL(ev_loss_kernel, dim3(1), dim3(256), 0, h->stream, h->partial, (int)h->n_u_items, h->wsums, h->hsums, h->Ht, h->TP, h->PADL, h->T, h->N, h->K, h->K32,
                       h->L, h->count_sum, dst);
    KCHK("ev_loss_kernel");
    h->launches += 1;
    return CMF_OK;
}

// update_feature_maps! (mult.jl:42-58): the ratio from the new W, numH, denomH, mult.jl:51-52, then the loss from the new W and H
static int ev_h_phase(cmf_events_s *h, double l1H, double l2H, double *loss_dst)
{
    if (!(h->keep_ratio && h->ratio_valid)) CMFTRY(ev_ratio(h, false)); // (eval_mode: the loss pass of the iteration before left it)
    CMFTRY(ev_num_h(h));
    CMFTRY(ev_den_h(h));
    hipLaunchKernelGGL(h_update_kernel, dim3((h->T + HUPD_T - 1) / HUPD_T, h->KB), dim3(256), 0, h->stream, h->H, h->Ht, h->numH, (size_t)0, 1, h->denH, (size_t)0, 1, h->T,
                       h->K, h->K32, h->PADL, h->TP, (float)l1H, (float)(2.0 * l2H));
    KCHK("h_update_kernel");
    h->launches += 1;
    h->ratio_valid = false;
    return ev_loss(h, loss_dst, true);
}

static int ev_read(cmf_events_s *h, const double *src, double *dst, size_t n)
{
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CMF_OK;
}

// ------------------------------------------------------------------------------------------
// the C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int cmf_events_create(cmf_events *out, int device, int64_t N, int64_t T, int64_t K, int64_t L, int64_t nnz, const int32_t *unit, const int32_t *time,
                      const double *count)
{
    if (!out) return fail(CMF_ERR_ARG, "NULL argument: the handle's address");
    *out = nullptr;
    std::string msg;
    const int bad = cmf_events_validate(N, T, K, L, nnz, unit, time, count, &msg); // (before anything touches a device)
    if (bad) return fail(bad == 1 ? CMF_ERR_ARG : CMF_ERR_UNSUPPORTED, "cmf_events_create: %s", msg.c_str());
    cmf_events_s *h = new cmf_events_s();
    h->N = (int)N; h->T = (int)T; h->K = (int)K; h->L = (int)L; h->nnz = nnz;
    h->Np = (int)rup(N, 128);
    h->KB = (int)((K + 31) / 32);
    h->K32 = 32 * h->KB;
    h->PADL = (int)rup(L - 1, 32) + 32;
    h->TP = h->PADL + (int)rup(T + L, 512) + 256;
    h->Lp = L <= 32 ? (int)rup(L, 4) : (int)rup(L, 32);
    h->LK = h->L * h->K32;
    if ((double)h->Lp * h->Np * h->K32 * 4.0 >= 2147483648.0 || (double)h->TP * h->K32 * 4.0 >= 2147483648.0) {
        delete h;
        return fail(CMF_ERR_UNSUPPORTED, "cmf_events_create: W (L*N*K) or H (T*K) exceeds 2 GiB in its padded fp32 layout");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        delete h;
        return fail(CMF_ERR_HIP, "no HIP device available (libcmf_hip has no CPU fallback)");
    }
    if (device < 0 || device >= ndev) {
        delete h;
        return fail(CMF_ERR_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    }
    h->device = device;
    auto body = [&]() -> int {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        CmfEventsIndex ix;
        cmf_events_build_index(N, T, nnz, unit, time, count, &ix);
        h->count_sum = ix.count_sum;
        CMFTRY(ev_alloc(h, &h->H, (size_t)h->TP * h->K32));
        CMFTRY(ev_alloc(h, &h->Ht, (size_t)h->K32 * h->TP));
        CMFTRY(ev_alloc(h, &h->Wt, (size_t)h->Lp * h->K32 * h->Np));
        CMFTRY(ev_alloc(h, &h->Wn, (size_t)h->Lp * h->Np * h->K32));
        CMFTRY(ev_alloc(h, &h->numW, (size_t)h->L * h->K32 * h->Np));
        CMFTRY(ev_alloc(h, &h->denW, (size_t)h->L * h->K32 * h->Np));
        CMFTRY(ev_alloc(h, &h->numH, (size_t)h->T * h->K32));
        CMFTRY(ev_alloc(h, &h->denH, (size_t)h->T * h->K32));
        CMFTRY(ev_alloc(h, &h->hsums, (size_t)h->K32 * KL_HCHUNKS));
        CMFTRY(ev_alloc(h, &h->wsums, (size_t)h->L * h->K32));
        CMFTRY(ev_alloc(h, &h->d_loss, (size_t)1));
        CMFTRY(ev_alloc(h, &h->ratio, (size_t)nnz));
        CMFTRY(ev_upload(h, &h->um_time, ix.um_time));
        CMFTRY(ev_upload(h, &h->um_count, ix.um_count));
        CMFTRY(ev_upload(h, &h->tm_unit, ix.tm_unit));
        CMFTRY(ev_upload(h, &h->tm_time, ix.tm_time));
        CMFTRY(ev_upload(h, &h->tm_src, ix.tm_src));
        h->unit_ptr.swap(ix.unit_ptr);
        h->time_ptr.swap(ix.time_ptr);
        return ev_build_tables(h);
    };
    const int rc = body();
    if (rc != CMF_OK) {
        ev_destroy(h);
        return rc;
    }
    *out = h;
    return CMF_OK;
}

int cmf_events_destroy(cmf_events h) { return ev_destroy(h); }

int cmf_events_set_factors(cmf_events h, const double *W, const double *H)
{
    if (!h || !W || !H) return fail(CMF_ERR_ARG, "NULL argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t nW = (size_t)h->L * h->N * h->K, nH = (size_t)h->T * h->K;
    CMFTRY(ev_ensure_stage(h, std::max(nW, nH)));
    // padding must be zero: clear, then scatter the valid entries
    HIPCHK(hipMemsetAsync(h->Wt, 0, (size_t)h->Lp * h->K32 * h->Np * sizeof(float), h->stream));
    HIPCHK(hipMemsetAsync(h->Wn, 0, (size_t)h->Lp * h->Np * h->K32 * sizeof(float), h->stream));
    HIPCHK(hipMemcpyAsync(h->stage, W, nW * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(pack_W_kernel, dim3(1024), dim3(256), 0, h->stream, h->stage, h->N, h->K, h->L, h->Wt, h->Wn, h->Np, h->K32);
    KCHK("pack_W_kernel");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemsetAsync(h->H, 0, (size_t)h->TP * h->K32 * sizeof(float), h->stream));
    HIPCHK(hipMemsetAsync(h->Ht, 0, (size_t)h->K32 * h->TP * sizeof(float), h->stream));
    HIPCHK(hipMemcpyAsync(h->stage, H, nH * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(pack_H_kernel, dim3(1024), dim3(256), 0, h->stream, h->stage, h->T, h->K, h->H, h->Ht, h->K32, h->TP, h->PADL);
    KCHK("pack_H_kernel");
    HIPCHK(hipStreamSynchronize(h->stream));
    h->launches += 2;
    h->factors_set = true;
    h->ratio_valid = false;
    return CMF_OK;
}

int cmf_events_get_factors(cmf_events h, double *W, double *H)
{
    CMFTRY(ev_ready(h));
    const size_t nW = (size_t)h->L * h->N * h->K, nH = (size_t)h->T * h->K;
    CMFTRY(ev_ensure_stage(h, std::max(nW, nH)));
    if (W) {
        hipLaunchKernelGGL(unpack_W_kernel<double>, dim3(1024), dim3(256), 0, h->stream, h->stage, h->N, h->K, h->L, h->Wn, h->Np, h->K32);
        KCHK("unpack_W_kernel");
        CMFTRY(ev_read(h, h->stage, W, nW));
    }
    if (H) {
        hipLaunchKernelGGL(unpack_H_kernel<double>, dim3(1024), dim3(256), 0, h->stream, h->stage, h->T, h->K, h->H, h->K32, h->PADL);
        KCHK("unpack_H_kernel");
        CMFTRY(ev_read(h, h->stage, H, nH));
    }
    return CMF_OK;
}

int cmf_events_update_motifs(cmf_events h, double l1W, double l2W)
{
    CMFTRY(ev_ready(h));
    return ev_w_phase(h, l1W, l2W);
}

int cmf_events_update_feature_maps(cmf_events h, double l1H, double l2H, double *loss)
{
    CMFTRY(ev_ready(h));
    CMFTRY(ev_h_phase(h, l1H, l2H, h->d_loss));
    double v = 0.0;
    CMFTRY(ev_read(h, h->d_loss, &v, 1)); // (synchronises, like the dense entry)
    if (loss) *loss = v;
    return CMF_OK;
}

int cmf_events_compute_loss(cmf_events h, double *loss)
{
    CMFTRY(ev_ready(h));
    if (!loss) return fail(CMF_ERR_ARG, "NULL argument");
    CMFTRY(ev_loss(h, h->d_loss, false));
    return ev_read(h, h->d_loss, loss, 1);
}

int cmf_events_iterate(cmf_events h, int64_t n_iter, int eval_mode, double l1W, double l2W, double l1H, double l2H, double *loss_hist)
{
    CMFTRY(ev_ready(h));
    if (n_iter < 0) return fail(CMF_ERR_ARG, "n_iter must be >= 0 (got %lld)", (long long)n_iter);
    if (n_iter == 0) return CMF_OK;
    if (h->hist_elems < (size_t)n_iter) {
        if (h->d_hist) HIPCHK(hipFree(h->d_hist));
        h->d_hist = nullptr;
        h->device_bytes -= (int64_t)(h->hist_elems * sizeof(double));
        h->hist_elems = 0;
        HIPCHK(hipMalloc(&h->d_hist, (size_t)n_iter * sizeof(double)));
        h->hist_elems = (size_t)n_iter;
        h->device_bytes += (int64_t)(h->hist_elems * sizeof(double));
    }
    for (int64_t it = 0; it < n_iter; ++it) { // (everything enqueued; the host waits once, at the end)
        if (!eval_mode) CMFTRY(ev_w_phase(h, l1W, l2W));
        CMFTRY(ev_h_phase(h, l1H, l2H, h->d_hist + it));
    }
    if (loss_hist) return ev_read(h, h->d_hist, loss_hist, (size_t)n_iter);
    HIPCHK(hipStreamSynchronize(h->stream));
    return CMF_OK;
}

int cmf_events_terms(cmf_events h, double *ratio, double *numW, double *numH, double *denomW, double *denomH)
{
    CMFTRY(ev_ready(h));
    const size_t nW = (size_t)h->L * h->N * h->K, nH = (size_t)h->T * h->K;
    CMFTRY(ev_ensure_stage(h, std::max(std::max(nW, nH), (size_t)h->nnz)));
    CMFTRY(ev_ratio(h, false)); // every term from the resident W, H
    if (ratio) {
        hipLaunchKernelGGL(ev_widen_kernel, dim3(1024), dim3(256), 0, h->stream, h->stage, h->ratio, (size_t)h->nnz);
        KCHK("ev_widen_kernel");
        CMFTRY(ev_read(h, h->stage, ratio, (size_t)h->nnz));
    }
    if (numW || denomW) {
        CMFTRY(ev_num_w(h));
        CMFTRY(ev_den_w(h));
        for (int which = 0; which < 2; ++which) {
            double *dst = which ? denomW : numW;
            if (!dst) continue;
            hipLaunchKernelGGL(ev_unpack_wt_kernel, dim3(1024), dim3(256), 0, h->stream, h->stage, h->N, h->K, h->L, which ? h->denW : h->numW, h->Np, h->K32);
            KCHK("ev_unpack_wt_kernel");
            CMFTRY(ev_read(h, h->stage, dst, nW));
        }
    }
    if (numH || denomH) {
        CMFTRY(ev_num_h(h));
        CMFTRY(ev_den_h(h));
        for (int which = 0; which < 2; ++which) {
            double *dst = which ? denomH : numH;
            if (!dst) continue;
            hipLaunchKernelGGL(unpack_H_kernel<double>, dim3(1024), dim3(256), 0, h->stream, h->stage, h->T, h->K, which ? h->denH : h->numH, h->K32, 0);
            KCHK("unpack_H_kernel");
            CMFTRY(ev_read(h, h->stage, dst, nH));
        }
    }
    return CMF_OK;
}

int cmf_events_set_option(cmf_events h, const char *name, int value)
{
    if (!h || !name) return fail(CMF_ERR_ARG, "NULL argument");
    const std::string nm(name);
    if (nm == "keep_ratio") {
        if (value != 0 && value != 1) return fail(CMF_ERR_ARG, "keep_ratio must be 0 or 1 (got %d)", value);
        h->keep_ratio = value;
        h->ratio_valid = false;
        return CMF_OK;
    }
    if (nm != "unit_chunk" && nm != "time_chunk") return fail(CMF_ERR_ARG, "unknown option \"%s\" (an event handle has unit_chunk, time_chunk, keep_ratio)", name);
    if (value < 1) return fail(CMF_ERR_ARG, "%s must be at least 1 (got %d)", name, value);
    HIPCHK(hipSetDevice(h->device));
    int &slot = nm == "unit_chunk" ? h->unit_chunk : h->time_chunk;
    const int old = slot;
    if (old == value) return CMF_OK;
    slot = value;
    const int rc = ev_build_tables(h);
    if (rc == CMF_ERR_UNSUPPORTED) { // (refused before the tables in place were touched)
        slot = old;
        return rc;
    }
    return rc;
}

static const CounterRow<cmf_events_s> kEventCounters[] = {
    CMF_COUNTER_ROW("device_bytes", h->device_bytes, 0), CMF_COUNTER_ROW("launches", h->launches, 0), CMF_COUNTER_ROW("ratio_passes", h->ratio_passes, 0), CMF_COUNTER_ROW("nnz", h->nnz, 0),
    CMF_COUNTER_ROW("unit_chunk", h->unit_chunk, 0), CMF_COUNTER_ROW("time_chunk", h->time_chunk, 0), CMF_COUNTER_ROW("keep_ratio", h->keep_ratio, 0),
    CMF_COUNTER_ROW("unit_items", h->n_u_items, 0), CMF_COUNTER_ROW("time_items", h->n_t_items, 0), CMF_COUNTER_ROW("unit_split", h->n_u_fixes, 0), CMF_COUNTER_ROW("time_split", h->n_t_fixes, 0),
    CMF_COUNTER_ROW("w_block_units", 64, 0),       // units per workgroup of w_update_kernel
    CMF_COUNTER_ROW("h_block_columns", HUPD_T, 0), // columns per workgroup of h_update_kernel
    CMF_COUNTER_ROW("ratio_waves", 4, 0),          // events a workgroup of ev_ratio_kernel has in flight
};
int cmf_events_get_counter(cmf_events h, const char *name, int64_t *value)
{
    if (!h || !name || !value) return fail(CMF_ERR_ARG, "NULL argument");
    const CounterRow<cmf_events_s> *r = row_named(kEventCounters, name);
    if (!r) return fail(CMF_ERR_ARG, "unknown counter \"%s\"", name);
    *value = r->get(h);
    return CMF_OK;
}

} // extern "C"
