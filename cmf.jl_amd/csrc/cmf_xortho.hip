// cmf_xortho.hip -- seqNMF's cross-orthogonality penalties (Mackevicius et al., eLife 2019) on the squared-error MU rule: the host side of
// cmf_mu_set_xortho / cmf_mu_xortho_cost / cmf_mu_xortho_terms and the two hooks the rule calls (w_phase_impl, h_update_impl in cmf_api.hip).
// The kernels are in cmf_xortho.h; the penalty contraction is the C2 kernel with G = off(S(H)) in H's place (hxt_contract's left operand).
#include "cmf_internal.h"
#include "cmf_xortho.h"

struct XoState {
    float *G = nullptr, *Gt = nullptr; // off(S(H)) in the layouts of H [TP][K32] and Ht [K32][TP]: padding rows and columns k >= K are exact zeros
    float *S = nullptr;                // [Tl][K32]: a window sum on its way into off
    float *AD = nullptr;               // [2][Tl][K32]: the summed slabs of the C3 contraction (numH and denomH in the order of the form)
    float *den = nullptr;              // [Tl][K32]: the finished denominator of H
    float *xH = nullptr;               // [Tl][K32]: off(S(numH)) for cmf_mu_xortho_terms
    float *xW = nullptr;               // [L][K32][Np]: the penalty contraction (G, data)
    float *Wf = nullptr, *oW = nullptr; // [K32][Np]: Wflat and off(Wflat)
    double *partial = nullptr;         // [XO_NPART]: block sums of a cost
    int64_t g_gen = -1;                // est_gen for which G belongs to the resident H (set_est counts every change of H)
    bool w_g = false;                  // the W side of the call in flight made G current
};

void xo_free(cmf_handle_s *h)
{
    if (!h->xo) return;
    XoState *x = h->xo;
    for (float *p : {x->G, x->Gt, x->S, x->AD, x->den, x->xH, x->xW, x->Wf, x->oW})
        if (p) (void)hipFree(p);
    if (x->partial) (void)hipFree(x->partial);
    delete x;
    h->xo = nullptr;
}

static int xo_ensure(cmf_handle_s *h)
{
    if (h->xo) return CMF_OK;
    const CmfDims &d = h->d;
    const size_t TK = (size_t)d.Tl * d.K32, KN = (size_t)d.K32 * d.Np;
    h->xo = new XoState();
    XoState *x = h->xo;
    int rc = dalloc_zero(&x->G, (size_t)d.TP * d.K32);
    if (rc == CMF_OK) rc = dalloc_zero(&x->Gt, (size_t)d.K32 * d.TP);
    if (rc == CMF_OK) rc = dalloc_zero(&x->S, TK);
    if (rc == CMF_OK) rc = dalloc_zero(&x->AD, 2 * TK);
    if (rc == CMF_OK) rc = dalloc_zero(&x->den, TK);
    if (rc == CMF_OK) rc = dalloc_zero(&x->xH, TK);
    if (rc == CMF_OK) rc = dalloc_zero(&x->xW, (size_t)d.L * KN);
    if (rc == CMF_OK) rc = dalloc_zero(&x->Wf, KN);
    if (rc == CMF_OK) rc = dalloc_zero(&x->oW, KN);
    if (rc == CMF_OK) rc = dalloc_zero(&x->partial, (size_t)XO_NPART);
    if (rc != CMF_OK) xo_free(h);
    return rc;
}

// out = S(in) on [Tl][K32] tables
static int xo_window(cmf_handle_s *h, const float *in, float *out)
{
    const CmfDims &d = h->d;
    hipLaunchKernelGGL(xo_window_kernel, dim3((d.Tl + XO_WIN_T - 1) / XO_WIN_T, d.KB), dim3(256), 0, h->stream, in, out, d.Tl, d.K32, d.L);
    KCHK("xo_window_kernel");
    h->xo_launches += 1;
    return CMF_OK;
}

static int xo_off(cmf_handle_s *h, const float *in, float *out, float *outT, const float *base, const float *g, double lam, double lam2)
{
    const CmfDims &d = h->d;
    hipLaunchKernelGGL(xo_off_kernel, dim3((d.Tl + XO_OFF_T - 1) / XO_OFF_T), dim3(256), 0, h->stream, in, out, outT, d.TP, d.Tl, d.K, d.K32, base, g, (float)lam,
                       (float)lam2);
    KCHK("xo_off_kernel");
    h->xo_launches += 1;
    return CMF_OK;
}

// G = off(S(H)) of the resident H, in both layouts; nothing when it is current
static int xo_ensure_G(cmf_handle_s *h)
{
    XoState *x = h->xo;
    const CmfDims &d = h->d;
    if (x->g_gen == h->est_gen) return CMF_OK;
    CMFTRY(xo_window(h, h->H + (size_t)d.PADL * d.K32, x->S));
    CMFTRY(xo_off(h, x->S, x->G + (size_t)d.PADL * d.K32, x->Gt + d.PADL, nullptr, nullptr, 0.0, 0.0));
    x->g_gen = h->est_gen;
    return CMF_OK;
}

// oW = off(Wflat) of the resident W (and Wflat itself)
static int xo_off_w(cmf_handle_s *h)
{
    XoState *x = h->xo;
    const CmfDims &d = h->d;
    hipLaunchKernelGGL(xo_wflat_kernel, dim3(d.Np / 128, d.K), dim3(128), 0, h->stream, h->Wt, x->Wf, d.L, d.K32, d.Np);
    KCHK("xo_wflat_kernel");
    hipLaunchKernelGGL(xo_off_w_kernel, dim3(d.Np / 128), dim3(128), 0, h->stream, x->Wf, x->oW, d.K, d.Np);
    KCHK("xo_off_w_kernel");
    h->xo_launches += 2;
    return CMF_OK;
}

// xW[l][k][n] = sum_t G[t - l][k] data[t][n]: ONE one-source C2 contraction with G as the left operand (mult.jl:32 with G in H's place).
// Its slab sum takes no deferred loss: the contraction of the rule in front of it has taken it.
static int xo_contract_w(cmf_handle_s *h)
{
    XoState *x = h->xo;
    CMFTRY(xo_ensure_G(h));
    return hxt_contract(h, h->X, h->X, 1, x->xW, false, false, x->G, x->Gt);
}

int xo_fold_w(cmf_handle_s *h)
{
    CMFTRY(xo_ensure(h));
    XoState *x = h->xo;
    const CmfDims &d = h->d;
    const double lam = h->xo_lam[0], lamW = h->xo_lam[2];
    x->w_g = false;
    if (lam == 0.0 && lamW == 0.0) return CMF_OK; // (lambda_H alone: nothing on this side)
    if (lam > 0.0) {
        CMFTRY(xo_contract_w(h));
        x->w_g = true;
    }
    if (lamW > 0.0) CMFTRY(xo_off_w(h));
    const size_t KN4 = (size_t)d.K32 * d.Np / 4, n4 = (size_t)d.L * KN4;
    // (a weight of 0 multiplies a table that is allocated, finite and possibly stale: exactly 0)
    hipLaunchKernelGGL(xo_fold_w_kernel, dim3((unsigned)std::min<size_t>(2048, (n4 + 255) / 256)), dim3(256), 0, h->stream, h->numden + (size_t)d.L * d.K32 * d.Np, x->xW,
                       x->oW, n4, KN4, (float)lam, (float)lamW);
    KCHK("xo_fold_w_kernel");
    h->xo_launches += 1;
    return CMF_OK;
}

void xo_after_w(cmf_handle_s *h) // W has changed, H has not: G stays the table of the resident H
{
    if (h->xo && h->xo->w_g) h->xo->g_gen = h->est_gen;
    if (h->xo) h->xo->w_g = false;
}

int xo_h_tables(cmf_handle_s *h, int nslabs, size_t stride, int num_pos, int den_pos, const float **num, const float **den)
{
    CMFTRY(xo_ensure(h));
    XoState *x = h->xo;
    const CmfDims &d = h->d;
    const size_t TK = (size_t)d.Tl * d.K32;
    if (stride != 2 * TK || num_pos < 0 || num_pos > 1 || den_pos < 0 || den_pos > 1) return fail(CMF_ERR_STATE, "internal: the penalties need the two-source C3 slabs");
    const double lam = h->xo_lam[0], lamH = h->xo_lam[1];
    CMFTRY(launch_slab_sum(h, x->AD, h->hslabs, nslabs, stride)); // the slabs in slab order (slab_sum_kernel): numH | denomH finished
    const float *A = x->AD + (size_t)num_pos * TK, *D = x->AD + (size_t)den_pos * TK;
    *num = A;
    *den = D;
    if (lam == 0.0 && lamH == 0.0) return CMF_OK; // (lambda_W alone: nothing on this side)
    if (lamH > 0.0) CMFTRY(xo_ensure_G(h)); // (first: it passes S(H) through x->S, which S(numH) takes next)
    if (lam > 0.0) CMFTRY(xo_window(h, A, x->S));
    // denomH + (lambda off(S(numH)) + lambda_H G)   (a weight of 0 multiplies a finite table: exactly 0)
    CMFTRY(xo_off(h, x->S, x->den, nullptr, D, x->G + (size_t)d.PADL * d.K32, lam, lamH));
    *den = x->den;
    return CMF_OK;
}

// ---- the C ABI ----
static int xo_entry_ready(cmf_handle_s *h, const char *what)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    if (h->group || h->root_only || h->sharded)
        return fail(CMF_ERR_UNSUPPORTED, "%s runs on a single-GPU handle: T-sharded groups (cmf_create_multi, cmf_create_shard) are not supported", what);
    HIPCHK(hipSetDevice(h->device));
    return CMF_OK;
}

int cmf_mu_set_xortho(cmf_handle h, double lambda_xortho, double lambda_ortho_H, double lambda_ortho_W)
{
    if (!h) return fail(CMF_ERR_ARG, "handle is NULL");
    const double w[3] = {lambda_xortho, lambda_ortho_H, lambda_ortho_W};
    const char *const names[3] = {"lambda_xortho", "lambda_ortho_H", "lambda_ortho_W"};
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) return fail(CMF_ERR_ARG, "%s must be finite and >= 0, got %g", names[i], w[i]);
    const bool any = w[0] > 0.0 || w[1] > 0.0 || w[2] > 0.0;
    if (any) {
        if (h->group || h->root_only || h->sharded)
            return fail(CMF_ERR_UNSUPPORTED, "the cross-orthogonality penalties run on a single-GPU handle: T-sharded groups (cmf_create_multi, cmf_create_shard) are not supported");
        CMFTRY(mu_ask(h, MuAsk{MU_ASK_SET_XORTHO})); // (under a mask, a divergence or the Gram forms: cmf_mu_install.h)
        HIPCHK(hipSetDevice(h->device));
        CMFTRY(xo_ensure(h));
    }
    if (w[0] == h->xo_lam[0] && w[1] == h->xo_lam[1] && w[2] == h->xo_lam[2]) return CMF_OK;
    // a speculated contraction and a deferred loss belong to the path the handle leaves (the weights change which launches follow);
    // est itself stays what it is: the penalties do not enter it
    if (h->carry.partial) {
        (void)hipSetDevice(h->device);
        HIPCHK(hipStreamSynchronize(h->stream));
        h->carry = CmfLossCarry{};
    }
    h->spec_gen = -1;
    for (int i = 0; i < 3; ++i) h->xo_lam[i] = w[i];
    return CMF_OK;
}

static int xo_terms_ready(cmf_handle_s *h, const char *what)
{
    CMFTRY(xo_entry_ready(h, what));
    if (!h->factors_set) return fail(CMF_ERR_STATE, "factors not set: call cmf_set_factors first");
    if (!h->have_data) return fail(CMF_ERR_STATE, "handle was created without data");
    return xo_ensure(h);
}

// A = transconv(W, data) of the resident W as a finished table (x->AD): one one-source C3 contraction and its slab sum
static int xo_transconv_data(cmf_handle_s *h)
{
    const CmfDims &d = h->d;
    CMFTRY(launch_transconv(h, 1, h->XT));
    return launch_slab_sum(h, h->xo->AD, h->hslabs, h->tc_S1, (size_t)d.Tl * d.K32);
}

static int xo_dot(cmf_handle_s *h, const float *a, const float *b, size_t n, double *out)
{
    XoState *x = h->xo;
    const int nb = (int)std::min<size_t>(XO_NPART, (n + 255) / 256);
    hipLaunchKernelGGL(xo_dot_kernel, dim3(nb), dim3(256), 0, h->stream, a, b, n, x->partial);
    KCHK("xo_dot_kernel");
    h->xo_launches += 1;
    std::vector<double> part((size_t)nb);
    HIPCHK(hipMemcpyAsync(part.data(), x->partial, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (double v : part) s += v;
    *out = s;
    return CMF_OK;
}

int cmf_mu_xortho_cost(cmf_handle h, double *xortho, double *ortho_H, double *ortho_W)
{
    CMFTRY(xo_terms_ready(h, "cmf_mu_xortho_cost"));
    XoState *x = h->xo;
    const CmfDims &d = h->d;
    const size_t TK = (size_t)d.Tl * d.K32;
    const float *Grows = x->G + (size_t)d.PADL * d.K32;
    if (xortho || ortho_H) CMFTRY(xo_ensure_G(h));
    if (xortho) { // sum_{i != j} (A S H')_ij = sum_{k,t} A[k][t] G[k][t]
        CMFTRY(xo_transconv_data(h));
        CMFTRY(xo_dot(h, x->AD, Grows, TK, xortho));
    }
    if (ortho_H) CMFTRY(xo_dot(h, h->H + (size_t)d.PADL * d.K32, Grows, TK, ortho_H)); // sum_{i != j} (H S H')_ij
    if (ortho_W) { // sum_{i != j} (Wflat' Wflat)_ij
        CMFTRY(xo_off_w(h));
        CMFTRY(xo_dot(h, x->Wf, x->oW, (size_t)d.K32 * d.Np, ortho_W));
    }
    return CMF_OK;
}

// a [rows][K32] table -> the caller's K x rows array (k fastest); a [L][K32][Np] table -> the caller's K x N x L array
static int xo_download(cmf_handle_s *h, const float *tbl, size_t count, std::vector<float> &host)
{
    host.resize(count);
    HIPCHK(hipMemcpyAsync(host.data(), tbl, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CMF_OK;
}

int cmf_mu_xortho_terms(cmf_handle h, double *xW, double *xH, double *oH, double *oW)
{
    CMFTRY(xo_terms_ready(h, "cmf_mu_xortho_terms"));
    XoState *x = h->xo;
    const CmfDims &d = h->d;
    const size_t TK = (size_t)d.Tl * d.K32, KN = (size_t)d.K32 * d.Np;
    std::vector<float> host;
    auto h_shaped = [&](const float *tbl, double *out) -> int {
        CMFTRY(xo_download(h, tbl, TK, host));
        for (int t = 0; t < d.Tl; ++t)
            for (int k = 0; k < d.K; ++k) out[(size_t)t * d.K + k] = (double)host[(size_t)t * d.K32 + k];
        return CMF_OK;
    };
    if (xW) {
        CMFTRY(xo_contract_w(h));
        CMFTRY(xo_download(h, x->xW, (size_t)d.L * KN, host));
        for (int l = 0; l < d.L; ++l)
            for (int n = 0; n < d.N; ++n)
                for (int k = 0; k < d.K; ++k) xW[((size_t)l * d.N + n) * d.K + k] = (double)host[((size_t)l * d.K32 + k) * d.Np + n];
    }
    if (xH) {
        CMFTRY(xo_transconv_data(h));
        CMFTRY(xo_window(h, x->AD, x->S));
        CMFTRY(xo_off(h, x->S, x->xH, nullptr, nullptr, nullptr, 0.0, 0.0));
        CMFTRY(h_shaped(x->xH, xH));
    }
    if (oH) {
        CMFTRY(xo_ensure_G(h));
        CMFTRY(h_shaped(x->G + (size_t)d.PADL * d.K32, oH));
    }
    if (oW) {
        CMFTRY(xo_off_w(h));
        CMFTRY(xo_download(h, x->oW, KN, host));
        for (int l = 0; l < d.L; ++l)
            for (int n = 0; n < d.N; ++n)
                for (int k = 0; k < d.K; ++k) oW[((size_t)l * d.N + n) * d.K + k] = (double)host[(size_t)k * d.Np + n];
    }
    return CMF_OK;
}
