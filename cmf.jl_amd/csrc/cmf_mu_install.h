// cmf_mu_install.h -- how a form of the MU rule is installed, left or refused, stated once and free of HIP (like cmf_events.h), so that a
// stand-alone program can walk it (tests/mu_install_matrix.cpp).  kMuForms (cmf_internal.h) says how a form RUNS; kMuDivs below says
// what a divergence needs to be INSTALLED, with and without a mask, and mu_refusal says when a request is answered with a code instead
// of device work.  mu_set_form (cmf_api.hip) is the one transition that reads both.  A new divergence: a row in kMuDivs; a new thing
// that cannot live beside a form: a line in mu_refusal.
#pragma once
#include "cmf_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

// mu_div of a handle under cmf_mu_set_beta_divergence: behind the kinds of cmf_mu_set_divergence, which does not take it
#define CMF_DIV_BETA 3

enum MuDataRule { MU_DATA_ANY, MU_DATA_POSITIVE_SUM, MU_DATA_STRICT, MU_DATA_NONNEG }; // -, finite and >= 0 with a sum > 0, finite and > 0, finite and >= 0
enum : unsigned { MU_BUF_KL = 1, MU_BUF_EST2 = 2, MU_BUF_XM = 4, MU_BUF_XS = 8 };   // kl_denH / kl_sums, est2 / est2T, Xm / XmT, Xs / XsT
struct MuDivRow {
    const char *form, *noun, *setter; // in messages: "no KL form", "the KL divergence is installed", the call that installs it
    const char *gate, *mask_gate;     // the option that must be on to take the kind / to have it together with a mask (nullptr: none)
    int data_rule;                    // what the data it reads must be (under a mask: where observed)
    bool count_norm;                  // data_sum holds the entry count (under a mask: the observed count) instead of the sum
    unsigned bufs, bufs_masked;       // what mu_set_form ensures without / with a mask; what a row does not list goes (est2 stays until the handle goes)
    const char *bad_data;             // the data check's text (one %.0f: the offending entries)
};
constexpr MuDivRow kMuDivs[4] = { // (indexed by CMF_DIV_*)
    {"squared-error", "squared error", "cmf_mu_set_divergence", nullptr, nullptr, MU_DATA_ANY, false, 0, MU_BUF_XM, ""},
    {"KL", "KL divergence", "cmf_mu_set_divergence", nullptr, "kl_mask", MU_DATA_POSITIVE_SUM, false, MU_BUF_KL, MU_BUF_KL | MU_BUF_XM,
     "the KL divergence needs finite, non-negative data (%.0f entries are negative, NaN or infinite)"},
    {"Itakura-Saito", "Itakura-Saito divergence", "cmf_mu_set_divergence", "is_div", "pq_mask", MU_DATA_STRICT, true, MU_BUF_EST2, MU_BUF_EST2 | MU_BUF_XM | MU_BUF_XS,
     "Itakura-Saito divergence needs finite, strictly positive data (%.0f entries are zero, negative, NaN or infinite): add a small floor to the spectrogram, "
     "e.g. data + 1e-6 * max(data)"},
    {"beta-divergence", "beta-divergence", "cmf_mu_set_beta_divergence", nullptr, "pq_mask", MU_DATA_NONNEG, true, MU_BUF_EST2, MU_BUF_EST2 | MU_BUF_XM | MU_BUF_XS,
     "the beta-divergence needs finite, non-negative data (%.0f entries are negative, NaN or infinite)"},
};

// What a refusal looks at, and what is asked.
struct MuFacts {
    int div; double beta; bool mask;     // the installed form
    int kl_mask, pq_mask, is_div;        // the gate options
    int gram; bool xortho, group, have_data; // option "gram", active weights of cmf_mu_set_xortho, a group / sharded handle, data on the device
    int hals_mask = 0;                   // option "hals_mask": the HALS entries run their imputed form under a mask (last: aggregates that end at have_data leave it 0)
    bool gate(const char *name) const { return !name || (name[0] == 'k' ? kl_mask : name[0] == 'p' ? pq_mask : is_div) != 0; }
};
enum MuAskKind {
    MU_ASK_SET_MASK, MU_ASK_CLEAR_MASK, // cmf_mu_set_mask(mask) / (NULL); value != 0: cmf_set_mask takes the mask for the PGD entries, which has made its own checks
    MU_ASK_SET_KIND, MU_ASK_SET_BETA,   // cmf_mu_set_divergence(kind), cmf_mu_set_beta_divergence(beta)
    MU_ASK_SET_GRAM, MU_ASK_GATE_OFF,   // cmf_set_option("gram", value), cmf_set_option(name, 0) of a gate
    MU_ASK_SQUARE_RULE,                 // a rule that minimises the squared error only is about to run (name: "HALS" has no masked form without option "hals_mask", "PGD" brings its own mask)
    MU_ASK_SET_XORTHO                   // cmf_mu_set_xortho with a weight > 0
};
struct MuAsk { int what; int kind = 0; double beta = 0.0; int value = 0; const char *name = nullptr; };

__attribute__((format(printf, 3, 4))) static inline int mu_refuse(std::string *msg, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *msg = buf;
    return code;
}

// CMF_OK, or the code and the text the request is refused with before anything touches the device.  The order of the lines is the
// precedence among refusals (beta's argument errors come before the group's, the gates' answers before the Gram forms').
static inline int mu_refusal(const MuFacts &f, const MuAsk &q, std::string *msg)
{
    static const char *const way_square = "restore CMF_DIV_SQUARE with cmf_mu_set_divergence first", *const way_unmask = "clear the mask of cmf_mu_set_mask first",
                      *const way_gram = "set gram = 0 first", *const way_xortho = "set the weights to 0 first";
    static const char *const no_groups = "T-sharded groups (cmf_create_multi, cmf_create_shard) are not supported";
    const MuDivRow &cur = kMuDivs[f.div];
    // the templates: what cannot live beside what, and the way out for the side that is being asked for
    auto unmasked_only = [&](const MuDivRow &r, const char *way) { return mu_refuse(msg, CMF_ERR_UNSUPPORTED, "the %s form of the MU rule has no masked form: %s", r.form, way); };
    auto gram_vs_form = [&](const MuDivRow &r, const char *way) {
        return mu_refuse(msg, CMF_ERR_UNSUPPORTED, "the Gram forms (option \"gram\") rewrite the squared-error denominators and have no %s form: %s", r.form, way); };
    auto gram_vs_mask = [&](const char *way) {
        return mu_refuse(msg, CMF_ERR_UNSUPPORTED, "the Gram forms (option \"gram\") have no masked form (the Gram rewriting of the denominators needs mask .* est, which is not a "
                                                   "product of Gram matrices): %s", way); };
    auto xortho_vs = [&](const char *what, const char *way) { return mu_refuse(msg, CMF_ERR_UNSUPPORTED, "the cross-orthogonality penalties of cmf_mu_set_xortho %s: %s", what, way); };
    static const char *const xo_mask = "have no masked form", *const xo_div = "are terms of the squared-error rule and have no divergence form",
                      *const xo_gram = "enter the denominators the Gram forms (option \"gram\") rewrite";
    switch (q.what) {
    case MU_ASK_SET_MASK:
    case MU_ASK_CLEAR_MASK:
        if (q.what == MU_ASK_CLEAR_MASK && q.value) return CMF_OK;
        if (f.group) return mu_refuse(msg, CMF_ERR_UNSUPPORTED, "the masked MU rule runs on a single-GPU handle: %s", no_groups);
        if (!f.have_data) return mu_refuse(msg, CMF_ERR_STATE, "handle was created without data");
        if (q.what == MU_ASK_CLEAR_MASK) return CMF_OK; // (the raw data is checked by the form's rule on the device: CMF_ERR_ARG, the mask stays)
        if (f.div != CMF_DIV_SQUARE && !f.gate(cur.mask_gate)) return unmasked_only(cur, way_square);
        if (f.gram) return gram_vs_mask(way_gram);
        if (f.xortho) return xortho_vs(xo_mask, way_xortho);
        return CMF_OK;
    case MU_ASK_SET_BETA: {
        const double w = CMF_BETA_WINDOW * (1.0 - 1e-9); // the accepted set (include/cmf_hip.h; the window's edges are accepted, whatever rounding made of 1 - 0.01)
        if (!std::isfinite(q.beta)) return mu_refuse(msg, CMF_ERR_ARG, "beta must be finite");
        if (q.beta == 0.0 || q.beta == 1.0)
            return mu_refuse(msg, CMF_ERR_ARG, "beta = %g is CMF_DIV_IS (beta = 0) or CMF_DIV_KL (beta = 1): the beta formula is 0/0 there, use cmf_mu_set_divergence with those kinds", q.beta);
        if (q.beta < 0.0 || q.beta > CMF_BETA_MAX) return mu_refuse(msg, CMF_ERR_ARG, "beta must lie in (0, %g], got %.17g", (double)CMF_BETA_MAX, q.beta);
        if (q.beta < w || std::fabs(q.beta - 1.0) < w)
            return mu_refuse(msg, CMF_ERR_ARG, "beta = %.17g lies within %g of 0 or 1, where the float32 loss loses its digits to the factor 1 / (beta (beta - 1)): use CMF_DIV_IS / "
                                               "CMF_DIV_KL, or a beta at least %g away", q.beta, (double)CMF_BETA_WINDOW, (double)CMF_BETA_WINDOW);
    }
        [[fallthrough]]; // (from here on a kind like the others)
    case MU_ASK_SET_KIND: {
        const int kind = q.what == MU_ASK_SET_BETA ? CMF_DIV_BETA : q.kind;
        // (a kind whose gate is off is answered as it was before the kind existed)
        if (q.what == MU_ASK_SET_KIND && (kind < 0 || kind >= CMF_DIV_BETA || !f.gate(kMuDivs[kind].gate)))
            return mu_refuse(msg, CMF_ERR_ARG, f.is_div ? "kind must be CMF_DIV_SQUARE (0), CMF_DIV_KL (1) or CMF_DIV_IS (2)" : "kind must be CMF_DIV_SQUARE (0) or CMF_DIV_KL (1)");
        const MuDivRow &to = kMuDivs[kind];
        if (f.group) return mu_refuse(msg, CMF_ERR_UNSUPPORTED, "the divergence of the MU rule is chosen on a single-GPU handle: %s", no_groups);
        if (kind == CMF_DIV_SQUARE) return CMF_OK;
        if (f.xortho) return xortho_vs(xo_div, way_xortho);
        if (!f.have_data) return mu_refuse(msg, CMF_ERR_STATE, "handle was created without data");
        if (f.gram) return gram_vs_form(to, way_gram);
        if (f.mask && !f.gate(to.mask_gate)) return unmasked_only(to, way_unmask);
        return CMF_OK;
    }
    case MU_ASK_SET_GRAM:
        if (!q.value) return CMF_OK;
        if (f.div != CMF_DIV_SQUARE) return gram_vs_form(cur, way_square);
        if (f.mask) return gram_vs_mask(way_unmask);
        if (f.xortho) return xortho_vs(xo_gram, way_xortho);
        return CMF_OK;
    case MU_ASK_GATE_OFF: // (a gate cannot go while what it let in is installed; "kl_mask", the first of them, has always held every divergence under a mask)
        if (f.div != CMF_DIV_SQUARE && f.mask && (!std::strcmp(q.name, "kl_mask") || (cur.mask_gate && !std::strcmp(q.name, cur.mask_gate))))
            return mu_refuse(msg, CMF_ERR_STATE, "%s: the %s and a mask are both installed; clear the mask or restore CMF_DIV_SQUARE first", q.name, cur.noun);
        if (cur.gate && !std::strcmp(q.name, cur.gate)) return mu_refuse(msg, CMF_ERR_STATE, "%s: the %s is installed; %s", q.name, cur.noun, way_square);
        return CMF_OK;
    case MU_ASK_SQUARE_RULE:
        if (f.mask && !f.hals_mask && !std::strcmp(q.name, "HALS"))
            return mu_refuse(msg, CMF_ERR_STATE, "a mask of cmf_mu_set_mask is installed: the HALS rule has no masked form (its denominators become per-entry masked norms); clear it first");
        if (f.div != CMF_DIV_SQUARE)
            return mu_refuse(msg, CMF_ERR_STATE, "the %s is installed (%s): this rule minimises the squared error only; restore CMF_DIV_SQUARE first", cur.noun, cur.setter);
        return CMF_OK;
    case MU_ASK_SET_XORTHO:
        if (f.mask) return xortho_vs(xo_mask, way_unmask);
        if (f.div != CMF_DIV_SQUARE) return xortho_vs(xo_div, way_square);
        if (f.gram) return xortho_vs(xo_gram, way_gram);
        return CMF_OK;
    }
    return mu_refuse(msg, CMF_ERR_ARG, "internal: unknown request %d", q.what);
}
