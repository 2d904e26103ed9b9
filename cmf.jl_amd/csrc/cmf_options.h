// cmf_options.h -- the string-keyed surface of the C ABI, stated once and free of HIP (like cmf_mu_install.h), so that a stand-alone
// program can walk it (tests/option_table_driver.cpp).  kOptions has one row per name of cmf_set_option: who may set it, which values it
// takes, the text of each refusal, and what setting it entails.  opt_decide answers a request from plain inputs -- the row, the code and
// text of a refusal, on what the row is to be applied -- before anything touches a handle; cmf_set_option (cmf_options.hip) applies the
// row.  cmf_option_names is the rows marked OPT_LISTED in their order.  A new option: a row (and a field of CmfOptionFields, or a case of
// opt_custom in cmf_options.hip where setting it is more than storing a value).  CounterRow is the row type of cmf_get_counter's and
// cmf_events_get_counter's tables.
#pragma once
#include "cmf_mu_install.h" // mu_refuse: a refusal's code and formatted text

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

// The options that are a stored value: base of cmf_handle_s, with their defaults.
struct CmfOptionFields {
    int reuse_est = 1, speculate = 1; // "reuse_est", "speculate"
    int gram = 0;          // "gram": 0 off, 1 Gram-form denominators, 2 also the loss from Gram sums
    int conv_variant = 0;  // "conv_kernel", K % 32 == 0: 3 = one-wave workgroups (conv3_kernel), 2 = 128 x 128 tiles (conv2_kernel), 0 = per mode
    int conv_split = 1;    // "conv_split": 0 = whole tiles only, 1 = quarter / sixteenth tiles for the thin last round of the one-wave conv kernel,
                           // 4 = quarter tiles only
    int sk_fuse = 1;       // "small_k_fuse": 1 = the element-wise update of H runs inside the C3 launch (cmf_small_k.h), 2 = also on one-round
                           // launches, where it is slower
    int hals_gram = 2;     // "hals_gram", the sweeps' projections as differences of the MU quantities: 2 = P of the H phase only (default: one conv
                           // launch fewer, H within the residual form's bars), 1 = G of the W phase too (~20x the rounding error in W: opt-in),
                           // 0 = both contracted from the stored residual
    // "hals_persist" (1 = the persistent pipeline where it fits, 0 = the stage pipeline, n > 1 = at most n pullers per row), "hals_general"
    // (bit 0 / 1: the general W / H sweeps at any shape), "hals_seg" / "hals_lag" (the stage pipeline's segment length and schedule),
    // "hals_debug" (CMF_TEST_HOOKS=1 only: 3 = the pullers leave at once, so that every bounded wait must run out)
    int hals_opt_persist = 1, hals_opt_general = 0, hals_opt_seg = 384, hals_opt_lag = 2, hals_debug = 0;
    int hals_opt_chase = -1;  // "hals_chase": per cent of the residual conv's tile rows that chase the row pipeline, 0 = off (-1: estimated from
                              // the shape, hals_chase_rows)
    int prof_mask = 0;        // "profile_mask": which kernel classes "profile" times (bit i: class i of kProfNames; 0 = all)
    int signif_batch = 0;     // "signif_batch": draws per batch of cmf_null_moments (0: the default of cmf_signif.h); the result does not depend on it
    int anls_backup_only = 0; // "anls_backup_only": every exchange of the ANLS solver is a backup-rule exchange (plain principal pivoting)
    int nnls_large = 0;       // "nnls_large": 129 .. 1024 unknowns run in nnls_large_kernel (cmf_nnls_large.h) instead of being refused
    // the gates of the MU forms: "kl_mask" = 1 lets the KL form, "pq_mask" = 1 the Itakura-Saito / beta forms and a mask of cmf_mu_set_mask be
    // installed together; "is_div" = 1 lets cmf_mu_set_divergence take CMF_DIV_IS
    int kl_mask = 0, pq_mask = 0, is_div = 0;
    int hals_mask = 0;        // "hals_mask": under a mask of cmf_mu_set_mask the HALS entries run on the data with its held-out entries imputed by the
                              // current estimate (the residual is the masked one; cmf_rules.hip) instead of being refused
};

enum OptScope {
    OPT_SINGLE, // single-GPU handles only: "<name>: <who> on single-GPU handles only" on a group, its front handle or a shard
    OPT_GROUP,  // a property of a group (opt_custom's group form); CMF_OK and nothing to do on a lone handle
    OPT_SHARDS, // a lone handle, or every shard of a group
    OPT_GRAM    // "gram": a lone form and a group form, each with its own accepted values
};
enum : unsigned {
    OPT_LISTED = 1,   // cmf_option_names lists it
    OPT_BOOL = 2,     // value != 0 is stored
    OPT_ELSE_0 = 4,   // a value outside lo .. hi is stored as 0 instead of being refused
    OPT_HOOKS = 8,    // a value other than 0 needs CMF_TEST_HOOKS=1
    FX_DROP_EST = 16, // what est holds is void afterwards (set_est(h, EST_NONE))
    FX_DROP_SPEC = 32, // a speculated contraction is void afterwards
    FX_SYNC = 64,     // the stream is synchronised before the value changes
    FX_REPLAN = 128,  // where the HALS scratch is ready: the stream is synchronised (unless FX_SYNC has) and the sweeps are planned again (hals_plan)
    FX_MU_GATE = 256  // a gate of the MU forms: cannot be switched off while what it let in is installed (mu_ask, MU_ASK_GATE_OFF)
};
enum OptCustom { OPT_STORE = 0, OPT_GRAM_FORM, OPT_SMALL_K, OPT_HALS_PREPARE, OPT_PROFILE, OPT_OVERLAP, OPT_ENQUEUE_THREADS, OPT_HALO_IN_ALLREDUCE };
constexpr int OPT_ANY = INT_MIN; // no lower bound / no hole (as hi: INT_MAX)

struct OptRow {
    const char *name;
    int scope;
    const char *who;             // OPT_SINGLE: the subject of its refusal
    int lo, hi, hole;            // accepted: lo <= value <= hi and value != hole
    const char *bad, *bad_hi;    // the refusal (one %s: the name) of a value below lo or at the hole / above hi (nullptr: `bad`)
    int CmfOptionFields::*field; // where the value is stored (nullptr: opt_custom sets what it sets)
    unsigned fx;
    int custom;                  // OptCustom: what setting it entails beyond `field` and `fx`
};
// the rows that take any value (listed, stored in `field` or set by opt_custom), the HALS rows (listed, >= 0), the unlisted 0/1 rows
#define OPT_ANY_VALUE(name, scope, field, fx, custom) {name, scope, nullptr, OPT_ANY, INT_MAX, OPT_ANY, nullptr, nullptr, field, OPT_LISTED | (fx), custom}
#define OPT_HALS(name, field, fx) {name, OPT_SHARDS, nullptr, 0, INT_MAX, OPT_ANY, "%s must be >= 0", nullptr, &CmfOptionFields::field, OPT_LISTED | (fx), OPT_STORE}
#define OPT_FLAG(name, who, fx) {#name, OPT_SINGLE, who, 0, 1, OPT_ANY, "%s must be 0 or 1", nullptr, &CmfOptionFields::name, fx, OPT_STORE}
static const OptRow kOptions[] = {
    OPT_ANY_VALUE("reuse_est", OPT_SHARDS, &CmfOptionFields::reuse_est, OPT_BOOL | FX_DROP_EST, OPT_STORE),
    // 1 (default): update_feature_maps! enqueues the next update_motifs!'s contraction behind its loss conv when the caller alternates the two calls
    OPT_ANY_VALUE("speculate", OPT_SHARDS, &CmfOptionFields::speculate, OPT_BOOL | FX_DROP_SPEC, OPT_STORE),
    {"gram", OPT_GRAM, nullptr, 0, 2, OPT_ANY, "gram must be 0, 1 or 2", nullptr, nullptr, OPT_LISTED, OPT_GRAM_FORM},
    {"conv_kernel", OPT_SHARDS, nullptr, 0, 3, 1, "conv_kernel must be 0 (per mode), 2 or 3", nullptr, &CmfOptionFields::conv_variant, OPT_LISTED | FX_DROP_EST, OPT_STORE},
    OPT_ANY_VALUE("conv_split", OPT_SHARDS, &CmfOptionFields::conv_split, FX_DROP_EST, OPT_STORE),
    // K <= 16: 1 = the few-component kernels (cmf_small_k.h; default), 0 = the general kernels, 2 = the few-component C3 form whatever T is
    OPT_ANY_VALUE("small_k", OPT_SHARDS, nullptr, 0, OPT_SMALL_K),
    {"small_k_fuse", OPT_SHARDS, nullptr, 0, 2, OPT_ANY, "small_k_fuse must be 0, 1 or 2", nullptr, &CmfOptionFields::sk_fuse, OPT_LISTED, OPT_STORE},
    // allocate the HALS scratch and check its shape limits now (rule construction)
    OPT_ANY_VALUE("hals_prepare", OPT_SHARDS, nullptr, 0, OPT_HALS_PREPARE),
    {"hals_gram", OPT_SHARDS, nullptr, 1, 2, OPT_ANY, nullptr, nullptr, &CmfOptionFields::hals_gram, OPT_LISTED | OPT_ELSE_0 | FX_DROP_EST, OPT_STORE},
    OPT_HALS("hals_persist", hals_opt_persist, FX_SYNC | FX_REPLAN),
    OPT_HALS("hals_general", hals_opt_general, FX_SYNC | FX_REPLAN),
    OPT_HALS("hals_seg", hals_opt_seg, FX_SYNC | FX_REPLAN),
    OPT_HALS("hals_lag", hals_opt_lag, FX_SYNC | FX_REPLAN),
    OPT_HALS("hals_debug", hals_debug, OPT_HOOKS), // results are wrong by design -- tests of the bounded waits only
    {"hals_chase", OPT_SHARDS, nullptr, -1, 100, OPT_ANY, "%s must be >= 0", "hals_chase is a percentage (0 = off)", &CmfOptionFields::hals_opt_chase, OPT_LISTED | FX_REPLAN, OPT_STORE},
    // (re)start or stop the in-loop kernel timing, every value-th launch of a class; collected times are dropped
    OPT_ANY_VALUE("profile", OPT_SHARDS, nullptr, 0, OPT_PROFILE),
    OPT_ANY_VALUE("profile_mask", OPT_SHARDS, &CmfOptionFields::prof_mask, 0, OPT_STORE),
    OPT_ANY_VALUE("allreduce_overlap", OPT_GROUP, nullptr, 0, OPT_OVERLAP),
    // 1: an enqueue worker per shard (cmf_workers.h), 0: the calling thread enqueues every shard
    OPT_ANY_VALUE("enqueue_threads", OPT_GROUP, nullptr, 0, OPT_ENQUEUE_THREADS),
    // 1 (default): the halo of H travels in the W-phase all-reduce where every shard can (cmf_groups.hip)
    OPT_ANY_VALUE("halo_in_allreduce", OPT_GROUP, nullptr, 0, OPT_HALO_IN_ALLREDUCE),
    // not listed (off by default, see the header; not paths of the listed rules)
    {"signif_batch", OPT_SINGLE, "cmf_null_moments runs", 0, INT_MAX, OPT_ANY, "signif_batch must be at least 0", nullptr, &CmfOptionFields::signif_batch, 0, OPT_STORE},
    OPT_FLAG(anls_backup_only, "the ANLS rule runs", 0),
    OPT_FLAG(nnls_large, "the ANLS rule and the separable fit run", 0), // cmf_anls_update_motifs / cmf_sep_nnls
    OPT_FLAG(kl_mask, "the mask and the divergence of the MU rule are chosen", FX_MU_GATE), // cmf_mu_set_mask + cmf_mu_set_divergence(KL) together
    OPT_FLAG(pq_mask, "the mask and the divergence of the MU rule are chosen", FX_MU_GATE), // cmf_mu_set_mask + the Itakura-Saito / beta form together
    OPT_FLAG(is_div, "the divergence of the MU rule is chosen", FX_MU_GATE),                // lets cmf_mu_set_divergence take CMF_DIV_IS
    OPT_FLAG(hals_mask, "the HALS rule runs", FX_DROP_EST | FX_DROP_SPEC),                  // cmf_mu_set_mask + cmf_hals_update_*: the imputed form (switchable at any time)
};
#undef OPT_ANY_VALUE
#undef OPT_FLAG
#undef OPT_HALS

// What kind of handle is asked, and what the group form of "gram" looks at.
struct OptKind {
    // fronts or belongs to a group; cmf_create_multi's front handle; made by cmf_create_shard / cmf_create_multi; a shard of cmf_create_shard
    // that holds a part of the columns and has no communicator yet
    bool group, root_only, sharded, partial;
    long long T = 0, L = 0; int nranks = 1;     // (a group: its global T and L, its rank count)
};
enum OptTarget { OPT_ON_NOTHING, OPT_ON_HANDLE, OPT_ON_GROUP, OPT_ON_SHARDS }; // refused or nothing to do; the handle; the group; each of its shards
// the row found, the code and text of a refusal, what the row is applied to, the value as the row's field takes it
struct OptDecision { const OptRow *row = nullptr; int rc = CMF_OK; std::string msg; int target = OPT_ON_NOTHING, stored = 0; };

// the row of a table (kOptions, a counter table) with this name
template <class Row, size_t N> static inline const Row *row_named(const Row (&rows)[N], const char *name)
{
    for (const Row &r : rows)
        if (std::strcmp(name, r.name) == 0) return &r;
    return nullptr;
}

// One lookup, one scope decision, one range check.  The order of the lines is the precedence among the refusals.
static inline OptDecision opt_decide(const char *name, int value, const OptKind &k, bool hooks)
{
    OptDecision d;
    auto refuse = [&](int code, const char *fmt, auto... args) { d.rc = mu_refuse(&d.msg, code, fmt, args...); d.target = OPT_ON_NOTHING; return d; };
    const OptRow *r = d.row = row_named(kOptions, name);
    if (!r) return refuse(CMF_ERR_ARG, "unknown option '%s'", name);
    if (r->scope == OPT_SINGLE && (k.group || k.root_only || k.sharded)) return refuse(CMF_ERR_UNSUPPORTED, "%s: %s on single-GPU handles only", name, r->who);
    if (r->scope == OPT_GROUP) {
        d.target = k.group ? OPT_ON_GROUP : OPT_ON_NOTHING; // (single GPU: nothing to overlap, nobody else to enqueue)
        return d;
    }
    d.target = !k.group ? OPT_ON_HANDLE : r->scope == OPT_GRAM ? OPT_ON_GROUP : OPT_ON_SHARDS;
    d.stored = (r->fx & OPT_BOOL) ? value != 0 : value;
    if (r->scope == OPT_GRAM && k.group) {
        if (value != 0 && value != 1) return refuse(CMF_ERR_UNSUPPORTED, "%s", "sharded handles take gram = 0 or 1 (the loss of gram = 2 is not exact to 1e-4)");
        if (value && k.nranks > 1 && k.T < 4 * k.L) return refuse(CMF_ERR_UNSUPPORTED, "the Gram form on a sharded handle needs T >= 4 L (got T=%lld, L=%lld)", k.T, k.L);
        return d;
    }
    const bool low = (r->lo != OPT_ANY && value < r->lo) || (r->hole != OPT_ANY && value == r->hole), high = value > r->hi;
    if ((low || high) && (r->fx & OPT_ELSE_0)) d.stored = 0;
    else if (low || high) return refuse(CMF_ERR_ARG, high && r->bad_hi ? r->bad_hi : r->bad, name);
    if ((r->fx & OPT_HOOKS) && value && !hooks) return refuse(CMF_ERR_STATE, "%s needs CMF_TEST_HOOKS=1", name);
    if (r->scope == OPT_GRAM && value && k.partial) return refuse(CMF_ERR_STATE, "%s", "the Gram form is not available on sharded handles");
    return d;
}

// cmf_option_names: the listed rows in their order, comma-separated
static inline std::string opt_names()
{
    std::string all;
    for (const OptRow &r : kOptions)
        if (r.fx & OPT_LISTED) all += (all.empty() ? "" : ",") + std::string(r.name);
    return all;
}

// A counter of a handle of type H: its name and how it is read.
enum : unsigned { CTR_SUM_SHARDS = 1, CTR_GROUP_ONLY = 2 }; // a group: summed over its shards; group handles only (unknown on a lone handle)
template <class H> struct CounterRow { const char *name; int64_t (*get)(const H *); unsigned flags; };
#define CMF_COUNTER_ROW(name, expr, flags) {name, [](const auto *h) -> int64_t { (void)h; return expr; }, flags} // (`expr` reads the handle as `h`)
