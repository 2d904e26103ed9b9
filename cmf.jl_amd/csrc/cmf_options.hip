// cmf_options.hip -- cmf_set_option, cmf_option_names and cmf_get_counter: the effects of the rows of cmf_options.h (which decides, free
// of HIP, whether a request is taken and on what it is applied) and the table of the counters.  No kernel is launched from here, so the
// device pass of this unit is empty: it does not carry a copy of the kernels of cmf_kernels.h that are not templates.  NOTHING IN THIS
// FILE MAY LAUNCH A KERNEL: the host pass would compile the launch, and the kernel would be missing from the device object.
#ifndef __HIP_DEVICE_COMPILE__
#include "cmf_internal.h"

static int stream_sync(cmf_handle_s *h) { HIPCHK(hipSetDevice(h->device)); HIPCHK(hipStreamSynchronize(h->stream)); return CMF_OK; }

// ---- options: what setting one entails where it is more than storing a value -----------------------------------------------------
static int opt_custom(cmf_handle_s *h, const OptRow &r, int value)
{
    switch (r.custom) {
    case OPT_GRAM_FORM: // (a lone handle; a group: opt_custom_group)
        CMFTRY(mu_ask(h, MuAsk{MU_ASK_SET_GRAM, 0, 0.0, value}));
        if (value && h->mu_recentre)
            return fail(CMF_ERR_UNSUPPORTED, "the Gram forms (option \"gram\") keep tables of W across the H phase that the re-centring of cmf_mu_set_recentre would leave stale: "
                                             "switch it off first");
        h->gram = value;
        set_est(h, EST_NONE);
        return CMF_OK;
    case OPT_SMALL_K:
        CMFTRY(stream_sync(h));
        h->small_k = value != 0 && h->small_k_ok;
        h->sk_wj_gen = -1;
        h->sk_tc = h->small_k && (h->sk_tc_ok || value == 2); // (2: the few-component C3 form whatever T is -- tests, measurements)
        h->tc_S = h->sk_tc ? 2 * h->sk3_NS : h->tc_S_full; // (own block | the spill of the next block, per piece of the reduction: g_gemm_fold_small_kernel)
        h->tc_S1 = h->sk_tc ? 2 * h->sk3_NS : h->tc_S1_full;
        set_est(h, EST_NONE);
        return CMF_OK;
    case OPT_HALS_PREPARE:
        HIPCHK(hipSetDevice(h->device));
        return hals_ensure(h);
    case OPT_PROFILE:
        CMFTRY(stream_sync(h));
        for (auto &rec : h->prof_recs) { h->prof_pool.push_back(rec.a); h->prof_pool.push_back(rec.b); }
        h->prof_recs.clear();
        h->prof = value != 0;
        h->prof_every = value > 1 ? value : 1;
        for (int &c : h->prof_seen) c = 0;
        return CMF_OK;
    }
    return fail(CMF_ERR_ARG, "internal: option '%s' has no effect", r.name);
}

static int opt_custom_group(cmf_group_s *g, const OptRow &r, int value)
{
    CMFTRY(group_sync(g));
    switch (r.custom) {
    case OPT_OVERLAP:
        if (value) CMFTRY(group_ensure_lane1(g)); // the communication stream gets a communicator of its own
        g->overlap = value != 0;
        break;
    case OPT_HALO_IN_ALLREDUCE:
        g->halo_opt = value != 0;
        g->halos_current = g->halos_pending = g->halo_wide = false; // (the next phase starts from a whole exchange in the form that is now in force)
        break;
    case OPT_ENQUEUE_THREADS:
        if (value) return group_start_workers(g);
        (void)group_stop_workers(g); // (the group has just been synchronised: nobody is inside a job)
        return CMF_OK;
    case OPT_GRAM_FORM:
        // Gram form on a T-sharded group: every shard contracts numW and its additive share of HH = H_unfold H_unfold'
        // from its own columns, the all-reduce carries [numW | HH | tail] (numW + (L*Kpad)^2 floats instead of 2 numW),
        // denomW = HH * W is formed on every shard; denomH = lag-Gram taps of W applied to H with the H halos.
        for (size_t i = 0; i < g->sh.size(); ++i) {
            cmf_handle_s *s = g->sh[i];
            CMFTRY(group_use(s));
            if (value) CMFTRY(gram_ensure(s));
            // the HH block shares its place with denomW of the default form; hals_hh_kernel writes the first L*K columns
            // of each 128-padded row only, and the all-reduce sums the whole block in place: whatever the pad columns
            // held would be multiplied by the rank count every iteration until it overflowed
            if (value && i < g->red.size() && g->red[i])
                HIPCHK(hipMemsetAsync(g->red[i] + g->LKN2 / 2, 0, (size_t)g->HHsz * sizeof(float), s->stream));
            s->gram = value;
            set_est(s, EST_NONE);
            s->carry = CmfLossCarry{};
        }
        g->gram = value;
        break;
    }
    g->num_ready = false;
    return CMF_OK;
}

// the row applied to one handle: a lone one, or a shard of a group
static int opt_apply(cmf_handle_s *h, const OptRow &r, int stored, int value)
{
    if (r.custom != OPT_STORE) return opt_custom(h, r, value);
    if ((r.fx & FX_MU_GATE) && !value) CMFTRY(mu_ask(h, MuAsk{MU_ASK_GATE_OFF, 0, 0.0, 0, r.name}));
    if (r.fx & FX_SYNC) CMFTRY(stream_sync(h));
    h->*r.field = stored;
    if (r.fx & FX_DROP_EST) set_est(h, EST_NONE);
    if (r.fx & FX_DROP_SPEC) h->spec_gen = -1;
    if ((r.fx & FX_REPLAN) && h->hals_ready && !(r.fx & FX_SYNC)) CMFTRY(stream_sync(h));
    if ((r.fx & FX_REPLAN) && h->hals_ready) hals_plan(h);
    return CMF_OK;
}

int cmf_set_option(cmf_handle h, const char *name, int value)
{
    if (!h || !name) return fail(CMF_ERR_ARG, "NULL argument");
    cmf_group_s *g = h->group;
    OptKind k{g != nullptr, h->root_only, h->sharded, h->sharded && h->T_global != h->d.Tl};
    if (g) k.T = g->T, k.L = g->L, k.nranks = g->nranks;
    const OptDecision d = opt_decide(name, value, k, test_hooks_on());
    // (a group first collects what its enqueue workers left behind, whatever the answer -- but for a single-GPU option's refusal)
    if (g && !(d.row && d.row->scope == OPT_SINGLE)) CMFTRY(group_join(g));
    if (d.rc != CMF_OK) return fail(d.rc, "%s", d.msg.c_str());
    if (d.target == OPT_ON_HANDLE) return opt_apply(h, *d.row, d.stored, value);
    if (d.target == OPT_ON_GROUP) return opt_custom_group(g, *d.row, value);
    if (d.target == OPT_ON_SHARDS) {
        for (cmf_handle_s *s : g->sh) CMFTRY(opt_apply(s, *d.row, d.stored, value));
        g->num_ready = false;
    }
    return CMF_OK;
}

int cmf_option_names(char *buf, int64_t len)
{
    if (!buf || len < 1) return fail(CMF_ERR_ARG, "bad buffer");
    const std::string all = opt_names();
    if ((int64_t)all.size() + 1 > len) return fail(CMF_ERR_ARG, "buffer too small: %zu bytes needed", all.size() + 1);
    std::memcpy(buf, all.c_str(), all.size() + 1);
    return CMF_OK;
}

// ---- counters ------------------------------------------------------------------------------------------------------------------------
static const CounterRow<cmf_handle_s> kCounters[] = {
    CMF_COUNTER_ROW("hals_pipeline_reruns", h->hals_reruns, 0),
    CMF_COUNTER_ROW("plan:n_cu", (h->root_only && h->group && !h->group->sh.empty()) ? h->group->sh[0]->n_cu : h->n_cu, 0), // the CU count the plan was dealt for (a group: its shards')
    CMF_COUNTER_ROW("writeback_calls", h->wb ? h->wb->armed_calls : 0, 0),          // cmf_arm_writeback calls
    CMF_COUNTER_ROW("writeback_overlapped", h->wb ? h->wb->hooked_calls : 0, 0),    // ... served by the copy stream behind the H update
    CMF_COUNTER_ROW("speculated_contractions", h->spec_hits, 0),                    // update_motifs! calls whose C2 contraction was already enqueued
    CMF_COUNTER_ROW("liveness_checks", g_liveness_checks.load(), 0),                // (process-wide) stream queries made while waiting for a loss
    CMF_COUNTER_ROW("pow_update_launches", h->pow_launches, 0),                     // launches of w_update_pow_kernel / h_update_pow_kernel (the beta form outside 1 < beta <= 2)
    CMF_COUNTER_ROW("xortho_launches", h->xo_launches, 0),                          // launches of the kernels of cmf_xortho.h (0 while the weights of cmf_mu_set_xortho are 0 and no cost / terms entry was called)
    CMF_COUNTER_ROW("recentre_launches", h->recentre_launches, 0),                  // launches of the kernels of cmf_recentre.hip (four per step of cmf_mu_set_recentre / cmf_recentre)
    CMF_COUNTER_ROW("signif_launches", h->signif_launches, 0),                      // launches of the kernels of cmf_signif.h (cmf_null_moments: three per batch of draws)
    CMF_COUNTER_ROW("hals_masked_convs", h->hals_masked_convs, 0),                  // conv launches with the masked residual epilogue (modes 6 and 7) made by the HALS entries (option "hals_mask")
    CMF_COUNTER_ROW("small_k_fused_h_updates", h->sk_fused_h, CTR_SUM_SHARDS),      // H updates that ran inside the few-component C3 launch
    // host cost of the pipelined iterations of a group (reading a counter resets nothing)
    CMF_COUNTER_ROW("allreduce_calls", h->group->n_allreduce, CTR_GROUP_ONLY),      // collectives this handle has issued since it was made
    CMF_COUNTER_ROW("allgather_calls", h->group->n_allgather, CTR_GROUP_ONLY),      // (per shard: every rank makes each of them once)
    CMF_COUNTER_ROW("halo_in_allreduce", (h->group->halo_opt && h->group->halo_can && !h->group->gram && h->group->nranks > 1) ? 1 : 0, CTR_GROUP_ONLY),
    CMF_COUNTER_ROW("enqueue_ns", h->group->enqueue_ns, CTR_GROUP_ONLY),            // calling thread: enqueueing / posting
    CMF_COUNTER_ROW("enqueue_iters", h->group->enqueue_iters, CTR_GROUP_ONLY),      // ... over this many iterations
    // busiest enqueue worker: time inside its jobs
    {"worker_ns", [](const cmf_handle_s *h) { int64_t m = 0; for (const auto &w : h->group->pool.w) m = std::max<int64_t>(m, w->busy_ns.load()); return m; }, CTR_GROUP_ONLY},
};

// a per-shard count of the handle; a group: over its shards
template <class F> static int64_t over_shards(const cmf_handle_s *h, F get)
{
    int64_t v = get(h);
    if (h->group)
        for (const cmf_handle_s *s : h->group->sh) v += (s != h) ? get(s) : 0;
    return v;
}

int cmf_get_counter(cmf_handle h, const char *name, int64_t *value)
{
    if (!h || !name || !value) return fail(CMF_ERR_ARG, "NULL argument");
    if (std::strncmp(name, "launches:", 9) == 0) { // launches of one path (kLaunchNames; a group: over its shards)
        for (int c = 0; c < LA_NCLS; ++c)
            if (std::strcmp(name + 9, kLaunchNames[c]) == 0) { *value = over_shards(h, [c](const cmf_handle_s *s) { return s->launches[c]; }); return CMF_OK; }
        for (int c = 0; c < HL_NCLS; ++c) // the HALS entries' table (a HALS handle is never a group)
            if (std::strcmp(name + 9, kHalsLaunchNames[c]) == 0) { *value = h->hals_launches[c]; return CMF_OK; }
        return fail(CMF_ERR_ARG, "unknown launch path '%s'", name + 9);
    }
    const CounterRow<cmf_handle_s> *r = row_named(kCounters, name);
    if (r && (h->group || !(r->flags & CTR_GROUP_ONLY))) {
        *value = (r->flags & CTR_SUM_SHARDS) ? over_shards(h, r->get) : r->get(h);
        return CMF_OK;
    }
    // the fp64 rules answer for their own state: reverts of the last ADMM call of each kind, pivoting rounds of the last NNLS step of the
    // separable fit, pivoting rounds, backup-rule and capped problems of the last ANLS call
    if (admm_counter(h, name, value) || sep_counter(h, name, value) || anls_counter(h, name, value)) return CMF_OK;
    return fail(CMF_ERR_ARG, "unknown counter '%s'", name);
}
#endif // !__HIP_DEVICE_COMPILE__
