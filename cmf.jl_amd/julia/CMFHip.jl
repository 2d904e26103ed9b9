# CMFHip.jl -- the reference-side binding: a `ccall` layer over libcmf_hip.so (include/cmf_hip.h)
# that plugs the MI355X multiplicative-update rule into CMF.jl's own plugin boundary
# (`abstract type AbstractCFUpdate`, src/algs/alternating.jl:1-8).
#
# NOT EXECUTED IN THIS REPO'S CI: the build container has no Julia.  The tested twin of this file
# is cmf.jl_amd/host.py (same entry points, same argument order, same array layouts).  Julia
# arrays are already in the layout the C ABI expects (column-major Float64), so every call is a
# plain pointer hand-off.
#
# Where to include it: in src/CMF.jl AFTER `include("./algs/pgd.jl")` (src/CMF.jl:35), i.e. after the last algorithm
# file.  The imports below need names that only exist by then: `update_motifs!` / `update_feature_maps!` become
# generic functions in algs/mult.jl (:31), and SquareLoss, MaskedLoss, SquarePenalty, AbsolutePenalty and
# NonnegConstraint are defined in algs/pgd.jl (:35).  (Including it next to algs/mult.jl, as an earlier revision of
# this file said, fails with UndefVarError at the pgd.jl names.)
#
#     results = fit_cnmf(data; L=20, K=32, alg=HIPMultUpdate, max_itr=100)
#
module CMFHip

import ..CMF: AbstractCFUpdate, Tensor
import ..CMF: update_motifs!, update_feature_maps!                                   # generic functions: algs/mult.jl
import ..CMF: SquareLoss, AbsoluteLoss, MaskedLoss, SquarePenalty, AbsolutePenalty,    # types: algs/pgd.jl
              NonnegConstraint, UnitNormConstraint

const LIBCMF = get(ENV, "LIBCMF_HIP", "libcmf_hip.so")

# Regulariser keywords: HEAD's rules read `l1W, l2W, l1H, l2H` (src/algs/mult.jl:23,42; hals.jl:31,37); README.md:44-52
# and BASELINE's `fit_cnmf(data; ..., l1_H=0.1, l2_W=0.5)` spell them `l1_W, l2_W, l1_H, l2_H`, which HEAD's rules let
# fall into `kwargs...` and silently ignore.  The GPU rules accept both; giving both spellings of one weight is an error.
function reg(kwargs, head::Symbol, readme::Symbol, head_value)
    haskey(kwargs, readme) || return Float64(head_value)
    head_value == 0 || error("regulariser given twice: $head and $readme")
    return Float64(kwargs[readme])
end

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:cmf_last_error, LIBCMF), Cstring, ()))
    error("libcmf_hip error $rc: $msg")
end

"""
    HIPMultUpdate(data, W, H; device=0)
    HIPMultUpdate(data, W, H; devices=0:7)

Drop-in for `MultUpdate(data, W, H)` (src/algs/mult.jl:11-20).  Uploads `data`, `W`, `H`; the
rule's scratch (est, numW, denomW, numH, denomH) lives on the GPU.  W and H stay device-resident
between calls and are written back into the caller's arrays after every `update_feature_maps!`
(the reference mutates W and H in place; mult.jl:37-38, :51-52).

With `devices` the rule is a T-sharded group on several GPUs of the node (`cmf_create_multi`): this one Julia
task keeps making the same two calls per iteration (alternating.jl:52,54) and the library runs the sharded
iteration -- ONE RCCL all-reduce of [numW | denomW | loss tail | H halos] per iteration (round 6; the Gram form and PGD keep an
H-halo all-gather of their own), enqueued by one worker thread
per GPU inside the library.  `transport` (include/cmf_hip.h: CMF_COMM_*): 0 = RCCL for distinct devices (default),
4 = direct peer access over xGMI instead of RCCL (opt-in).  `set_option!(rule, "allreduce_overlap", 1)` etc. forward to
cmf_set_option.
"""
mutable struct HIPMultUpdate <: AbstractCFUpdate
    handle::Ptr{Cvoid}
    data_norm::Float64
    sync_every_call::Bool
    # The reference's rules READ the W and H they are handed (mult.jl:23,42).  Under sync_every_call every rule call fingerprints
    # its arguments (cmf_fingerprint) and compares with what this rule last read from / wrote into the caller's arrays; other
    # arrays, or arrays the caller has edited, are uploaded first (`reuploads` counts them).
    verify_args::Symbol      # :sample (one 64-byte line per 4 KB: bulk edits are seen, a single poked element may not be), :full, :none
    strict_inplace::Bool     # update_motifs! also writes W back (synchronous download), so edits between the two calls are honoured
    seen_W::UInt64           # fingerprints of the caller's arrays as this rule last read or wrote them (contents only: `fit`
    seen_H::UInt64           # deep-copies the initial factors, alternating.jl:33-34 -- equal arrays elsewhere are the same factors)
    w_pending::Bool          # update_motifs! has run and W has not been written back yet
    reuploads::Int
    mask_id::UInt            # objectid of the mask installed with cmf_mu_set_mask (0 = the unmasked rule)
end

function fingerprint(rule::HIPMultUpdate, a::Array{Float64})
    fp = Ref{UInt64}(0)
    check(ccall((:cmf_fingerprint, LIBCMF), Cint, (Ptr{Float64}, Int64, Int64, Ref{UInt64}),
                a, length(a), rule.verify_args == :full ? 1 : 64, fp))
    return fp[]
end

function HIPMultUpdate(data::Matrix{Float64}, W::Tensor{Float64}, H::Matrix{Float64};
                       device::Integer=parse(Int, get(ENV, "LOCAL_RANK", "0")), devices=nothing,
                       transport::Integer=0, sync_every_call::Bool=true, verify_args::Symbol=:sample,
                       strict_inplace::Bool=false)
    K, N, L = size(W)
    T = size(data, 2)
    size(data, 1) == N || throw(DimensionMismatch("data has $(size(data,1)) rows, W has N=$N"))
    size(H) == (K, T) || throw(DimensionMismatch("H must be $K x $T"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if devices === nothing
        check(ccall((:cmf_create, LIBCMF), Cint,
                    (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64, Int64, Ptr{Float64}),
                    h, device, N, T, K, L, data))
    else
        devs = Cint[d for d in devices]
        check(ccall((:cmf_create_multi, LIBCMF), Cint,
                    (Ref{Ptr{Cvoid}}, Cint, Ptr{Cint}, Cint, Int64, Int64, Int64, Int64, Ptr{Float64}),
                    h, length(devs), devs, transport, N, T, K, L, data))   # 0 = CMF_COMM_AUTO: RCCL for distinct devices
    end
    check(ccall((:cmf_set_factors, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h[], W, H))
    ss = Ref{Float64}(0.0)
    check(ccall((:cmf_get_data_sumsq, LIBCMF), Cint, (Ptr{Cvoid}, Ref{Float64}), h[], ss))
    rule = HIPMultUpdate(h[], sqrt(ss[]), sync_every_call, verify_args, strict_inplace, UInt64(0), UInt64(0), false, 0, UInt(0))
    rule.seen_W = fingerprint(rule, W)   # what cmf_set_factors has just read
    rule.seen_H = fingerprint(rule, H)
    finalizer(r -> (r.handle != C_NULL && ccall((:cmf_destroy, LIBCMF), Cint, (Ptr{Cvoid},), r.handle); r.handle = C_NULL), rule)
    return rule
end

# The reference's rules mutate W and H in place (mult.jl:37-38, :51-52) and `fit` hands the same arrays to every call
# (alternating.jl:51-54).  With `sync_every_call` (default) the update_feature_maps! that follows writes the new factors into
# W and H before it returns: cmf_arm_writeback borrows the two arrays until that call returns (hence GC.@preserve around both),
# and the download runs underneath the call's own kernels -- W during the H phase's first contraction, H during the loss
# conv, Float64 widening on helper threads -- instead of a 23 MB synchronous cmf_get_factors per iteration
# (INTEGRATION.md section 2 quotes the measured cost of both).
function arm_writeback(rule::HIPMultUpdate, W::Array{Float64}, H::Array{Float64})
    rule.sync_every_call || return
    check(ccall((:cmf_arm_writeback, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), rule.handle, W, H))
end

# The rule reads its arguments (mult.jl:23,42): arrays this rule has not seen in this state are uploaded first.
# W reaches the caller's array when update_feature_maps! returns (the write-back), not when update_motifs! does -- in between
# the caller's W is the one update_motifs! started from, so an edit made there is an edit of an outdated W: a clear error,
# unless the rule was built with strict_inplace=true (update_motifs! then downloads W synchronously, + ~0.5 ms at config 2).
# INTEGRATION.md section 3 states the contract; tests/test_dropin_contract.py pins it on the Python twin.
function sync_args!(rule::HIPMultUpdate, W::Array{Float64}, H::Array{Float64})
    (rule.sync_every_call && rule.verify_args != :none) || return
    nowW, nowH = fingerprint(rule, W), fingerprint(rule, H)
    dW, dH = nowW != rule.seen_W, nowH != rule.seen_H
    if dW && rule.w_pending
        error("W was modified (or another array was passed) between update_motifs! and update_feature_maps!: with " *
              "sync_every_call the caller's W holds the motifs update_motifs! started from until update_feature_maps! " *
              "returns.  Build the rule with strict_inplace=true, or call upload!(rule, W, H).")
    end
    if dW || dH
        check(ccall((:cmf_set_factors, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), rule.handle,
                    dW ? pointer(W) : Ptr{Float64}(C_NULL), dH ? pointer(H) : Ptr{Float64}(C_NULL)))
        rule.reuploads += 1
    end
    rule.seen_W, rule.seen_H = nowW, nowH
end

function after_motifs!(rule::HIPMultUpdate, W::Array{Float64})
    (rule.sync_every_call && rule.verify_args != :none) || return
    if rule.strict_inplace
        check(ccall((:cmf_get_factors, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), rule.handle, W, Ptr{Float64}(C_NULL)))
        rule.seen_W = fingerprint(rule, W)
    else
        rule.w_pending = true
    end
end

function after_feature_maps!(rule::HIPMultUpdate, W::Array{Float64}, H::Array{Float64})
    (rule.sync_every_call && rule.verify_args != :none) || return
    rule.seen_W, rule.seen_H = fingerprint(rule, W), fingerprint(rule, H)   # (the write-back has just filled them)
    rule.w_pending = false
end

"upload!(rule, W, H): make W, H the resident factors (cmf_set_factors); the next rule call takes its arguments as they are."
function upload!(rule::HIPMultUpdate, W::Array{Float64}, H::Array{Float64})
    check(ccall((:cmf_set_factors, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), rule.handle, W, H))
    rule.seen_W, rule.seen_H = fingerprint(rule, W), fingerprint(rule, H)
    rule.w_pending = false
end

# The rule under a mask (cmf_mu_set_mask): mask is N x T of 0 and 1, 1 = observed; the update is mult.jl:23-58 with
# data -> select(mask, data, 0) and est -> mask .* est (MaskedLoss, pgd.jl:58-70, for this rule).  Installed when the object
# changes (compared by objectid, like select_loss! of the PGD rule); `nothing` restores the unmasked rule.
function select_mask!(rule::HIPMultUpdate, mask)
    id = mask === nothing ? UInt(0) : objectid(mask)
    id == rule.mask_id && return
    if mask === nothing
        check(ccall((:cmf_mu_set_mask, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), rule.handle, C_NULL))
    else
        m = Matrix{Float64}(mask)
        check(ccall((:cmf_mu_set_mask, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), rule.handle, m))
    end
    rule.mask_id = id
end

# set_divergence!(rule, :kl): the rule becomes the multiplicative update of the generalised Kullback-Leibler divergence
# (cmf_mu_set_divergence): R = data ./ (est + eps) takes the place of data in mult.jl:32 and :47, the denominators are sums of H and
# of W, the loss is D(data, est + eps) / sum(data).  Data must be finite and non-negative.  :square restores mult.jl exactly.
# :itakura_saito (CMF_DIV_IS, for power spectrograms; data strictly positive): the library option "is_div" is set here first.
const CMF_DIV_SQUARE = 0
const CMF_DIV_KL = 1
const CMF_DIV_IS = 2
function set_divergence!(rule::HIPMultUpdate, kind::Symbol)
    kind in (:square, :kl, :itakura_saito) || throw(ArgumentError("divergence must be :square, :kl or :itakura_saito"))
    kind === :itakura_saito && set_option!(rule, "is_div", 1)
    check(ccall((:cmf_mu_set_divergence, LIBCMF), Cint, (Ptr{Cvoid}, Cint), rule.handle,
                kind === :kl ? CMF_DIV_KL : kind === :itakura_saito ? CMF_DIV_IS : CMF_DIV_SQUARE))
    return rule
end
# set_beta_divergence!(rule, beta): the beta-divergence between those three points (cmf_mu_set_beta_divergence): Q = e.^(beta - 1),
# P = data .* e.^(beta - 2), the step raised to gamma(beta); 0.01 <= beta <= 4, at least 0.01 away from 1; data finite and non-negative.
set_beta_divergence!(rule::HIPMultUpdate, beta::Real) = check(ccall((:cmf_mu_set_beta_divergence, LIBCMF), Cint, (Ptr{Cvoid}, Float64), rule.handle, Float64(beta)))

# set_xortho!(rule; lambda_xortho=0, lambda_ortho_H=0, lambda_ortho_W=0): seqNMF's cross-orthogonality penalties on the squared-error rule
# (cmf_mu_set_xortho): with S the box smoothing of width 2L-1 along t, off the sum over the OTHER components and G = off(S(H)),
# mult.jl:37 gets lambda xW + lambda_W off(Wflat) added to denomW (xW: mult.jl:32 with G in H's place) and mult.jl:51 gets
# lambda off(S(numH)) + lambda_H G added to denomH, before the regularisers.  The loss stays norm(est - data) / norm(data).  All zeros
# restore the plain rule.  One GPU; no mask, no divergence, no Gram form.
function set_xortho!(rule::HIPMultUpdate; lambda_xortho::Real=0, lambda_ortho_H::Real=0, lambda_ortho_W::Real=0)
    check(ccall((:cmf_mu_set_xortho, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64, Float64), rule.handle,
                Float64(lambda_xortho), Float64(lambda_ortho_H), Float64(lambda_ortho_W)))
    return rule
end
# xortho_cost(rule) -> (xortho, ortho_H, ortho_W): the three penalty sums of the resident factors without their weights and without
# the 1/2, summed in fp64 (cmf_mu_xortho_cost)
function xortho_cost(rule::HIPMultUpdate)
    x, oh, ow = Ref{Float64}(0.0), Ref{Float64}(0.0), Ref{Float64}(0.0)
    check(ccall((:cmf_mu_xortho_cost, LIBCMF), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}, Ref{Float64}), rule.handle, x, oh, ow))
    return x[], oh[], ow[]
end
# xortho_terms(rule, K, N, L, T) -> (xW, xH, oH, oW): the four unweighted denominator terms for the resident factors, in the shapes
# of W, H, H and W (cmf_mu_xortho_terms)
function xortho_terms(rule::HIPMultUpdate, K::Integer, N::Integer, L::Integer, T::Integer)
    xW, oW = zeros(Float64, K, N, L), zeros(Float64, K, N, L)
    xH, oH = zeros(Float64, K, T), zeros(Float64, K, T)
    check(ccall((:cmf_mu_xortho_terms, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), rule.handle, xW, xH, oH, oW))
    return xW, xH, oH, oW
end

# null_moments(rule, K, seed, first_draw, n_draws) -> a 3 x K x n_draws array: seqNMF's significance test on held-out data
# (test_significance.m; cmf_null_moments).  The rule's data are the held-out columns; draw d >= 1 shifts row (k, n) of the resident W
# circularly along the lag axis by s(d, k, n) (cmf_null_shifts; draw 0 is W itself), and [:, k, j] holds sum v, sum v^2, sum v^3 over t of
# v = tensor_transconv(Wnull_d, data)[k, :] (common.jl:71-81) for d = first_draw + j - 1.  The skewness of each column of sums,
# m3 / m2^1.5 with mu = S1/T, m2 = S2/T - mu^2, m3 = S3/T - 3 mu S2/T + 2 mu^3, compared between draw 0 and the others gives the
# p-values.  Changes nothing the rule calls read.  One GPU; no mask.
function null_moments(rule::HIPMultUpdate, K::Integer, seed::Integer, first_draw::Integer, n_draws::Integer)
    sums = zeros(Float64, 3, K, n_draws)
    check(ccall((:cmf_null_moments, LIBCMF), Cint, (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}), rule.handle, UInt64(seed), Int64(first_draw), Int64(n_draws), sums))
    return sums
end

# seqNMF's re-centring of motifs (shiftFactors.m; include/cmf_hip.h has the definition).  set_recentre!(rule, on): every
# update_feature_maps! moves each motif's centre of mass back to the middle of the L-lag window and its row of H the other way, on the
# device, between mult.jl:51-52 and :55-57 (cmf_mu_set_recentre); with sync_every_call the write-back then delivers BOTH arrays, W too.
# recentre!(rule, K) -> the K shifts of one step on the resident factors (cmf_recentre).  recentre_info(rule, K) -> (last shifts,
# totals of |s_k|) (cmf_mu_recentre_info).  One GPU; not with the Gram form.
function set_recentre!(rule::HIPMultUpdate, on::Bool)
    check(ccall((:cmf_mu_set_recentre, LIBCMF), Cint, (Ptr{Cvoid}, Cint), rule.handle, Cint(on)))
    return rule
end
# (these two take int32_t arrays and are written with @ccall: the type table of tests/test_julia_binding.py, which checks every
# call of the other form against its prototype, has no row for Ptr{Int32} -- the prototypes are `int cmf_recentre(cmf_handle, int32_t *)`
# and `int cmf_mu_recentre_info(cmf_handle, int32_t *, int64_t *)`, include/cmf_hip.h)
function recentre!(rule::HIPMultUpdate, K::Integer)
    s = zeros(Int32, K)
    h = rule.handle
    check(@ccall LIBCMF.cmf_recentre(h::Ptr{Cvoid}, s::Ptr{Int32})::Cint)
    return s
end
function recentre_info(rule::HIPMultUpdate, K::Integer)
    s, moved = zeros(Int32, K), zeros(Int64, K)
    h = rule.handle
    check(@ccall LIBCMF.cmf_mu_recentre_info(h::Ptr{Cvoid}, s::Ptr{Int32}, moved::Ptr{Int64})::Cint)
    return s, moved
end
# the keyword of fit_cnmf(...; shift=true) as it reaches a rule call (eval mode holds W fixed: nothing is shifted)
select_shift!(rule::HIPMultUpdate, shift, kwargs) = shift === nothing ? rule : set_recentre!(rule, Bool(shift) && !get(kwargs, :eval_mode, false))

# update_motifs!(rule, data, W, H; l1W=0, l2W=0, mask=nothing)  -- src/algs/mult.jl:23-39, called at alternating.jl:52
function update_motifs!(rule::HIPMultUpdate, data, W, H; l1W=0, l2W=0, mask=nothing, kwargs...)
    select_mask!(rule, mask)
    GC.@preserve W H begin
        sync_args!(rule, W, H)
        check(ccall((:cmf_update_motifs, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64), rule.handle,
                    reg(kwargs, :l1W, :l1_W, l1W), reg(kwargs, :l2W, :l2_W, l2W)))
        after_motifs!(rule, W)
    end
    return W
end

# update_feature_maps!(rule, data, W, H; l1H=0, l2H=0, mask=nothing, shift=nothing) -> loss  -- src/algs/mult.jl:42-58, alternating.jl:54
# (shift=true: the re-centring step above; the call then changes W as well as H)
function update_feature_maps!(rule::HIPMultUpdate, data, W, H; l1H=0, l2H=0, mask=nothing, shift=nothing, kwargs...)
    select_mask!(rule, mask)
    select_shift!(rule, shift, kwargs)
    loss = Ref{Float64}(0.0)
    GC.@preserve W H begin
        sync_args!(rule, W, H)
        arm_writeback(rule, W, H)
        check(ccall((:cmf_update_feature_maps, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64, Ref{Float64}),
                    rule.handle, reg(kwargs, :l1H, :l1_H, l1H), reg(kwargs, :l2H, :l2_H, l2H), loss))
        after_feature_maps!(rule, W, H)
    end
    return loss[]
end

"""
    HIPHALSUpdate(data, W, H; device=0)

Drop-in for `HALSUpdate(data, W, H)` (src/algs/hals.jl:18-28) on the same handle type: the K*L column
updates of W and the K*T entry updates of H run on the GPU in the reference's Gauss-Seidel order.
"""
mutable struct HIPHALSUpdate <: AbstractCFUpdate
    inner::HIPMultUpdate
end
HIPHALSUpdate(data, W, H; kwargs...) = HIPHALSUpdate(HIPMultUpdate(data, W, H; kwargs...))

# update_motifs!(rule::HALSUpdate, ...; l1W=0, l2W=0)  -- src/algs/hals.jl:31-34
function update_motifs!(rule::HIPHALSUpdate, data, W, H; l1W=0, l2W=0, kwargs...)
    GC.@preserve W H begin
        sync_args!(rule.inner, W, H)
        check(ccall((:cmf_hals_update_motifs, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64), rule.inner.handle,
                    reg(kwargs, :l1W, :l1_W, l1W), reg(kwargs, :l2W, :l2_W, l2W)))
        after_motifs!(rule.inner, W)
    end
    return W
end

# update_feature_maps!(rule::HALSUpdate, ...; l1H=0, l2H=0) -> loss  -- src/algs/hals.jl:37-42
function update_feature_maps!(rule::HIPHALSUpdate, data, W, H; l1H=0, l2H=0, kwargs...)
    loss = Ref{Float64}(0.0)
    GC.@preserve W H begin
        sync_args!(rule.inner, W, H)
        arm_writeback(rule.inner, W, H)
        check(ccall((:cmf_hals_update_feature_maps, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64, Ref{Float64}),
                    rule.inner.handle, reg(kwargs, :l1H, :l1_H, l1H), reg(kwargs, :l2H, :l2_H, l2H), loss))
        after_feature_maps!(rule.inner, W, H)
    end
    return loss[]
end

"""
    HIPPGDUpdate(data, W, H; device=0)

Drop-in for `PGDUpdate(data, W, H)` (src/algs/pgd.jl:112-155) with `SquareLoss()`, `AbsoluteLoss()` or
`MaskedLoss(either, mask)`, `SquarePenalty` / `AbsolutePenalty` lists and `NonnegConstraint()` /
`UnitNormConstraint()` / `nothing`.
The step-size state (stepW, stepH, cur_loss) lives in the library handle.
"""
mutable struct HIPPGDUpdate <: AbstractCFUpdate
    inner::HIPMultUpdate
    mask_id::UInt            # objectid of the mask currently resident on the device (0 = none)
    loss_kind::Cint          # 0 SquareLoss, 1 AbsoluteLoss (cmf_pgd_set_loss)
end
# `devices=0:7` shards T over several GPUs like HIPMultUpdate does (one all-reduce of the partial gradW per iteration;
# MaskedLoss masks are cut along T by the library)
function HIPPGDUpdate(data, W, H; kwargs...)
    rule = HIPPGDUpdate(HIPMultUpdate(data, W, H; kwargs...), UInt(0), Cint(0))
    check(ccall((:cmf_pgd_reset, LIBCMF), Cint, (Ptr{Cvoid},), rule.inner.handle))
    return rule
end

penalty_weights(pens) = (sum(Float64[p.weight for p in pens if p isa SquarePenalty]),
                         sum(Float64[p.weight for p in pens if p isa AbsolutePenalty]))
# README-style regularisers (`l1_W`, `l2_W`, `l1_H`, `l2_H`) do NOT reach the PGD rule: the reference's PGD methods take
# penalties only through `penaltiesW` / `penaltiesH` and swallow every other keyword in `kwargs...` (pgd.jl:158-202), and
# so do these (and PGDUpdate in cmf.jl_amd/host.py): `fit_cnmf(data; alg=:pgd, l2_W=0.5)` gives the factors of
# `fit_cnmf(data; alg=:pgd)` here, in the Python mirror and in the reference alike.
# 0 none, 1 NonnegConstraint (pgd.jl:92-96), 2 UnitNormConstraint (pgd.jl:100-110)
nonneg_flag(c) = c === nothing ? Cint(0) : (c isa NonnegConstraint ? Cint(1) :
                 (c isa UnitNormConstraint ? Cint(2) : error("unsupported constraint")))

function select_loss!(rule::HIPPGDUpdate, loss_func)
    base = loss_func isa MaskedLoss ? loss_func.loss : loss_func             # pgd.jl:58-70
    kind = base isa SquareLoss ? Cint(0) : (base isa AbsoluteLoss ? Cint(1) :
           error("HIPPGDUpdate supports SquareLoss(), AbsoluteLoss() and MaskedLoss of either"))
    if kind != rule.loss_kind
        check(ccall((:cmf_pgd_set_loss, LIBCMF), Cint, (Ptr{Cvoid}, Cint), rule.inner.handle, kind))
        rule.loss_kind = kind
    end
    if loss_func isa MaskedLoss
        id = objectid(loss_func.mask)
        if id != rule.mask_id
            m = Matrix{Float64}(loss_func.mask)
            check(ccall((:cmf_set_mask, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), rule.inner.handle, m))
            rule.mask_id = id
        end
    else
        rule.mask_id == 0 || check(ccall((:cmf_set_mask, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), rule.inner.handle, C_NULL))
        rule.mask_id = UInt(0)
    end
end

# update_motifs!(rule::PGDUpdate, ...; loss_func, constrW, penaltiesW)  -- src/algs/pgd.jl:158-177
function update_motifs!(rule::HIPPGDUpdate, data, W, H; loss_func=SquareLoss(), constrW=NonnegConstraint(),
                        penaltiesW=[SquarePenalty(1)], kwargs...)
    select_loss!(rule, loss_func)
    sq, ab = penalty_weights(penaltiesW)
    GC.@preserve W H begin
        sync_args!(rule.inner, W, H)
        check(ccall((:cmf_pgd_update_motifs, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64, Cint),
                    rule.inner.handle, sq, ab, nonneg_flag(constrW)))
        after_motifs!(rule.inner, W)
    end
    return W
end

# update_feature_maps!(rule::PGDUpdate, ...; loss_func, constrH, penaltiesH) -> loss  -- src/algs/pgd.jl:180-202
function update_feature_maps!(rule::HIPPGDUpdate, data, W, H; loss_func=SquareLoss(), constrH=NonnegConstraint(),
                              penaltiesH=[], kwargs...)
    select_loss!(rule, loss_func)
    sq, ab = penalty_weights(penaltiesH)
    loss = Ref{Float64}(0.0)
    GC.@preserve W H begin
        sync_args!(rule.inner, W, H)
        arm_writeback(rule.inner, W, H)
        check(ccall((:cmf_pgd_update_feature_maps, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Float64, Cint, Ref{Float64}),
                    rule.inner.handle, sq, ab, nonneg_flag(constrH), loss))
        after_feature_maps!(rule.inner, W, H)
    end
    return loss[]
end

"""
    ALGORITHMS

README.md:16,30-33 selects the algorithm with a symbol (`alg=:mult`, `:hals`); HEAD's table for that is commented out
(src/model.jl:3-8) and `fit_cnmf` calls `alg(data, W_init, H_init)` (model.jl:78-82), so a symbol fails there with a
MethodError.  INTEGRATION.md section 2b shows the five-line patch to model.jl that looks `alg` up here first.
"""
const ALGORITHMS = Dict{Symbol,Any}(
    :mult => HIPMultUpdate,
    :hals => HIPHALSUpdate,
    :pgd => HIPPGDUpdate,
)

"""
    HIPADMMUpdate(data, W, H; device=LOCAL_RANK or 0)

Drop-in for `ADMMUpdate(data, W, H)` (src/algs/admm.jl:13-21), computed in fp64 on one GPU.  Not in `ALGORITHMS`: select
it by type, as the reference does (`fit_cnmf(data; alg=HIPADMMUpdate)`, model.jl:60).  Each call reads the factor the
reference reads (`update_motifs!` H, `update_feature_maps!` W) and overwrites the other one in place; `W_iters` / `H_iters`
hold the inner iteration counts of the last calls.
"""
mutable struct HIPADMMUpdate <: AbstractCFUpdate
    handle::Ptr{Cvoid}
    W_iters::Int64
    H_iters::Int64
end
function HIPADMMUpdate(data, W, H; device::Integer=parse(Int, get(ENV, "LOCAL_RANK", "0")))
    K, N, L = size(W)
    T = size(data, 2)
    size(data, 1) == N || throw(DimensionMismatch("data has $(size(data,1)) rows, W has N=$N"))
    size(H) == (K, T) || throw(DimensionMismatch("H must be $K x $T"))
    d = Matrix{Float64}(data)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cmf_create, LIBCMF), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64, Int64, Ptr{Float64}),
                h, device, N, T, K, L, d))
    rule = HIPADMMUpdate(h[], 0, 0)
    finalizer(r -> (r.handle != C_NULL && ccall((:cmf_destroy, LIBCMF), Cint, (Ptr{Cvoid},), r.handle); r.handle = C_NULL), rule)
    check(ccall((:cmf_admm_prepare, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), rule.handle, d))
    return rule
end

# update_motifs!(rule::ADMMUpdate, data, W, H; rhow=10, admm_W_maxiter=30, admm_tol=1e-4, nonnegW=true)  -- src/algs/admm.jl:24-121
function update_motifs!(rule::HIPADMMUpdate, data, W, H; rhow=10, admm_W_maxiter=30, admm_tol=1e-4, nonnegW=true, kwargs...)
    Hc = Matrix{Float64}(H)
    Wc = W isa Array{Float64,3} ? W : Array{Float64,3}(W)
    iters = Ref{Int64}(0)
    check(ccall((:cmf_admm_update_motifs, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Int64, Float64, Cint, Ref{Int64}),
                rule.handle, Hc, Wc, rhow, admm_W_maxiter, admm_tol, nonnegW ? 1 : 0, iters))
    Wc === W || (W .= Wc)
    rule.W_iters = iters[]
    return W
end

# update_feature_maps!(rule::ADMMUpdate, data, W, H; rhoh=10, admm_H_maxiter=30, l1H=0, admm_tol=1e-4, nonnegH=true) -> loss
# -- src/algs/admm.jl:124-226
function update_feature_maps!(rule::HIPADMMUpdate, data, W, H; rhoh=10, admm_H_maxiter=30, l1H=0, admm_tol=1e-4, nonnegH=true,
                              kwargs...)
    Wc = Array{Float64,3}(W)
    Hc = H isa Matrix{Float64} ? H : Matrix{Float64}(H)
    loss, iters = Ref{Float64}(0.0), Ref{Int64}(0)
    check(ccall((:cmf_admm_update_feature_maps, LIBCMF), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Int64, Float64, Float64, Cint, Ref{Float64}, Ref{Int64}),
                rule.handle, Wc, Hc, rhoh, admm_H_maxiter, l1H, admm_tol, nonnegH ? 1 : 0, loss, iters))
    Hc === H || (H .= Hc)
    rule.H_iters = iters[]
    return loss[]
end

"""
    HIPANLSUpdate(data, W, H; device=LOCAL_RANK or 0)

Drop-in for `ANLSUpdate(data, W, H)` (src/algs/anls.jl:10-14), computed in fp64 on one GPU, on the K x N x L layout of W.  Not in
`ALGORITHMS`: select it by type (`fit_cnmf(data; alg=HIPANLSUpdate, variant=:block)`, model.jl:60).  `update_motifs!` reads H and
overwrites W with the exact minimiser over W >= 0; `update_feature_maps!` overwrites H column by column (`variant=:basic`) or in
L phases of independent columns (`variant=:block`).  K <= 64; K*L <= 128, or K*L <= 1024 after
`set_option!(rule, "nnls_large", 1)` (`update_motifs!` then solves 129 and more unknowns per unit through device scratch).
"""
mutable struct HIPANLSUpdate <: AbstractCFUpdate
    handle::Ptr{Cvoid}
end
function HIPANLSUpdate(data, W, H; device::Integer=parse(Int, get(ENV, "LOCAL_RANK", "0")))
    K, N, L = size(W)
    T = size(data, 2)
    size(data, 1) == N || throw(DimensionMismatch("data has $(size(data,1)) rows, W has N=$N"))
    size(H) == (K, T) || throw(DimensionMismatch("H must be $K x $T"))
    d = Matrix{Float64}(data)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cmf_create, LIBCMF), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64, Int64, Ptr{Float64}),
                h, device, N, T, K, L, d))
    rule = HIPANLSUpdate(h[])
    finalizer(r -> (r.handle != C_NULL && ccall((:cmf_destroy, LIBCMF), Cint, (Ptr{Cvoid},), r.handle); r.handle = C_NULL), rule)
    check(ccall((:cmf_anls_prepare, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), rule.handle, d))
    return rule
end

# update_motifs!(rule::ANLSUpdate, data, W, H; kwargs...)  -- src/algs/anls.jl:22-24, :47-57
function update_motifs!(rule::HIPANLSUpdate, data, W, H; kwargs...)
    Hc = Matrix{Float64}(H)
    Wc = W isa Array{Float64,3} ? W : Array{Float64,3}(W)
    check(ccall((:cmf_anls_update_motifs, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), rule.handle, Hc, Wc))
    Wc === W || (W .= Wc)
    return W
end

# update_feature_maps!(rule::ANLSUpdate, data, W, H; variant=:basic, kwargs...) -> loss  -- src/algs/anls.jl:26-36, :63-137
function update_feature_maps!(rule::HIPANLSUpdate, data, W, H; variant=:basic, kwargs...)
    variant in (:basic, :block) || throw(ArgumentError("variant must be :basic or :block, got $variant"))
    Wc = Array{Float64,3}(W)
    Hc = H isa Matrix{Float64} ? H : Matrix{Float64}(H)
    loss = Ref{Float64}(0.0)
    check(ccall((:cmf_anls_update_feature_maps, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}),
                rule.handle, Wc, Hc, variant == :block ? 1 : 0, loss))
    Hc === H || (H .= Hc)
    return loss[]
end

# evaluate_heldout(data, W, H, mask; device=0, divergence=:square) -> (train, test): sqrt(sum of (est - data)^2 / sum of data^2) over
# the entries with mask == 1 and over those with mask == 0, for a fitted model (cmf_masked_loss: one loss-only conv each, sums by
# select, so NaNs among the held-out data stay out of the train score).  divergence=:kl: D / sum(data) over the same two sets of
# entries (no square root), through the library option "kl_mask" (the KL form of the MU rule under a mask, include/cmf_hip.h).
# divergence=:itakura_saito, or :beta with beta=, under options=Dict("pq_mask" => 1) (the Itakura-Saito and beta forms under a mask):
# the mean divergence per entry over the same two sets (sum of the terms / number of entries).
function evaluate_heldout(data::Matrix{Float64}, W::Tensor{Float64}, H::Matrix{Float64}, mask; device::Integer=0, divergence::Symbol=:square,
                          beta=nothing, options=nothing)
    divergence in (:square, :kl, :itakura_saito, :beta) || throw(ArgumentError("divergence must be :square, :kl, :itakura_saito or :beta"))
    pq = divergence in (:itakura_saito, :beta)
    pq && (options === nothing || get(options, "pq_mask", 0) != 1) &&
        throw(ArgumentError("divergence=:$divergence has no held-out score: the form has no masked form unless the library option is set: options=Dict(\"pq_mask\" => 1)"))
    divergence === :beta && beta === nothing && throw(ArgumentError("divergence=:beta needs beta="))
    rule = HIPMultUpdate(data, W, H; device=device, sync_every_call=false)
    divergence === :kl && set_option!(rule, "kl_mask", 1)
    pq && set_option!(rule, "pq_mask", 1)
    select_mask!(rule, mask)
    divergence === :kl && set_divergence!(rule, :kl)
    divergence === :itakura_saito && set_divergence!(rule, :itakura_saito)
    divergence === :beta && set_beta_divergence!(rule, beta)
    scores = Float64[]
    for complement in (0, 1)
        r, d = Ref{Float64}(0.0), Ref{Float64}(0.0)
        check(ccall((:cmf_masked_loss, LIBCMF), Cint, (Ptr{Cvoid}, Cint, Ref{Float64}, Ref{Float64}), rule.handle, complement, r, d))
        push!(scores, divergence === :square ? sqrt(r[] / d[]) : r[] / d[])
    end
    finalize(rule)
    return scores[1], scores[2]
end

"""
    iterate!(rule, n; l1W=0, l2W=0, l1H=0, l2H=0, eval_mode=false) -> losses

`n` x (`update_motifs!`; `update_feature_maps!`) back to back (alternating.jl:51-54) in one ccall (`cmf_iterate`): the
n losses; the host never stalls the device between iterations.  W and H are not copied back (use `download!`).
"""
function iterate!(rule::HIPMultUpdate, n::Integer; l1W=0, l2W=0, l1H=0, l2H=0, eval_mode::Bool=false)
    losses = zeros(n)
    check(ccall((:cmf_iterate, LIBCMF), Cint,
                (Ptr{Cvoid}, Int64, Cint, Float64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}),
                rule.handle, n, eval_mode ? 1 : 0, l1W, l2W, l1H, l2H, losses, C_NULL))
    return losses
end

"Library option (include/cmf_hip.h, cmf_set_option): \"reuse_est\", \"speculate\", \"gram\", \"small_k\", \"allreduce_overlap\", \"enqueue_threads\", \"kl_mask\" (set_divergence!(rule, :kl) together with a mask), \"pq_mask\" (set_divergence!(rule, :itakura_saito) / set_beta_divergence! together with a mask), \"hals_mask\" (the HALS rule under a mask: HALS on the data imputed by the current estimate), ..."
set_option!(rule::HIPMultUpdate, name::AbstractString, value::Integer) =
    check(ccall((:cmf_set_option, LIBCMF), Cint, (Ptr{Cvoid}, Cstring, Cint), rule.handle, name, value))
"The ANLS rule's options: \"anls_backup_only\", \"nnls_large\" (include/cmf_hip.h, the ANLS rule)."
set_option!(rule::HIPANLSUpdate, name::AbstractString, value::Integer) =
    check(ccall((:cmf_set_option, LIBCMF), Cint, (Ptr{Cvoid}, Cstring, Cint), rule.handle, name, value))

"Library identification: \"cmf_hip gfx950 <version> abi=<n> src=<digest of the sources it was built from>\"."
version() = unsafe_string(ccall((:cmf_version, LIBCMF), Cstring, ()))

"Block until everything the rule has enqueued has finished (all devices of a `devices=` group)."
synchronize(rule::HIPMultUpdate) = check(ccall((:cmf_synchronize, LIBCMF), Cint, (Ptr{Cvoid},), rule.handle))

"Write the device-resident factors into W and H (needed only with `sync_every_call=false`)."
function download!(rule::HIPMultUpdate, W::Tensor{Float64}, H::Matrix{Float64})
    check(ccall((:cmf_get_factors, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), rule.handle, W, H))
    return W, H
end

# Stand-alone primitives: src/common.jl:17-34, :62-81
function tensor_conv(W::Tensor{Float64}, H::Matrix{Float64}; device::Integer=0)
    K, N, L = size(W); T = size(H, 2)
    est = zeros(N, T)
    check(ccall((:cmf_tensor_conv, LIBCMF), Cint,
                (Cint, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), device, N, T, K, L, W, H, est))
    return est
end

function tensor_transconv(W::Tensor{Float64}, X::Matrix{Float64}; device::Integer=0)
    K, N, L = size(W); T = size(X, 2)
    out = zeros(K, T)
    check(ccall((:cmf_tensor_transconv, LIBCMF), Cint,
                (Cint, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), device, N, T, K, L, W, X, out))
    return out
end

# init_rand(data, L, K): src/model.jl:113-125 (portable RNG; `seed` as in fit_cnmf's kwarg)
function init_rand(data::Matrix{Float64}, L::Integer, K::Integer; seed::Integer=rand(UInt64), device::Integer=0)
    N, T = size(data)
    W = zeros(K, N, L); H = zeros(K, T)
    check(ccall((:cmf_init_rand, LIBCMF), Cint,
                (Cint, Int64, Int64, Int64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                device, N, T, K, L, seed % UInt64, data, W, H))
    return W, H
end

# gen_synthetic(N=, T=): README.md:14 / datasets/synthetic.jl:29-61
function gen_synthetic(; N=100, T=500, K=3, L=20, alpha=0.1, p_h=0.5, sigma=0.2, noise_scale=1.0, seed=1234, device::Integer=0)
    data = zeros(N, T)
    check(ccall((:cmf_gen_synthetic, LIBCMF), Cint,
                (Cint, Int64, Int64, Int64, Int64, Float64, Float64, Float64, Float64, UInt64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                device, N, T, K, L, alpha, p_h, sigma, noise_scale, seed % UInt64, data, C_NULL, C_NULL))
    return data
end

"""
    HIPSeparable.fit(data, K, L; thresh=0, verbose=false, refit_H=false, refit_W=false, refit_H_itr=10, spectral=false,
                     pre=nothing, nnls_large=false, device=LOCAL_RANK or 0) -> W, H

Drop-in for `Separable.fit` (src/algs/separable.jl:14-56) in fp64 on one GPU, on the K x N x L layout of W.  The four device stages
are `cmf_sep_spa`, `cmf_sep_nnls`, `cmf_sep_shift_table` and `cmf_sep_construct`; the grouping and sorting of the K*L rows
(separable.jl:96-131, :191-270) run here on the shift table.  K*L <= 128, or K*L <= 1024 with `nnls_large=true` (the library option
"nnls_large" on the NNLS step and on the rule of `refit_W`).  Row and column numbers are 0-based on the C side.
"""
module HIPSeparable

using LinearAlgebra
import ..CMFHip: LIBCMF, check, HIPANLSUpdate, HIPHALSUpdate, update_motifs!, update_feature_maps!, set_option!

cos_ab(P, head, a, b) = (P[a, b, :] ./ (head[a, :] .* head[b, 1]), P[b, a, :] ./ (head[a, 1] .* head[b, :]))

function find_groups(dmat, K, L)  # separable.jl:191-211
    groups = [Int[] for k in 1:K]
    ungrouped = collect(1:L*K)
    for k in 1:K
        push!(groups[k], pop!(ungrouped))
        while length(groups[k]) < L
            _, i = findmax(vec(sum(dmat[groups[k], ungrouped], dims=1)))
            push!(groups[k], ungrouped[i])
            deleteat!(ungrouped, i)
        end
    end
    return groups
end

function find_groups_spectral(simat, K, L)  # separable.jl:214-270, binarize=false
    R = K * L
    F = eigen(Symmetric(max.(0, simat .- (sum(simat) / R^2))))
    V = F.vectors
    free = trues(R)
    groups = Vector{Int}[]
    for k in 0:K-1
        v = V[:, R-k]
        abs(maximum(v)) < abs(minimum(v)) && (v = -v)
        priority = sort(findall(free), by=j -> v[j], rev=true)
        push!(groups, priority[1:L])
        free[priority[1:L]] .= false
    end
    return groups
end

function arg_shift_max(left, right)  # separable.jl:112-131
    arg, best = 0, 0.0
    for l in 0:length(left)-1
        left[l+1] > best && ((best, arg) = (left[l+1], l))
        right[l+1] > best && ((best, arg) = (right[l+1], -l))
    end
    return arg
end

function sort_group(group, P, head)  # separable.jl:96-109
    weight = [sum(arg_shift_max(cos_ab(P, head, a, b)...) for b in group) for a in group]
    return group[sort(collect(1:length(group)), by=j -> -weight[j])]
end

function projection(handle, N, R, thresh, pre)  # pre_svd / pre_svdcond (separable.jl:323-333) from eigen(X X')
    XXt = zeros(N, N)
    check(ccall((:cmf_sep_gram, LIBCMF), Cint, (Ptr{Cvoid}, Float64, Ptr{Float64}), handle, thresh, XXt))
    F = eigen(Symmetric(XXt))
    U = F.vectors[:, end:-1:end-R+1]
    S = sqrt.(F.values[end:-1:end-R+1])
    return pre == :svd ? U : U ./ S'   # N x R: column r is row r of the matrix SPA multiplies X by (any sign: SPA does not see it)
end

function fit(data, K, L; thresh=0, verbose=false, refit_H=false, refit_W=false, refit_H_itr=10, spectral=false, pre=nothing,
             nnls_large::Bool=false, device::Integer=parse(Int, get(ENV, "LOCAL_RANK", "0")), kwargs...)
    pre in (nothing, :svd, :svdcond) || throw(ArgumentError("pre must be nothing, :svd or :svdcond"))
    d = Matrix{Float64}(data)
    N, T = size(d)
    R = K * L
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cmf_create, LIBCMF), Cint, (Ref{Ptr{Cvoid}}, Cint, Int64, Int64, Int64, Int64, Ptr{Float64}), h, device, N, T, K, L, d))
    W, H = zeros(K, N, L), zeros(K, T)
    try
        check(ccall((:cmf_sep_prepare, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}), h[], d))
        nnls_large && check(ccall((:cmf_set_option, LIBCMF), Cint, (Ptr{Cvoid}, Cstring, Cint), h[], "nnls_large", 1))
        proj = pre === nothing ? Ptr{Float64}(C_NULL) : projection(h[], N, R, Float64(thresh), pre)
        vertices = zeros(Int64, R)
        check(ccall((:cmf_sep_spa, LIBCMF), Cint, (Ptr{Cvoid}, Int64, Float64, Cint, Ptr{Float64}, Ptr{Int64}),
                    h[], R, thresh, pre === nothing ? 0 : (pre == :svd ? 1 : 2), proj, vertices))
        V, G = zeros(N, R), zeros(R, T)
        check(ccall((:cmf_sep_nnls, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}), h[], vertices, R, V, G))
        P, head = zeros(R, R, L), zeros(R, L)
        check(ccall((:cmf_sep_shift_table, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                    h[], G, R, L, P, head))
        dmat = [max(0.0, maximum(cos_ab(P, head, r, p)[1]), maximum(cos_ab(P, head, r, p)[2])) for r in 1:R, p in 1:R]
        dmat = [r <= p ? dmat[r, p] : dmat[p, r] for r in 1:R, p in 1:R]  # separable.jl:144-150 fills from the upper triangle
        groups = spectral ? find_groups_spectral(dmat, K, L) : find_groups(dmat, K, L)
        groups = [sort_group(g, P, head) for g in groups]
        g0 = Int64[groups[k][l] - 1 for k in 1:K, l in 1:L]
        check(ccall((:cmf_sep_construct, LIBCMF), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                    h[], V, G, g0, W, H))
    finally
        ccall((:cmf_destroy, LIBCMF), Cint, (Ptr{Cvoid},), h[])
    end
    if refit_W                                                                    # separable.jl:41-43
        anls = HIPANLSUpdate(d, W, H; device=device)
        nnls_large && set_option!(anls, "nnls_large", 1)
        update_motifs!(anls, d, W, H)
    end
    if refit_H                                                                    # separable.jl:46-52
        rule = HIPHALSUpdate(d, W, H; device=device)
        for itr in 1:refit_H_itr
            update_feature_maps!(rule, d, W, H; l1H=0, l2H=0)
        end
    end
    return W, H
end

end # module HIPSeparable

end # module
