"""Host-side mirror of CMF.jl's interface for the multiplicative-update path.

The reference host language is Julia, which is not available where this is built,
so the host layer above the C ABI is written in Python with the reference's own
names, argument meaning and loop semantics (the Julia ``ccall`` twin of this file
is cmf.jl_amd/julia/CMFHip.jl, shown in INTEGRATION.md).  Citations are relative to
the reference checkout.

    fit_cnmf(data; L, K, alg=:mult, max_itr, max_time, l1_*, l2_*, seed, ...)   src/model.jl:58-85
    CNMF_results(data, W, H, time_hist, loss_hist)                                src/model.jl:11-30
    init_rand(data, L, K)                                                         src/model.jl:113-125
    converged(loss_hist, patience, tol)                                           src/model.jl:91-107
    AlternatingOptimizer / fit                                                    src/algs/alternating.jl:10-71
    MultUpdate: ctor, update_motifs!, update_feature_maps!                        src/algs/mult.jl:1-58
    tensor_conv / tensor_transconv / compute_loss                                 src/common.jl:17-81
    gen_synthetic                                                                 README.md:14, datasets/synthetic.jl:29-61
    separable_fit (alg=:sep), gen_sep_data, cos_score, permute_factors, ...       src/algs/separable.jl:14-56, :422-483, datasets/sep.jl:4-39

Arrays use Julia's index order: ``data[n, t]`` (N,T), ``W[k, n, l]`` (K,N,L), ``H[k, t]`` (K,T).
The arithmetic on the data runs on the GPU through libcmf_hip.so; the host decides only on small tables (the grouping of the
separable fit, R x R numbers).
"""
from __future__ import annotations

import ctypes
import math
import os
import time
import warnings

import numpy as np

from . import _lib
from ._lib import CMFError, check, farr, ptr

EPSILON = float(np.finfo(np.float64).eps)  # src/CMF.jl:20


# --------------------------------------------------------------------------------------
# results
# --------------------------------------------------------------------------------------
class CNMF_results:
    """Holds results from a single CNMF fit (src/model.jl:11-17)."""

    def __init__(self, data, W, H, time_hist, loss_hist):
        self.data = data
        self.W = W
        self.H = H
        self.time_hist = time_hist
        self.loss_hist = loss_hist

    # accessors: src/model.jl:21-30
    def num_lags(self):
        return self.W.shape[2]

    def num_units(self):
        return self.W.shape[1]

    def num_components(self):
        return self.W.shape[0]

    def num_iter(self):
        return len(self.loss_hist)


# --------------------------------------------------------------------------------------
# stand-alone primitives (src/common.jl)
# --------------------------------------------------------------------------------------
def _dims(W, H=None, X=None):
    K, N, L = W.shape
    T = H.shape[1] if H is not None else X.shape[1]
    return N, T, K, L


def tensor_conv(W, H, device=None):
    """tensor_conv(W, H) -> est (N x T): src/common.jl:17-34."""
    lib = _lib.load()
    W = farr(W)
    N, T, K, L = _dims(W, H=np.asarray(H))
    H = farr(H, (K, T))
    est = np.zeros((N, T), order="F")
    check(lib.cmf_tensor_conv(_dev(device), N, T, K, L, ptr(W), ptr(H), ptr(est)))
    return est


def tensor_transconv(W, X, device=None):
    """tensor_transconv(W, X) -> (K x T): src/common.jl:62-81."""
    lib = _lib.load()
    W = farr(W)
    N, T, K, L = _dims(W, X=np.asarray(X))
    X = farr(X, (N, T))
    out = np.zeros((K, T), order="F")
    check(lib.cmf_tensor_transconv(_dev(device), N, T, K, L, ptr(W), ptr(X), ptr(out)))
    return out


def compute_loss(data, W, H, device=None):
    """compute_loss(data, W, H): src/common.jl:54-59.  For an event list (EventData or an object with ``.tocoo()``) the loss of the
    only rule that fits one: the KL loss D(data, est + eps) / sum(data) of EventKLUpdate."""
    events = _as_events(data)
    if events is not None:
        rule = EventKLUpdate(events, W, H, device=device)
        try:
            return rule.compute_loss()
        finally:
            rule.close()
    rule = MultUpdate(data, W, H, device=device)
    try:
        return rule.compute_loss()
    finally:
        rule.close()


def converged(loss_hist, patience, tol):
    """Check for model convergence: src/model.jl:91-107."""
    lib = _lib.load()
    lh = np.ascontiguousarray(loss_hist, dtype=np.float64)
    return bool(lib.cmf_converged(ptr(lh), len(lh), int(patience), float(tol)))


def _dev(device):
    return _lib.default_device() if device is None else int(device)


def rccl_version():
    """{"version": code, "lib": path} of the RCCL this process binds (cmf_rccl_version); raises CMFError without one."""
    lib = _lib.load()
    v = ctypes.c_int()
    buf = ctypes.create_string_buffer(1024)
    check(lib.cmf_rccl_version(ctypes.byref(v), buf, 1024))
    return {"version": v.value, "lib": buf.value.decode()}


# --------------------------------------------------------------------------------------
# update rules (the plugin boundary: abstract type AbstractCFUpdate, alternating.jl:1-8)
# --------------------------------------------------------------------------------------
# CMF_DIV_SQUARE, CMF_DIV_KL, CMF_DIV_IS (include/cmf_hip.h); ":beta" is no kind of cmf_mu_set_divergence: it has an entry of its
# own, cmf_mu_set_beta_divergence, and is numbered here only
_DIVERGENCES = {":square": 0, "square": 0, ":kl": 1, "kl": 1, ":itakura_saito": 2, "itakura_saito": 2, ":beta": 3, "beta": 3}
_DIV_KL = 1
_DIV_IS = 2
_DIV_BETA = 3
_DIV_NAMES = {0: ":square", 1: ":kl", 2: ":itakura_saito", 3: ":beta"}
# per divergence form: its label in fit_cnmf's messages, the library option that lets it run under mask=, the KL text's "yet"
_DIV_FIT = {_DIV_KL: ("KL", "kl_mask", " yet"), _DIV_IS: ("Itakura-Saito", "pq_mask", ""), _DIV_BETA: ("beta-divergence", "pq_mask", "")}
BETA_WINDOW = 0.01  # CMF_BETA_WINDOW (include/cmf_hip.h; profiles/mu_beta_precision.txt: window)
BETA_MAX = 4.0      # CMF_BETA_MAX


def _divergence_kind(kind):
    key = kind if isinstance(kind, str) else (":" + getattr(kind, "name", str(kind)))
    if key not in _DIVERGENCES:
        raise ValueError(f"divergence must be ':square' or ':kl' (or ':itakura_saito', spelled out, or ':beta' with beta=), got {kind!r}")
    return _DIVERGENCES[key]


def _check_beta(kind_code, beta):
    """The beta of divergence=":beta" as cmf_mu_set_beta_divergence accepts it (the library's wording), or None for the other kinds."""
    if kind_code != _DIV_BETA:
        if beta is not None:
            raise ValueError("beta= goes with divergence=':beta' only")
        return None
    if beta is None:
        raise ValueError("divergence=':beta' needs beta=")
    b = float(beta)
    w = BETA_WINDOW * (1.0 - 1e-9)  # (the window's edges are accepted)
    if not math.isfinite(b):
        raise ValueError("beta must be finite")
    if b == 0.0 or b == 1.0:
        raise ValueError(f"beta = {b:g} is CMF_DIV_IS (beta = 0) or CMF_DIV_KL (beta = 1): the beta formula is 0/0 there, use "
                         "divergence=':itakura_saito' or ':kl'")
    if b < 0.0 or b > BETA_MAX:
        raise ValueError(f"beta must lie in (0, {BETA_MAX:g}], got {b!r}")
    if b < w or abs(b - 1.0) < w:
        raise ValueError(f"beta = {b!r} lies within {BETA_WINDOW:g} of 0 or 1, where the float32 loss loses its digits to the factor "
                         f"1 / (beta (beta - 1)): use CMF_DIV_IS / CMF_DIV_KL, or a beta at least {BETA_WINDOW:g} away")
    return b


_XORTHO_KW = ("lambda_xortho", "lambda_ortho_H", "lambda_ortho_W")


def _check_xortho(*weights):
    """The three penalty weights as cmf_mu_set_xortho accepts them: finite and >= 0."""
    out = []
    for name, w in zip(_XORTHO_KW, weights):
        w = float(w)
        if not math.isfinite(w) or w < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, got {w!r}")
        out.append(w)
    return tuple(out)


class AbstractCFUpdate:
    """An update rule that updates both W and H (src/algs/alternating.jl:1-8).

    Must implement ``Rule(data, W, H)``, ``update_motifs(data, W, H, **kwargs)`` and
    ``update_feature_maps(data, W, H, **kwargs) -> loss``.
    """


class MultUpdate(AbstractCFUpdate):
    """MultUpdate on MI355X: drop-in for src/algs/mult.jl behind the rule interface.

    ``MultUpdate(data, W, H)`` mirrors the reference constructor (mult.jl:11-20): it
    uploads ``data`` and the factors and owns the rule's scratch (est, numW, denomW,
    numH, denomH) on the device.  The working copies of W and H stay device-resident
    between calls; ``update_motifs`` / ``update_feature_maps`` advance them, and
    :meth:`download` writes them back into the caller's arrays (``fit`` does this
    once at the end, which is observably the same as the reference's in-place
    mutation for every caller that only reads W and H after ``fit`` returns).  If the
    caller changes W or H on the host between calls, it must call :meth:`upload`.

    ``devices=[d0, d1, ...]`` builds the rule as a T-sharded group on several GPUs of this node, driven by this one
    process (cmf_create_multi): the rule methods keep their meaning and the library runs the sharded iteration --
    ONE RCCL all-reduce of [numW | denomW | loss tail | H halos] per iteration (the Gram form and PGD keep
    an H-halo all-gather of their own).  Listing
    one device several times puts that many shards on it (loopback transport; tests).
    """

    def __init__(self, data, W, H, device=None, devices=None, transport=_lib.CMF_COMM_AUTO, sync_every_call=None, verify_args=None,
                 strict_inplace=None):
        lib = _lib.load()
        self._lib = lib
        for name, val in (("sync_every_call", sync_every_call), ("verify_args", verify_args), ("strict_inplace", strict_inplace)):
            if val is not None:  # (CMFHip.jl's constructor keywords; the class attributes below are the defaults)
                setattr(self, name, val)
        if self.verify_args not in ("sample", "full", "none"):
            raise ValueError('verify_args must be "sample", "full" or "none"')
        self._h = ctypes.c_void_p()
        data = farr(data)
        if data.ndim != 2:
            raise ValueError("data must be a matrix (N x T)")
        W = farr(W)
        if W.ndim != 3:
            raise ValueError("W must be a K x N x L tensor")
        K, N, L = W.shape
        if data.shape[0] != N:
            raise ValueError(f"DimensionMismatch: data has {data.shape[0]} rows, W has N={N}")
        T = data.shape[1]
        H = farr(H, (K, T))
        self.N, self.T, self.K, self.L = N, T, K, L
        if devices is not None:
            devs = [int(x) for x in devices]
            if not devs:
                raise ValueError("devices must not be empty")
            self.device, self.devices = devs[0], devs
            arr = (ctypes.c_int * len(devs))(*devs)
            check(lib.cmf_create_multi(ctypes.byref(self._h), len(devs), arr, int(transport), N, T, K, L, ptr(data)))
        else:
            self.device, self.devices = _dev(device), None
            check(lib.cmf_create(ctypes.byref(self._h), self.device, N, T, K, L, ptr(data)))
        try:
            check(lib.cmf_set_factors(self._h, ptr(W), ptr(H)))
        except Exception:
            self.close()
            raise
        ss = ctypes.c_double()
        check(lib.cmf_get_data_sumsq(self._h, ctypes.byref(ss)))
        self.data_norm = math.sqrt(ss.value)  # mult.jl:13
        # what the rule has read from the caller's arrays (the rule calls compare their arguments with it under sync_every_call)
        self._seen = {"W": self._fingerprint(W), "H": self._fingerprint(H)}

    # ``rule.sync_every_call = True`` (CMFHip.jl's default): every update_feature_maps call also writes the new factors into
    # the W and H it is handed -- the reference's in-place semantics (mult.jl:37-38,51-52) for a caller that looks at its
    # arrays between calls.  The download rides underneath the call's own kernels (cmf_arm_writeback).
    sync_every_call = False
    # The reference's rules READ their W and H arguments (mult.jl:23,42); here the working copies are device-resident.  Under
    # sync_every_call the two are kept equivalent: every rule call fingerprints the arrays it is handed (cmf_fingerprint) and
    # compares with what the rule last read from / wrote into the caller's arrays -- arrays with other contents (other arrays, or
    # the same ones edited by the caller) are uploaded first (``reuploads`` counts).  "sample": one 64-byte line per 4 KB (bulk edits -- rescaling, a new
    # initialisation, zeroed rows -- are seen, a single poked element may not be); "full": every element (+ ~1 ms per call at
    # config 2); "none": the round-5 behaviour (the caller calls upload()).
    verify_args = "sample"
    # W reaches the caller's array when update_feature_maps returns (the write-back), not when update_motifs does: in between
    # the caller's W is the one update_motifs started from.  A caller that edits W there gets a clear error -- unless
    # strict_inplace is set: update_motifs then also downloads W (synchronously: + ~0.5 ms at config 2), so the caller sees the
    # reference's state at every point and its edits are honoured like the reference's (tests/test_dropin_contract.py).
    strict_inplace = False
    reuploads = 0
    _seen = None       # {"W": fingerprint, "H": fingerprint} of the caller's arrays as this rule last read or wrote them
    _w_pending = False  # update_motifs has run and W has not been written back yet

    def _fingerprint(self, a):
        fp = ctypes.c_uint64()
        check(self._lib.cmf_fingerprint(ptr(a), a.size, 1 if self.verify_args == "full" else 64, ctypes.byref(fp)))
        return (self.verify_args, fp.value)  # (contents only, tagged with the form that was taken -- a rule switched to another form uploads once: `fit` deep-copies the initial factors, alternating.jl:33-34 -- equal arrays at another address are the same factors)

    def _check_arrays(self, W, H):
        for a, shape, nm in ((W, (self.K, self.N, self.L), "W"), (H, (self.K, self.T), "H")):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == shape
                                      and a.flags.f_contiguous and a.flags.writeable):
                raise ValueError(f"sync_every_call: {nm} must be a writeable Float64 array of shape {shape} in Julia's (column-major) order")

    def _sync_args(self, W, H):
        """The rule reads its arguments (mult.jl:23,42): arrays this rule has not seen in this state are uploaded first."""
        if not self.sync_every_call or self.verify_args == "none" or W is None or H is None:
            return
        self._check_arrays(W, H)
        now = {"W": self._fingerprint(W), "H": self._fingerprint(H)}
        if self._seen is None:  # (after upload(): the arrays a rule call is handed are taken as they are)
            self._seen = {"W": None, "H": None}
        dW, dH = now["W"] != self._seen["W"], now["H"] != self._seen["H"]
        if dW and self._w_pending:
            raise RuntimeError(
                "W was modified (or another array was passed) between update_motifs and update_feature_maps: with sync_every_call the "
                "caller's W holds the motifs update_motifs started from until update_feature_maps returns, so the edit was made to an "
                "outdated W.  Set rule.strict_inplace = True (update_motifs then writes W back and edits are honoured like the "
                "reference's, mult.jl:42), or call rule.upload(W, H) with the factors you mean (INTEGRATION.md section 3).")
        if dW or dH:
            check(self._lib.cmf_set_factors(self._h, ptr(W) if dW else None, ptr(H) if dH else None))
            self.reuploads += 1
        self._seen = now

    def _after_motifs(self, W):
        if not self.sync_every_call or self.verify_args == "none" or W is None:
            return
        if self.strict_inplace:
            self._check_arrays(W, None)
            check(self._lib.cmf_get_factors(self._h, ptr(W), None))
            if self._seen is not None:
                self._seen["W"] = self._fingerprint(W)
        else:
            self._w_pending = True

    def _after_feature_maps(self, W, H):
        if not self.sync_every_call or self.verify_args == "none" or W is None or H is None:
            return
        self._seen = {"W": self._fingerprint(W), "H": self._fingerprint(H)}  # (the write-back has just filled them)
        self._w_pending = False

    def _arm_writeback(self, W, H):
        if not self.sync_every_call or (W is None and H is None):
            return
        self._check_arrays(W, H)
        check(self._lib.cmf_arm_writeback(self._h, None if W is None else ptr(W), None if H is None else ptr(H)))

    # -- the rule under a mask (cmf_mu_set_mask) -----------------------------------------
    _mu_mask_key = None  # id() of the mask object the rule methods last installed (None: unmasked)
    _mu_mask_ref = None  # ... and the object itself, so that its id cannot be reused while it is the key

    def set_mask(self, mask):
        """Fit under a 0/1 mask (1 = observed): the multiplicative update of norm(mask .* (data - tensor_conv(W, H)))^2
        (MaskedLoss, pgd.jl:58-70, for this rule).  What ``data`` holds under ``mask == 0`` never enters, NaN included; the loss is
        norm(mask .* (est - data)) / norm(select(mask, data, 0)).  ``None`` restores the unmasked rule."""
        if mask is None:
            check(self._lib.cmf_mu_set_mask(self._h, None))
            self._mu_mask_key = self._mu_mask_ref = None
            return
        m = farr(mask)
        if m.shape != (self.N, self.T):
            raise ValueError(f"mask must be {self.N} x {self.T} like data, got {m.shape}")
        check(self._lib.cmf_mu_set_mask(self._h, ptr(m)))
        self._mu_mask_key, self._mu_mask_ref = id(mask), mask

    def _select_mask(self, kwargs):
        """``mask=`` of a rule call: installed when the object changes (compared by identity, like PGDUpdate._select_loss)."""
        if "mask" not in kwargs:
            return
        mask = kwargs["mask"]
        if (None if mask is None else id(mask)) != self._mu_mask_key:
            self.set_mask(mask)

    def masked_loss(self, complement=False):
        """(sum of (tensor_conv(W, H) - data)^2, sum of data^2) over the entries with mask == 1 -- with ``complement`` over those
        with mask == 0 -- for the resident factors (cmf_masked_loss); est, the factors and the rule's state stay as they are.
        Under ``set_divergence(":kl")`` with a mask (option "kl_mask") the pair is (sum of the divergence terms
        (x > 0 ? x log(x / e) : 0) - x + e, sum of data) over the same entries: their quotient is the KL loss on them."""
        r, d = ctypes.c_double(), ctypes.c_double()
        check(self._lib.cmf_masked_loss(self._h, int(bool(complement)), ctypes.byref(r), ctypes.byref(d)))
        return r.value, d.value

    # -- the divergence the rule minimises (cmf_mu_set_divergence) ---------------------------
    def set_divergence(self, kind, beta=None):
        """``":kl"``: the multiplicative update of the generalised Kullback-Leibler divergence (Smaragdis' convolutive NMF), for counts
        and spectrogram magnitudes: R = data ./ (est + eps) takes the place of data in the numerators, the denominators are sums of H
        and of W, and the loss is D(data, est + eps) / sum(data).  Data must be finite and non-negative with a positive sum.
        ``":square"`` restores the squared-error rule of mult.jl exactly.  Together with ``set_mask`` (either order) after
        ``set_option("kl_mask", 1)``: R = select(mask, data, 0) ./ (est + eps), the denominators are the contractions of H and of W
        with the mask, the loss runs over the observed entries, and data need be valid only where observed.
        ``":itakura_saito"``: the multiplicative update of the Itakura-Saito divergence (beta = 0), the scale-invariant objective for
        power spectrograms: with Q = 1 ./ (est + eps) and P = (data .* Q) .* Q the numerators contract P, the denominators Q, the
        update takes the square root of their quotient, and the loss is the mean of (r - 1) - log(r), r = data ./ (est + eps), per
        entry.  Data must be finite and strictly positive (add a floor to the spectrogram).  The library option "is_div" is set
        here; no mask, no Gram form, one GPU.
        ``":beta"`` with ``beta=``: the beta-divergence between those three points (cmf_mu_set_beta_divergence; beta = 0.5 for audio,
        1 < beta < 2 the Tweedie range): Q = e.^(beta - 1), P = data .* e.^(beta - 2), e = est + eps, the update raises the quotient
        to gamma(beta) (1 for 1 < beta <= 2), the loss is the mean beta-divergence per entry.  BETA_WINDOW <= beta <= BETA_MAX,
        at least BETA_WINDOW away from 1; data finite and non-negative; no mask, no Gram form, one GPU."""
        code = _divergence_kind(kind)
        beta = _check_beta(code, beta)
        if code == _DIV_BETA:
            check(self._lib.cmf_mu_set_beta_divergence(self._h, beta))
            return
        if code == _DIV_IS:
            self.set_option("is_div", 1)
        check(self._lib.cmf_mu_set_divergence(self._h, code))

    # -- seqNMF's cross-orthogonality penalties (cmf_mu_set_xortho) ---------------------------
    def set_xortho(self, lam, ortho_H=0.0, ortho_W=0.0):
        """The weights of seqNMF's penalties on the squared-error rule: ``lam`` of the cross-orthogonality term
        sum_{i != j} (transconv(W, data) S H')_ij, ``ortho_H`` of sum_{i != j} (H S H')_ij / 2 and ``ortho_W`` of
        sum_{i != j} (Wflat' Wflat)_ij / 2 (S: the box smoothing of width 2L - 1 along time).  Each rule call then adds the term's
        gradient to its denominator (include/cmf_hip.h has the formulas); the loss stays norm(est - data) / norm(data).  All zeros
        restore the plain rule launch for launch.  One GPU, no mask, no divergence, no Gram form."""
        w = _check_xortho(lam, ortho_H, ortho_W)
        check(self._lib.cmf_mu_set_xortho(self._h, *w))

    def xortho_cost(self):
        """(xortho, ortho_H, ortho_W): the three penalty sums of the resident factors without their weights and without the 1/2
        (cmf_mu_xortho_cost; fp64 sums)."""
        c = [ctypes.c_double() for _ in range(3)]
        check(self._lib.cmf_mu_xortho_cost(self._h, *[ctypes.byref(v) for v in c]))
        return tuple(v.value for v in c)

    def xortho_terms(self):
        """(xW, xH, oH, oW): the four unweighted denominator terms for the resident factors, in the shapes of W, H, H and W
        (cmf_mu_xortho_terms)."""
        K, N, L, T = self.K, self.N, self.L, self.T
        xW, oW = np.zeros((K, N, L), order="F"), np.zeros((K, N, L), order="F")
        xH, oH = np.zeros((K, T), order="F"), np.zeros((K, T), order="F")
        check(self._lib.cmf_mu_xortho_terms(self._h, ptr(xW), ptr(xH), ptr(oH), ptr(oW)))
        return xW, xH, oH, oW

    # -- seqNMF's significance test on held-out data (cmf_null_moments) ------------------------
    def null_moments(self, seed, first_draw, n_draws):
        """The raw power sums of the overlaps of the null motifs of the resident W with the rule's data, a (3, K, n_draws) array:
        ``[:, k, j]`` = (sum v, sum v^2, sum v^3) over the columns, v = tensor_transconv(Wnull_d, data)[k, :] of draw
        d = first_draw + j, whose motif rows are circularly shifted by ``null_shifts``; draw 0 is the resident W itself.
        Changes nothing the rule calls read (cmf_null_moments)."""
        n_draws = int(n_draws)
        sums = np.zeros((3, self.K, max(n_draws, 0)), order="F")
        check(self._lib.cmf_null_moments(self._h, int(seed) & (2**64 - 1), int(first_draw), n_draws, ptr(sums)))
        return sums

    # -- seqNMF's re-centring of motifs (cmf_mu_set_recentre, cmf_recentre) ---------------------
    def set_recentre(self, on):
        """``True``: every update_feature_maps (and every iteration of ``iterate`` / ``fit_native`` outside eval mode) moves each
        motif's centre of mass back to the middle of the L-lag window and its row of H the other way, between the update of H and the
        loss conv (seqNMF's shiftFactors; include/cmf_hip.h has the definition).  On the device, inside the iteration; a step whose
        shifts are all zero moves nothing.  One GPU, not with the Gram form.  ``False`` restores the plain rule launch for launch."""
        check(self._lib.cmf_mu_set_recentre(self._h, int(bool(on))))

    def recentre(self):
        """One re-centring step on the resident factors, whatever produced them (cmf_recentre): the K shifts as an int32 array.
        The caller's arrays are not touched: :meth:`download` fetches the moved factors."""
        s = np.zeros(self.K, dtype=np.int32)
        check(self._lib.cmf_recentre(self._h, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return s

    def recentre_info(self):
        """(last_shifts, moved): the K shifts of the most recent step and the per-component totals of |s_k| since the rule was made
        (cmf_mu_recentre_info; synchronises)."""
        s, m = np.zeros(self.K, dtype=np.int32), np.zeros(self.K, dtype=np.int64)
        check(self._lib.cmf_mu_recentre_info(self._h, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return s, m

    # -- the two rule methods -----------------------------------------------------------
    def update_motifs(self, data=None, W=None, H=None, l1W=0, l2W=0, **kwargs):
        """update_motifs!(rule, data, W, H; l1W=0, l2W=0, mask=nothing): src/algs/mult.jl:23-39."""
        self._select_mask(kwargs)
        self._sync_args(W, H)
        check(self._lib.cmf_update_motifs(self._h, float(l1W), float(l2W)))
        self._after_motifs(W)

    def update_feature_maps(self, data=None, W=None, H=None, l1H=0, l2H=0, **kwargs):
        """update_feature_maps!(rule, data, W, H; l1H=0, l2H=0, mask=nothing) -> loss: src/algs/mult.jl:42-58."""
        loss = ctypes.c_double()
        self._select_mask(kwargs)
        self._sync_args(W, H)
        self._arm_writeback(W, H)
        check(self._lib.cmf_update_feature_maps(self._h, float(l1H), float(l2H), ctypes.byref(loss)))
        self._after_feature_maps(W, H)
        return loss.value

    # -- helpers ------------------------------------------------------------------------
    def compute_loss(self):
        """compute_loss(data, W, H) on the resident factors: src/common.jl:54-59."""
        loss = ctypes.c_double()
        check(self._lib.cmf_compute_loss(self._h, ctypes.byref(loss)))
        return loss.value

    def iterate(self, n, eval_mode=False, l1W=0, l2W=0, l1H=0, l2H=0, stamps=False):
        """n x (update_motifs!; update_feature_maps!) back to back (alternating.jl:51-54) in one ccall (cmf_iterate):
        the losses of the n iterations, read one iteration late so the device never waits for the host."""
        losses = np.zeros(int(n))
        st = np.zeros(int(n))
        check(self._lib.cmf_iterate(self._h, int(n), int(bool(eval_mode)), float(l1W), float(l2W), float(l1H), float(l2H),
                                    ptr(losses), ptr(st)))
        return (losses, st) if stamps else losses

    def synchronize(self):
        """Wait for everything the rule has enqueued (every stream of every local shard of a group)."""
        check(self._lib.cmf_synchronize(self._h))

    def counter(self, name):
        """Event counter of the handle (cmf_get_counter), e.g. "hals_pipeline_reruns"."""
        v = ctypes.c_int64()
        check(self._lib.cmf_get_counter(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    overlap = False
    transport_fallback = None

    def set_overlap(self, flag):
        """Group handles: switch between the two forms of the W phase (library option "allreduce_overlap")."""
        self.set_option("allreduce_overlap", int(bool(flag)))
        self.overlap = bool(flag)

    def comm_info(self):
        buf = ctypes.create_string_buffer(1024)
        check(self._lib.cmf_comm_info(self._h, buf, 1024))
        return buf.value.decode()

    def shard_bounds(self, rank):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.cmf_shard_bounds(self._h, int(rank), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_option(self, name, value):
        """Library option, e.g. ``set_option("reuse_est", 0)`` to recompute est in update_motifs! like the reference."""
        check(self._lib.cmf_set_option(self._h, name.encode(), int(value)))

    def upload(self, W, H):
        W = farr(W, (self.K, self.N, self.L))
        H = farr(H, (self.K, self.T))
        check(self._lib.cmf_set_factors(self._h, ptr(W), ptr(H)))
        self._seen, self._w_pending = None, False  # (the next rule call takes the arrays it is handed as they are)

    def download(self, W=None, H=None):
        """Write the resident factors into W, H (in place when given) and return them."""
        Wf = np.zeros((self.K, self.N, self.L), order="F")
        Hf = np.zeros((self.K, self.T), order="F")
        check(self._lib.cmf_get_factors(self._h, ptr(Wf), ptr(Hf)))
        if W is not None:
            W[...] = Wf
            Wf = W
        if H is not None:
            H[...] = Hf
            Hf = H
        return Wf, Hf

    def fit_native(self, max_itr, max_time, check_convergence, patience, tol, eval_mode,
                   l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0):
        """The whole alternating.jl:16-71 loop inside the library (one ccall)."""
        lh = np.zeros(int(max_itr) + 1)
        th = np.zeros(int(max_itr) + 1)
        n = ctypes.c_int64(0)
        early = ctypes.c_int(0)
        check(self._lib.cmf_fit(self._h, int(max_itr), float(max_time), int(bool(check_convergence)), int(patience),
                                float(tol), int(bool(eval_mode)), float(l1W), float(l2W), float(l1H), float(l2H),
                                ptr(lh), ptr(th), ctypes.byref(n), ctypes.byref(early)))
        return lh[: n.value].copy(), th[: n.value].copy(), bool(early.value)

    def kernel_times(self, name):
        """(mean ms, launches) recorded for one kernel class since set_option("profile", 1)."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        check(self._lib.cmf_kernel_times(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def time_kernel(self, name, reps=5):
        """(avg ms, algorithmic flops per launch) of one hot kernel, timed with HIP events."""
        ms, fl = ctypes.c_double(), ctypes.c_double()
        check(self._lib.cmf_time_kernel(self._h, name.encode(), int(reps), ctypes.byref(ms), ctypes.byref(fl)))
        return ms.value, fl.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.cmf_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


HIPMultUpdate = MultUpdate


# --------------------------------------------------------------------------------------
# the KL form of the MU rule on an event list (cmf_events_*, include/cmf_hip.h)
# --------------------------------------------------------------------------------------
class EventData:
    """Sparse counts as an event list: ``data[unit[j], time[j]] = count[j]`` of an N x T matrix that is zero elsewhere.

    ``EventData(unit, time, count, shape)`` validates and sorts by (unit, time), sums duplicates in fp64 in input order and
    drops exact zeros; a negative or non-finite count and an index outside ``shape`` are refused.  ``unit`` / ``time`` are
    then int32 and ``count`` float64 arrays of length ``nnz`` in the order cmf_events_create takes."""

    def __init__(self, unit, time, count, shape):
        N, T = (int(s) for s in shape)
        if N < 1 or T < 1:
            raise ValueError(f"shape must be (N, T) with N, T >= 1, got {tuple(shape)}")
        unit, time = np.asarray(unit), np.asarray(time)
        count = np.asarray(count, dtype=np.float64)
        if unit.ndim != 1 or unit.shape != time.shape or unit.shape != count.shape:
            raise ValueError("unit, time and count must be vectors of one length")
        for name, a in (("unit", unit), ("time", time)):
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{name} must hold integers")
        unit, time = unit.astype(np.int64), time.astype(np.int64)
        if unit.size and (unit.min() < 0 or unit.max() >= N or time.min() < 0 or time.max() >= T):
            raise ValueError(f"an event lies outside the {N} x {T} matrix (index out of range)")
        if not np.isfinite(count).all():
            raise ValueError("counts must be finite (got NaN or infinity)")
        if (count < 0).any():
            raise ValueError("counts must not be negative")
        keep = count != 0.0  # exact zeros are no events
        unit, time, count = unit[keep], time[keep], count[keep]
        key = unit * T + time
        order = np.argsort(key, kind="stable")  # (stable: duplicates stay in input order)
        key, count = key[order], count[order]
        first = np.ones(key.size, dtype=bool)
        first[1:] = key[1:] != key[:-1]
        group = np.cumsum(first) - 1
        summed = np.zeros(int(first.sum()))
        np.add.at(summed, group, count)  # (one addition after the other, in input order)
        if not np.isfinite(summed).all():
            raise ValueError("the sum of duplicate events is not finite")
        key = key[first]
        self.shape = (N, T)
        self.unit = (key // T).astype(np.int32)
        self.time = (key % T).astype(np.int32)
        self.count = summed

    @property
    def nnz(self):
        return int(self.count.size)

    def sum(self):
        return float(np.sum(self.count))

    def todense(self):
        a = np.zeros(self.shape, order="F")
        a[self.unit, self.time] = self.count
        return a

    @classmethod
    def from_dense(cls, a):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError("data must be a matrix (N x T)")
        if not np.isfinite(a).all():
            raise ValueError("counts must be finite (got NaN or infinity)")
        unit, time = np.nonzero(a)
        return cls(unit, time, a[unit, time], a.shape)

    @classmethod
    def from_sparse(cls, m):
        """Any object with ``.tocoo()`` giving ``row`` (unit), ``col`` (time), ``data`` and ``shape`` (scipy.sparse matrices do;
        the package itself never imports scipy)."""
        c = m.tocoo()
        return cls(np.asarray(c.row), np.asarray(c.col), np.asarray(c.data), tuple(c.shape))


def _as_events(data):
    """EventData for an EventData or an object with ``.tocoo()``; None for anything else."""
    if isinstance(data, EventData):
        return data
    if hasattr(data, "tocoo") and not isinstance(data, np.ndarray):
        return EventData.from_sparse(data)
    return None


def _events_sum_est(W, H):
    """The sum of tensor_conv(W, H) over ALL N x T entries from the sums of W over n and of H over t (no N x T array):
    sum_k sum_{l < min(L, T)} (sum_n W[k, n, l]) (sum_{t < T - l} H[k, t])."""
    K, N, L = W.shape
    T = H.shape[1]
    wsum = np.sum(W, axis=1)  # K x L
    hcum = np.concatenate([np.zeros((K, 1)), np.cumsum(H, axis=1)], axis=1)  # hcum[k, m] = sum of the first m columns
    lags = np.arange(min(L, T))
    return float(np.sum(wsum[:, lags] * hcum[:, T - lags]))


def _rng_u01(seed, stream, n):
    """The library's counter RNG (csrc/cmf_rng.h: u01 of stream `stream`, counters 0 .. n-1) -- the draws cmf_init_rand takes."""
    m64 = (1 << 64) - 1

    def mix(z):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    with np.errstate(over="ignore"):
        base = mix(np.array([(int(seed) + 0x632BE59BD9B4E019 * (stream + 1)) & m64], dtype=np.uint64))[0]
        i = np.arange(1, n + 1, dtype=np.uint64)
        bits = mix(base + i * np.uint64(0x9E3779B97F4A7C15))
    return (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def init_rand_events(events, L, K, seed=None):
    """init_rand (src/model.jl:113-125) for an event list: the same uniform draws as ``init_rand`` takes for that seed, scaled by
    sqrt(alpha) with alpha = sum(x) / sum_all(est) -- the scalar that minimises the KL divergence, from the closed form of the
    sum of est.  (``init_rand``'s least-squares alpha needs norm(est)^2, a dense quantity; a seeded event fit therefore starts
    elsewhere than the seeded dense fit of the same data: the draws agree, the scale does not.)  Host arithmetic only."""
    ev = _as_events(events)
    if ev is None:
        raise TypeError("init_rand_events takes an EventData or an object with .tocoo()")
    N, T = ev.shape
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    seed = int(seed) & (2**64 - 1)
    W = _rng_u01(seed, 0, K * N * L).reshape((K, N, L), order="F")
    H = _rng_u01(seed, 1, K * T).reshape((K, T), order="F")
    s = math.sqrt(abs(ev.sum() / _events_sum_est(W, H)))
    return np.asfortranarray(W * s), np.asfortranarray(H * s)


class EventKLUpdate(AbstractCFUpdate):
    """The KL form of the MU rule (``MultUpdate`` with ``set_divergence(":kl")``) on sparse counts given as an event list: the same
    rule, with every sum over the data taken over its non-zero entries (cmf_events_*, include/cmf_hip.h).  Nothing of size N x T
    is allocated on the device or the host.

    ``EventKLUpdate(data, W, H)`` takes an :class:`EventData` (or an object with ``.tocoo()``) and keeps working copies of W and
    H on the device; ``update_feature_maps`` writes both back into the arrays it is handed, like the fp64 rules.  One GPU."""

    def __init__(self, data, W, H, device=None, devices=None):
        if devices is not None:
            raise NotImplementedError("EventKLUpdate runs on one GPU: devices=[...] (T sharding) is not available for event lists")
        ev = _as_events(data)
        if ev is None:
            raise TypeError("EventKLUpdate takes an EventData or an object with .tocoo() (dense data: MultUpdate with set_divergence(':kl'))")
        if ev.nnz < 1:
            raise ValueError("the KL divergence needs data with a positive sum: the event list is empty")
        lib = _lib.load()
        self._lib = lib
        self._h = ctypes.c_void_p()
        W = farr(W)
        if W.ndim != 3:
            raise ValueError("W must be a K x N x L tensor")
        K, N, L = W.shape
        if ev.shape[0] != N:
            raise ValueError(f"DimensionMismatch: data has {ev.shape[0]} rows, W has N={N}")
        T = ev.shape[1]
        H = farr(H, (K, T))
        self.N, self.T, self.K, self.L = N, T, K, L
        self.data, self.nnz = ev, ev.nnz
        self.device = _dev(device)
        i32 = ctypes.POINTER(ctypes.c_int32)
        unit, time = np.ascontiguousarray(ev.unit, dtype=np.int32), np.ascontiguousarray(ev.time, dtype=np.int32)
        count = np.ascontiguousarray(ev.count, dtype=np.float64)
        check(lib.cmf_events_create(ctypes.byref(self._h), self.device, N, T, K, L, ev.nnz, unit.ctypes.data_as(i32), time.ctypes.data_as(i32),
                                    ptr(count)))
        try:
            check(lib.cmf_events_set_factors(self._h, ptr(W), ptr(H)))
        except Exception:
            self.close()
            raise

    def update_motifs(self, data=None, W=None, H=None, l1W=0, l2W=0, **kwargs):
        """update_motifs! of the KL rule at the events (mult.jl:23-39 with data -> R).  The new W reaches the caller's array with
        the next update_feature_maps."""
        check(self._lib.cmf_events_update_motifs(self._h, float(l1W), float(l2W)))

    def update_feature_maps(self, data=None, W=None, H=None, l1H=0, l2H=0, **kwargs):
        """update_feature_maps! of the KL rule at the events -> loss (mult.jl:42-58); W and H, when given, receive the new factors."""
        loss = ctypes.c_double()
        check(self._lib.cmf_events_update_feature_maps(self._h, float(l1H), float(l2H), ctypes.byref(loss)))
        if W is not None or H is not None:
            self.download(W, H)
        return loss.value

    def compute_loss(self):
        """D(data, est + eps) / sum(data) of the resident factors, the sum of est from its closed form."""
        loss = ctypes.c_double()
        check(self._lib.cmf_events_compute_loss(self._h, ctypes.byref(loss)))
        return loss.value

    def iterate(self, n, eval_mode=False, l1W=0, l2W=0, l1H=0, l2H=0):
        """n x (update_motifs!; update_feature_maps!) in one call (cmf_events_iterate): the n losses."""
        losses = np.zeros(int(n))
        check(self._lib.cmf_events_iterate(self._h, int(n), int(bool(eval_mode)), float(l1W), float(l2W), float(l1H), float(l2H), ptr(losses)))
        return losses

    def upload(self, W, H):
        W = farr(W, (self.K, self.N, self.L))
        H = farr(H, (self.K, self.T))
        check(self._lib.cmf_events_set_factors(self._h, ptr(W), ptr(H)))

    def download(self, W=None, H=None):
        """Write the resident factors into W, H (in place when given) and return them."""
        Wf = np.zeros((self.K, self.N, self.L), order="F")
        Hf = np.zeros((self.K, self.T), order="F")
        check(self._lib.cmf_events_get_factors(self._h, ptr(Wf), ptr(Hf)))
        if W is not None:
            W[...] = Wf
            Wf = W
        if H is not None:
            H[...] = Hf
            Hf = H
        return Wf, Hf

    def terms(self):
        """(ratio, numW, numH, denomW, denomH) of both updates for the resident factors, the fp32 values the update kernels
        read (cmf_events_terms): ratio has one value per event in the order of ``data``."""
        K, N, L, T = self.K, self.N, self.L, self.T
        ratio = np.zeros(self.nnz)
        numW, denW = np.zeros((K, N, L), order="F"), np.zeros((K, N, L), order="F")
        numH, denH = np.zeros((K, T), order="F"), np.zeros((K, T), order="F")
        check(self._lib.cmf_events_terms(self._h, ptr(ratio), ptr(numW), ptr(numH), ptr(denW), ptr(denH)))
        return ratio, numW, numH, denW, denH

    def counter(self, name):
        v = ctypes.c_int64()
        check(self._lib.cmf_events_get_counter(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def set_option(self, name, value):
        """"unit_chunk", "time_chunk", "keep_ratio" (cmf_events_set_option)."""
        check(self._lib.cmf_events_set_option(self._h, name.encode(), int(value)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.cmf_events_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fit_cnmf_events(events, L, K, rule_type, max_itr, max_time, kw, device, devices, options):
    """fit_cnmf for an event list: the refusals (before anything touches a device), init_rand_events, the ordinary fit() loop."""
    if rule_type is not MultUpdate:
        raise NotImplementedError("event data is fitted by alg=:mult with divergence=':kl' only: the other rules have no event form")
    div = kw.get("divergence", ":square")
    if _divergence_kind(div) != _DIV_KL:
        raise NotImplementedError(f"event data is fitted with divergence=':kl' only (got {div!r}): the sums of the squared-error, "
                                  "Itakura-Saito and beta forms do not collapse onto the events")
    if kw.get("mask", None) is not None:
        raise NotImplementedError("mask= is not available for event data: the event form of the KL rule has no masked form")
    if any(_check_xortho(*[kw.get(k, 0.0) for k in _XORTHO_KW])):
        raise NotImplementedError("lambda_xortho / lambda_ortho_H / lambda_ortho_W are not available for event data: the "
                                  "cross-orthogonality penalties run on the squared-error MU rule")
    if devices is not None:
        raise NotImplementedError("devices=[...] (T sharding) is not available for event data: the event form runs on one GPU")
    W_init, H_init = init_rand_events(events, L, K, seed=kw.get("seed", None))  # :70 (always runs, like the reference)
    W_init = kw.get("W_init", W_init)
    H_init = kw.get("H_init", H_init)
    rule = EventKLUpdate(events, W_init, H_init, device=device)
    try:
        for name, value in (options or {}).items():
            rule.set_option(name, value)
        opt = AlternatingOptimizer(rule, max_itr, max_time)
        loop_kw = {k: v for k, v in kw.items() if k not in ("seed", "W_init", "H_init", "divergence", "beta", "mask") + _XORTHO_KW}
        return fit(opt, events, L, K, W_init, H_init, **loop_kw)
    finally:
        rule.close()


class HALSUpdate(MultUpdate):
    """HALSUpdate on MI355X: drop-in for src/algs/hals.jl behind the same rule interface.

    ``HALSUpdate(data, W, H)`` mirrors hals.jl:18-28.  The residual the reference carries in the
    rule (``resids = tensor_conv(W, H) - data``) is kept implicitly (est on the device); the K*L column
    updates of W (hals.jl:90-112) and the K*T entry updates of H (hals.jl:121-154) run in the
    reference's Gauss-Seidel order on Gram-projected state (see cmf_kernels.h).  Clamp at 0,
    ``+ l2`` regularisation and the incremental-residual loss are the reference's.
    """

    def __init__(self, data, W, H, device=None, **kw):
        super().__init__(data, W, H, device=device, **kw)
        try:  # the rule constructor (hals.jl:18-28): scratch + the shape limits of the on-chip sweeps, reported here
            self.set_option("hals_prepare", 1)
        except Exception:
            self.close()
            raise

    def update_motifs(self, data=None, W=None, H=None, l1W=0, l2W=0, **kwargs):
        """update_motifs!(rule::HALSUpdate, data, W, H; l1W=0, l2W=0): src/algs/hals.jl:31-34."""
        self._sync_args(W, H)
        check(self._lib.cmf_hals_update_motifs(self._h, float(l1W), float(l2W)))
        self._after_motifs(W)

    def update_feature_maps(self, data=None, W=None, H=None, l1H=0, l2H=0, **kwargs):
        """update_feature_maps!(rule::HALSUpdate, data, W, H; l1H=0, l2H=0) -> loss: src/algs/hals.jl:37-42."""
        loss = ctypes.c_double()
        self._sync_args(W, H)
        self._arm_writeback(W, H)
        check(self._lib.cmf_hals_update_feature_maps(self._h, float(l1H), float(l2H), ctypes.byref(loss)))
        self._after_feature_maps(W, H)
        return loss.value

    def fit_native(self, *a, **kw):
        raise NotImplementedError("cmf_fit runs the multiplicative-update rule; drive HALSUpdate with fit()")

    def iterate(self, *a, **kw):
        raise NotImplementedError("cmf_iterate runs the multiplicative-update rule; call update_motifs / update_feature_maps")


HIPHALSUpdate = HALSUpdate


# pgd.jl's loss / penalty / constraint types, as far as the GPU rule supports them
class SquareLoss:
    """D(b, est) = ||b - est||^2 (src/algs/pgd.jl:29-36)."""


class AbsoluteLoss:
    """D(b, est) = ||b - est||_1 with gradient sign(est - b) (src/algs/pgd.jl:41-47)."""


class MaskedLoss:
    """MaskedLoss(loss, mask): gradient and loss of `loss` restricted by an N x T mask (src/algs/pgd.jl:58-70;
    the loss_func of the reference's test/test.jl:45).  `loss` is SquareLoss() or AbsoluteLoss()."""

    def __init__(self, loss, mask):
        if not isinstance(loss, (SquareLoss, AbsoluteLoss)):
            raise NotImplementedError("MaskedLoss on the GPU wraps SquareLoss or AbsoluteLoss")
        self.loss = loss
        self.mask = farr(mask)


class SquarePenalty:
    """R(x) = weight * ||x||_2^2 (src/algs/pgd.jl:73-80)."""

    def __init__(self, weight):
        self.weight = float(weight)


class AbsolutePenalty:
    """R(x) = weight * ||x||_1 (src/algs/pgd.jl:83-89)."""

    def __init__(self, weight):
        self.weight = float(weight)


class NonnegConstraint:
    """x_i >= 0, projected as max(eps(), x) (src/algs/pgd.jl:92-96)."""


class UnitNormConstraint:
    """Every slice along the first dimension (a component k) with norm > 1 is scaled to norm 1 (src/algs/pgd.jl:100-110;
    `constrW=CMF.UnitNormConstraint()` in figures/thesis/exp_reconstruct_synth.jl:69)."""


def _penalty_weights(penalties):
    sq = sum(p.weight for p in penalties if isinstance(p, SquarePenalty))
    ab = sum(p.weight for p in penalties if isinstance(p, AbsolutePenalty))
    if any(not isinstance(p, (SquarePenalty, AbsolutePenalty)) for p in penalties):
        raise NotImplementedError("PGDUpdate on the GPU supports SquarePenalty and AbsolutePenalty")
    return sq, ab


def _nonneg_flag(constr):
    if constr is None:
        return 0
    if isinstance(constr, NonnegConstraint) or constr is NonnegConstraint:
        return 1
    if isinstance(constr, UnitNormConstraint) or constr is UnitNormConstraint:
        return 2
    raise NotImplementedError("PGDUpdate on the GPU supports NonnegConstraint, UnitNormConstraint or no constraint")


class PGDUpdate(MultUpdate):
    """PGDUpdate on MI355X: drop-in for src/algs/pgd.jl:112-202.

    The gradients are the same contractions as the MU numerators (compute_gradW! is the H_shift * X'
    product of mult.jl:31-34, compute_gradH! is tensor_transconv!), taken on the stored residual.
    The rule state (stepW, stepH, cur_loss) lives in the library handle.  ``devices=[...]`` shards T over several
    GPUs like MultUpdate does (one all-reduce of the partial gradW per iteration; the long recordings of
    notebooks/test_mouse.ipynb are fitted with this rule)."""

    def __init__(self, data, W, H, device=None, devices=None, transport=_lib.CMF_COMM_AUTO, **kw):
        super().__init__(data, W, H, device=device, devices=devices, transport=transport, **kw)
        check(self._lib.cmf_pgd_reset(self._h))
        self._mask_key = None

    def _select_loss(self, loss_func):
        """loss_func=SquareLoss() (default), AbsoluteLoss() or MaskedLoss(either, mask): uploads the mask when it changes."""
        base = loss_func.loss if isinstance(loss_func, MaskedLoss) else loss_func
        if base is None or isinstance(base, SquareLoss) or base is SquareLoss:
            kind = 0
        elif isinstance(base, AbsoluteLoss) or base is AbsoluteLoss:
            kind = 1
        else:
            raise NotImplementedError("PGDUpdate on the GPU supports SquareLoss, AbsoluteLoss and MaskedLoss of either")
        if kind != getattr(self, "_loss_kind", 0):
            check(self._lib.cmf_pgd_set_loss(self._h, kind))
            self._loss_kind = kind
        key = id(loss_func) if isinstance(loss_func, MaskedLoss) else None
        if key == self._mask_key:
            return
        if key is None:
            self._upload_mask(None)
        else:
            if loss_func.mask.shape != (self.N, self.T):
                raise ValueError(f"mask must be {self.N} x {self.T} like data, got {loss_func.mask.shape}")
            self._upload_mask(loss_func.mask)
        self._mask_key = key

    def _upload_mask(self, mask):
        check(self._lib.cmf_set_mask(self._h, None if mask is None else ptr(mask)))

    def update_motifs(self, data=None, W=None, H=None, loss_func=None, constrW=NonnegConstraint, penaltiesW=None, **kwargs):
        """update_motifs!(rule::PGDUpdate, ...; loss_func=SquareLoss(), constrW=NonnegConstraint(),
        penaltiesW=[SquarePenalty(1)]): src/algs/pgd.jl:158-177."""
        self._select_loss(loss_func)
        sq, ab = _penalty_weights([SquarePenalty(1)] if penaltiesW is None else penaltiesW)
        self._sync_args(W, H)
        check(self._lib.cmf_pgd_update_motifs(self._h, sq, ab, _nonneg_flag(constrW)))
        self._after_motifs(W)

    def update_feature_maps(self, data=None, W=None, H=None, loss_func=None, constrH=NonnegConstraint, penaltiesH=None, **kwargs):
        """update_feature_maps!(rule::PGDUpdate, ...; constrH=NonnegConstraint(), penaltiesH=[]) -> loss:
        src/algs/pgd.jl:180-202."""
        self._select_loss(loss_func)
        sq, ab = _penalty_weights([] if penaltiesH is None else penaltiesH)
        loss = ctypes.c_double()
        self._sync_args(W, H)
        self._arm_writeback(W, H)
        check(self._lib.cmf_pgd_update_feature_maps(self._h, sq, ab, _nonneg_flag(constrH), ctypes.byref(loss)))
        self._after_feature_maps(W, H)
        return loss.value

    @property
    def steps(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        check(self._lib.cmf_pgd_get_steps(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def fit_native(self, *a, **kw):
        raise NotImplementedError("cmf_fit runs the multiplicative-update rule; drive PGDUpdate with fit()")

    def iterate(self, *a, **kw):
        raise NotImplementedError("cmf_iterate runs the multiplicative-update rule; call update_motifs / update_feature_maps")


HIPPGDUpdate = PGDUpdate


class _Fp64Rule(AbstractCFUpdate):
    """What the fp64 rules share: one single-GPU handle prepared with the data (``_PREPARE``), the caller's arrays written in
    place, the counters of the last call.  ``_NAME`` / ``_RULE`` are the words the messages name the rule by."""

    MAX_T = 65535 * 64  # columns one contraction launch covers (cmf_admm_prepare / cmf_anls_prepare refuse more)

    def __init__(self, data, W, H, device=None, devices=None):
        if devices is not None:
            raise NotImplementedError(f"{self._NAME} runs on one GPU: devices=[...] (T sharding) is not available for the {self._RULE} rule")
        lib = _lib.load()
        self._lib = lib
        self._h = ctypes.c_void_p()
        data = farr(data)
        if data.ndim != 2:
            raise ValueError("data must be a matrix (N x T)")
        W = farr(W)
        if W.ndim != 3:
            raise ValueError("W must be a K x N x L tensor")
        K, N, L = W.shape
        if data.shape[0] != N:
            raise ValueError(f"DimensionMismatch: data has {data.shape[0]} rows, W has N={N}")
        T = data.shape[1]
        farr(H, (K, T))
        if T > self.MAX_T:  # (cmf_create would cut such a recording into a T-sharded group, which these rules cannot run on)
            raise NotImplementedError(f"{self._NAME} runs on one handle of at most {self.MAX_T} columns (T = {T})")
        self.N, self.T, self.K, self.L = N, T, K, L
        self.device = _dev(device)
        check(lib.cmf_create(ctypes.byref(self._h), self.device, N, T, K, L, ptr(data)))
        try:
            check(getattr(lib, self._PREPARE)(self._h, ptr(data)))
        except Exception:
            self.close()
            raise
        self.data_norm = float(np.linalg.norm(data))  # admm.jl:17, anls.jl:12

    @staticmethod
    def _out(a, shape):
        """The caller's array if the library can write it in place, else a Fortran float64 copy (copied back after the call)."""
        if not isinstance(a, np.ndarray) or tuple(a.shape) != tuple(shape):
            raise ValueError(f"expected an array of shape {tuple(shape)}")
        if a.dtype == np.float64 and a.flags.f_contiguous and a.flags.writeable:
            return a
        return np.asfortranarray(a, dtype=np.float64).copy(order="F")

    def counter(self, name):
        v = ctypes.c_int64()
        check(self._lib.cmf_get_counter(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.cmf_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ADMMUpdate(_Fp64Rule):
    """ADMMUpdate on MI355X: drop-in for src/algs/admm.jl, computed in fp64 end to end.

    ``ADMMUpdate(data, W, H)`` mirrors admm.jl:13-21: it uploads ``data`` in fp64 and keeps its norm (cmf_admm_prepare).  Unlike
    the other rules nothing of W or H stays on the device between calls: each call reads exactly the factor the reference reads
    (``update_motifs`` reads H, ``update_feature_maps`` reads W) from the caller's array and overwrites the other one in place,
    as the reference does.  The inner ADMM loops restart from zero on every call (admm.jl:36-48, :152-163).

    After a call, ``last_W_iters`` / ``last_H_iters`` hold its inner iteration count and ``last_W_reverts`` /
    ``last_H_reverts`` its reverts (cmf_get_counter "admm_W_reverts" / "admm_H_reverts").  One GPU only.
    """

    last_W_iters = last_H_iters = last_W_reverts = last_H_reverts = 0
    _NAME, _RULE, _PREPARE = "ADMMUpdate", "ADMM", "cmf_admm_prepare"

    def update_motifs(self, data, W, H, rhow=10, admm_W_maxiter=30, admm_tol=1e-4, nonnegW=True, **kwargs):
        """update_motifs!(rule::ADMMUpdate, data, W, H; rhow=10, admm_W_maxiter=30, admm_tol=1e-4, nonnegW=true): admm.jl:24-121.
        Reads H, overwrites W."""
        Hin = farr(H, (self.K, self.T))
        Wout = self._out(W, (self.K, self.N, self.L))
        iters = ctypes.c_int64()
        check(self._lib.cmf_admm_update_motifs(self._h, ptr(Hin), ptr(Wout), float(rhow), int(admm_W_maxiter), float(admm_tol),
                                               1 if nonnegW else 0, ctypes.byref(iters)))
        if Wout is not W:
            W[...] = Wout
        self.last_W_iters, self.last_W_reverts = iters.value, self.counter("admm_W_reverts")

    def update_feature_maps(self, data, W, H, rhoh=10, admm_H_maxiter=30, l1H=0, admm_tol=1e-4, nonnegH=True, **kwargs):
        """update_feature_maps!(rule::ADMMUpdate, data, W, H; rhoh=10, admm_H_maxiter=30, l1H=0, admm_tol=1e-4, nonnegH=true)
        -> loss: admm.jl:124-226.  Reads W, overwrites H."""
        Win = farr(W, (self.K, self.N, self.L))
        Hout = self._out(H, (self.K, self.T))
        loss, iters = ctypes.c_double(), ctypes.c_int64()
        check(self._lib.cmf_admm_update_feature_maps(self._h, ptr(Win), ptr(Hout), float(rhoh), int(admm_H_maxiter), float(l1H),
                                                     float(admm_tol), 1 if nonnegH else 0, ctypes.byref(loss), ctypes.byref(iters)))
        if Hout is not H:
            H[...] = Hout
        self.last_H_iters, self.last_H_reverts = iters.value, self.counter("admm_H_reverts")
        return loss.value

    def set_option(self, name, value):
        raise NotImplementedError(f"ADMMUpdate has no library options (got {name!r}): cmf_set_option selects paths of the other rules")


HIPADMMUpdate = ADMMUpdate


class ANLSUpdate(_Fp64Rule):
    """ANLSUpdate on MI355X: drop-in for src/algs/anls.jl (alternating non-negative least squares), computed in fp64 end to end.

    ``ANLSUpdate(data, W, H)`` mirrors anls.jl:10-14: it uploads ``data`` in fp64 and keeps its norm (cmf_anls_prepare).  Nothing
    of W or H stays on the device between calls: ``update_motifs`` reads H from the caller's array and overwrites W with the exact
    minimiser over W >= 0; ``update_feature_maps`` reads W and H and overwrites H column by column (``variant=":basic"``) or in L
    phases of independent columns (``variant=":block"``), as the reference does.  Select it by type (``alg=ANLSUpdate``, what
    HEAD's fit_cnmf takes, model.jl:60); the name ``":anls"`` is not mapped.

    After a call, ``last_W_exchanges`` / ``last_H_exchanges`` hold the pivoting rounds of the NNLS solver summed over the call's
    problems (cmf_get_counter "anls_W_exchanges" / "anls_H_exchanges").  One GPU only; K <= 64, and K*L <= 128 unless
    ``set_option("nnls_large", 1)`` (or ``fit_cnmf(..., options={"nnls_large": 1})``) lets ``update_motifs`` solve up to
    K*L = 1024 unknowns per unit through device scratch (129 and more are refused without it; up to 128 nothing changes).
    """

    last_W_exchanges = last_H_exchanges = 0
    _NAME, _RULE, _PREPARE = "ANLSUpdate", "ANLS", "cmf_anls_prepare"
    _VARIANTS = {"basic": 0, "block": 1}

    @classmethod
    def _variant(cls, variant):
        name = variant.lstrip(":") if isinstance(variant, str) else variant
        if name not in cls._VARIANTS:
            raise ValueError(f"variant must be ':basic' or ':block', got {variant!r}")
        return cls._VARIANTS[name]

    def update_motifs(self, data, W, H, variant=":basic", **kwargs):
        """update_motifs!(rule::ANLSUpdate, data, W, H; kwargs...): anls.jl:22-24, :47-57.  Reads H, overwrites W.  (`variant`
        belongs to update_feature_maps; fit hands every keyword to both calls.)"""
        Hin = farr(H, (self.K, self.T))
        Wout = self._out(W, (self.K, self.N, self.L))
        try:
            check(self._lib.cmf_anls_update_motifs(self._h, ptr(Hin), ptr(Wout)))
        finally:
            self.last_W_exchanges = self.counter("anls_W_exchanges")
        if Wout is not W:
            W[...] = Wout

    def update_feature_maps(self, data, W, H, variant=":basic", **kwargs):
        """update_feature_maps!(rule::ANLSUpdate, data, W, H; variant=:basic) -> loss: anls.jl:26-36, :63-137.  Reads W and H,
        overwrites H."""
        code = self._variant(variant)
        Win = farr(W, (self.K, self.N, self.L))
        Hout = self._out(H, (self.K, self.T))
        loss = ctypes.c_double()
        try:
            check(self._lib.cmf_anls_update_feature_maps(self._h, ptr(Win), ptr(Hout), code, ctypes.byref(loss)))
        finally:
            self.last_H_exchanges = self.counter("anls_H_exchanges")
        if Hout is not H:
            H[...] = Hout
        return loss.value

    def set_option(self, name, value):
        if name not in ("anls_backup_only", "nnls_large"):
            raise NotImplementedError(f"ANLSUpdate has the library options 'anls_backup_only' and 'nnls_large' (got {name!r}): the "
                                      "other names of cmf_set_option select paths of the other rules")
        check(self._lib.cmf_set_option(self._h, name.encode(), int(value)))


HIPANLSUpdate = ANLSUpdate


# --------------------------------------------------------------------------------------
# the separable fit (src/algs/separable.jl)
# --------------------------------------------------------------------------------------
_SQRT_EPS = EPSILON ** 0.5


def _diagscale(c):
    """The diagonal of diagscale (separable.jl:389-391)."""
    return c + (c < EPSILON)


def row_normalize(H):
    """row_normalize(H): separable.jl:422-424."""
    H = np.asarray(H, dtype=np.float64)
    return H * (1.0 / _diagscale(np.abs(H).sum(axis=1)))[:, None]


def cos_score(trueH, estH):
    """cos_score(trueH, estH): separable.jl:432-441."""
    trueH, estH = np.asarray(trueH, dtype=np.float64), np.asarray(estH, dtype=np.float64)
    return float(np.mean([trueH[k] @ estH[k] / (np.linalg.norm(trueH[k]) * np.linalg.norm(estH[k])) for k in range(trueH.shape[0])]))


def permute_factors(trueH, estH):
    """permute_factors(trueH, estH): separable.jl:444-449 -- the permutation p that maximises cos_score(estH[p], trueH)."""
    import itertools

    estH = np.asarray(estH)
    perms = list(itertools.permutations(range(np.asarray(trueH).shape[0])))
    return list(perms[int(np.argmax([cos_score(estH[list(p)], trueH) for p in perms]))])


def is_separable(H, L):
    """is_separable(H, L): separable.jl:452-483 -- does the block form of H contain a scaled permuted identity?"""
    H = np.asarray(H)
    K, T = H.shape
    G = np.zeros((K * L, T))
    for l in range(L):
        G[l * K:(l + 1) * K, l:] = H[:, :T - l]
    nz = G != 0
    return bool(nz[:, nz.sum(axis=0) == 1].any(axis=1).all())


def gen_sep_data(N, T, K, L, H_sparsity=0.75, seed=None, device=None):
    """gen_sep_data(N, T, K, L; H_sparsity=0.75) -> (data, W, H): datasets/sep.jl:4-39, on the K x N x L layout, drawn from
    ``numpy.random.default_rng(seed)``; data = tensor_conv(W, H) on the GPU."""
    rng = np.random.default_rng(seed)
    if T < 3 * K * L:
        raise ValueError("T too small")  # sep.jl:13-16
    W = 0.5 + rng.random((K, N, L))
    H = rng.random((K, T)) * (rng.random((K, T)) > H_sparsity)
    hL = L // 2
    free = np.ones(T - L, dtype=bool)
    for k in range(K):
        for down, up in ((-L, hL), (-hL, L)):  # left and right side of the sequence (sep.jl:23)
            t = int(rng.choice(np.flatnonzero(free)))
            t1, t2 = max(0, t + down), min(T - 1, t + up)
            H[:, t1:t2 + 1] = 0.0
            H[k, t] = 0.5 + rng.random()
            free[t1:min(t2, T - L - 1) + 1] = False
    W, H = np.asfortranarray(W), np.asfortranarray(H)
    return tensor_conv(W, H, device=device), W, H


def _cos_ab(P, head, a, b):
    """cosL(G[a], G[b], l, "a") and (..., "b") for l = 0..L-1 from the shift table (separable.jl:374-385)."""
    return P[a, b, :] / (head[a, :] * head[b, 0]), P[b, a, :] / (head[a, 0] * head[b, :])


def _find_groups(dmat, K, L):
    """find_groups: separable.jl:191-211 (pop! takes the last ungrouped row, findmax the first maximum)."""
    groups = [[] for _ in range(K)]
    ungrouped = list(range(K * L))
    for k in range(K):
        groups[k].append(ungrouped.pop())
        while len(groups[k]) < L:
            sims = dmat[np.ix_(groups[k], ungrouped)].sum(axis=0)
            groups[k].append(ungrouped.pop(int(np.argmax(sims))))
    return groups


def _find_groups_spectral(simat, K, L):
    """find_groups_spectral: separable.jl:214-270 with binarize=false."""
    R = K * L
    simat = np.maximum(0.0, simat - simat.sum() / R ** 2)
    _, V = np.linalg.eigh(simat)
    free = np.ones(R, dtype=bool)
    groups = []
    for k in range(K):
        v = V[:, R - 1 - k]
        if abs(v.max()) < abs(v.min()):
            v = -v  # reorient (:242-244)
        rows = np.flatnonzero(free)
        priority = rows[np.argsort(-v[rows], kind="stable")]
        groups.append([int(r) for r in priority[:L]])
        free[priority[:L]] = False
    return groups


def _arg_shift_max(left, right):
    """arg_shift_max: separable.jl:112-131 (strict >, "a" before "b")."""
    arg, best = 0, 0.0
    for l in range(len(left)):
        if left[l] > best:
            best, arg = left[l], l
        if right[l] > best:
            best, arg = right[l], -l
    return arg


def _sort_group(group, P, head):
    """sort_group: separable.jl:96-109, the cosines from the shift table; a stable sort by descending weight."""
    weight = [sum(_arg_shift_max(*_cos_ab(P, head, a, b)) for b in group) for a in group]
    return [group[i] for i in np.argsort(-np.asarray(weight, dtype=np.float64), kind="stable")]


class Separable(_Fp64Rule):
    """The stages of the separable fit (src/algs/separable.jl) on one MI355X, in fp64: ``Separable(data, K, L)`` uploads the data
    (cmf_sep_prepare); ``spa``, ``nnls``, ``shift_table`` and ``construct`` are the four device stages (cmf_sep_*), ``cluster``
    the decisions on R x R numbers between them (numpy).  ``separable_fit`` runs them in the reference's order."""

    _NAME, _RULE, _PREPARE = "Separable", "separable", "cmf_sep_prepare"
    _PRE = {None: 0, "svd": 1, "svdcond": 2}

    def __init__(self, data, K, L, device=None):
        data = farr(data)
        if data.ndim != 2:
            raise ValueError("data must be a matrix (N x T)")
        N, T = data.shape
        super().__init__(data, np.zeros((K, N, L), order="F"), np.zeros((K, T), order="F"), device=device)
        self.R = K * L

    @classmethod
    def _pre(cls, pre):
        name = pre.lstrip(":") if isinstance(pre, str) else pre
        if name not in cls._PRE:
            raise ValueError(f"pre must be None, ':svd' or ':svdcond', got {pre!r}")
        return name

    def set_option(self, name, value):
        if name != "nnls_large":
            raise NotImplementedError(f"Separable has one library option, 'nnls_large' (got {name!r}): the other names of "
                                      "cmf_set_option select paths of the other rules")
        check(self._lib.cmf_set_option(self._h, name.encode(), int(value)))

    def projection(self, R, thresh, pre):
        """The R x N matrix that pre_svd / pre_svdcond (separable.jl:323-333) multiply X by, from the eigen-decomposition of
        X X' (cmf_sep_gram): U' for :svd (= Diagonal(S) * Vt), S^-1 U' for :svdcond (= Vt).  SPA is invariant under the sign of a
        singular vector (a row of the projected matrix changes sign; norms, inner products and the projector do not); the sign
        is fixed -- the entry of largest magnitude positive -- only so that two runs give the same matrix."""
        XXt = np.zeros((self.N, self.N), order="F")
        check(self._lib.cmf_sep_gram(self._h, float(thresh), ptr(XXt)))
        lam, U = np.linalg.eigh(XXt)
        lam, U = lam[::-1][:R], U[:, ::-1][:, :R]
        sgn = np.sign(U[np.abs(U).argmax(axis=0), np.arange(R)])
        U = U * np.where(sgn == 0, 1.0, sgn)[None, :]
        if pre == "svd":
            return np.ascontiguousarray(U.T)
        if not (lam > 0).all():
            raise ValueError("pre=:svdcond needs R positive singular values")
        return np.ascontiguousarray(U.T / np.sqrt(lam)[:, None])

    def spa(self, R=None, thresh=0, pre=None):
        """SPA(data, R; thresh, pre) -> sorted vertices (0-based): separable.jl:280-319."""
        R = self.R if R is None else int(R)
        pre = self._pre(pre)
        if not 1 <= R <= min(self.N, self.T):
            raise ValueError(f"SPA needs 1 <= R <= min(N, T) (R = {R}, N = {self.N}, T = {self.T})")
        proj = None if pre is None else self.projection(R, thresh, pre)
        vertices = np.zeros(R, dtype=np.int64)
        check(self._lib.cmf_sep_spa(self._h, R, float(thresh), self._PRE[pre], None if proj is None else ptr(proj),
                                    vertices.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return [int(v) for v in vertices]

    def nnls(self, vertices):
        """V = data[:, vertices]; G = nonneg_lsq(V, data); renormalize!(V, G) -> (V, G): separable.jl:23-27."""
        v = np.ascontiguousarray(vertices, dtype=np.int64)
        V = np.zeros((self.N, len(v)), order="F")
        G = np.zeros((len(v), self.T), order="F")
        try:
            check(self._lib.cmf_sep_nnls(self._h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(v), ptr(V), ptr(G)))
        finally:
            self.last_nnls_exchanges = self.counter("sep_nnls_exchanges")
        return V, G

    def shift_table(self, G, L=None):
        """(P, head) with P[a, b, l] = sum_t G[a, t] G[b, t+l] and head[a, l] = |G[a, :T-l]|: what shift_cos / cosL
        (separable.jl:364-385) are made of."""
        L = self.L if L is None else int(L)
        G = farr(G)
        R = G.shape[0]
        if G.shape != (R, self.T):
            raise ValueError(f"expected G of shape (R, {self.T}), got {G.shape}")
        P = np.zeros((R, R, L), order="F")
        head = np.zeros((R, L), order="F")
        check(self._lib.cmf_sep_shift_table(self._h, ptr(G), R, L, ptr(P), ptr(head)))
        return P, head

    def cluster(self, P, head, spectral=False):
        """shift_cluster and sort_group (separable.jl:140-172, :96-109) from the shift table -> K sorted groups of L rows."""
        R = P.shape[0]
        dmat = np.zeros((R, R))
        for r in range(R):  # :144-150, shift_cos (:364-370)
            for p in range(r, R):
                left, right = _cos_ab(P, head, r, p)
                dmat[r, p] = dmat[p, r] = max(0.0, left.max(), right.max())
        groups = (_find_groups_spectral if spectral else _find_groups)(dmat, self.K, self.L)
        return [_sort_group(g, P, head) for g in groups]

    def construct(self, V, G, groups):
        """construct_WH(V, G, groups): separable.jl:59-87 -> (W, H)."""
        g = np.asfortranarray(np.asarray(groups, dtype=np.int64).reshape(self.K, self.L))
        W = np.zeros((self.K, self.N, self.L), order="F")
        H = np.zeros((self.K, self.T), order="F")
        check(self._lib.cmf_sep_construct(self._h, ptr(farr(V, (self.N, self.R))), ptr(farr(G, (self.R, self.T))),
                                          g.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ptr(W), ptr(H)))
        return W, H


def separable_fit(data, K, L, thresh=0, verbose=False, refit_H=False, refit_W=False, refit_H_itr=10, spectral=False, pre=None,
                  device=None, stages=None, nnls_large=False, **kwargs):
    """Separable.fit(data, K, L; thresh=0, verbose=false, refit_H=false, refit_W=false, refit_H_itr=10, spectral=false,
    pre=nothing) -> (W, H): separable.jl:14-56.  ``verbose`` is accepted and plots nothing.  ``refit_W`` is
    ANLSUpdate.update_motifs (fp64), ``refit_H`` is ``refit_H_itr`` H sweeps of the HALS rule with l1H = l2H = 0 (fp32, like
    that rule).  ``stages`` (a dict) receives vertices, V, G, P, head and groups.  One GPU; K*L <= 128, or K*L <= 1024 with
    ``nnls_large=True`` (the option "nnls_large" on the NNLS step and on the ANLSUpdate of ``refit_W``)."""
    data = farr(data)
    rule = Separable(data, K, L, device=device)
    try:
        if nnls_large:
            rule.set_option("nnls_large", 1)
        vertices = rule.spa(thresh=thresh, pre=pre)  # step 1 (:22-23)
        V, G = rule.nnls(vertices)  # step 2 (:26-27)
        P, head = rule.shift_table(G)
        groups = rule.cluster(P, head, spectral=spectral)  # steps 3 and 4 (:30-35)
        W, H = rule.construct(V, G, groups)  # :38
    finally:
        rule.close()
    if stages is not None:
        stages.update(vertices=vertices, V=V, G=G, P=P, head=head, groups=groups)
    if refit_W:  # :41-43
        anls = ANLSUpdate(data, W, H, device=device)
        try:
            if nnls_large:
                anls.set_option("nnls_large", 1)
            anls.update_motifs(data, W, H)
        finally:
            anls.close()
    if refit_H:  # :46-52
        hals = HALSUpdate(data, W, H, device=device)
        try:
            for _ in range(int(refit_H_itr)):
                hals.update_feature_maps()
            hals.download(None, H)
        finally:
            hals.close()
    return W, H


def _resolve_alg(alg):
    """alg may be a rule type (HEAD, model.jl:60) or a README-style symbol (README.md:30-33)."""
    if isinstance(alg, str):
        name = alg.lstrip(":").lower()
        if name in ("mult", "mu"):
            return MultUpdate
        if name == "hals":
            return HALSUpdate
        if name == "pgd":
            return PGDUpdate
        if name == "admm":
            return ADMMUpdate
        if name == "anls":
            raise NotImplementedError("alg=:anls is not mapped as a name: select the ANLS rule by type, alg=ANLSUpdate (model.jl:60)")
        if name == "sep":
            return Separable
        raise ValueError(f"unknown algorithm {alg!r}")
    if isinstance(alg, type) and issubclass(alg, AbstractCFUpdate):
        return alg
    raise TypeError(f"alg must be an update-rule type or a name like ':mult', got {alg!r}")


def _is_hals(alg):
    try:
        return _resolve_alg(alg) is HALSUpdate
    except (TypeError, ValueError, NotImplementedError):
        return False


# --------------------------------------------------------------------------------------
# driver (src/algs/alternating.jl)
# --------------------------------------------------------------------------------------
class AlternatingOptimizer:
    """AlternatingOptimizer(update_rule, max_itr, max_time): src/algs/alternating.jl:10-14."""

    def __init__(self, update_rule, max_itr, max_time):
        self.update_rule = update_rule
        self.max_itr = max_itr
        self.max_time = max_time


def fit(alg, data, L, K, W_init, H_init, verbose=False, **kwargs):
    """fit(alg::AlternatingOptimizer, data, L, K, W_init, H_init; kwargs...): alternating.jl:16-71."""
    # Load keyword args (:23-31)
    check_convergence = kwargs.get("check_convergence", True)
    patience = kwargs.get("patience", 3)
    eval_mode = kwargs.get("eval_mode", False)
    assert patience >= 1
    tol = kwargs.get("tol", 1e-4)

    W = np.array(W_init, dtype=np.float64, order="F", copy=True)  # :33-34 deepcopy
    H = np.array(H_init, dtype=np.float64, order="F", copy=True)
    rule = alg.update_rule
    device_resident = hasattr(rule, "download")

    # Set up optimization tracking (:37-38)
    loss_hist = [rule.compute_loss() if device_resident else compute_loss(data, W, H)]
    time_hist = [0.0]

    if verbose:
        print("Starting ", end="", flush=True)

    itr = 1
    while itr <= alg.max_itr and time_hist[-1] <= alg.max_time:  # :45
        itr += 1
        t0 = time.time()
        if not eval_mode:  # Skip motif update in evaluation mode (:51-53)
            rule.update_motifs(data, W, H, **kwargs)
        loss = rule.update_feature_maps(data, W, H, **kwargs)  # :54 (synchronises)
        dur = time.time() - t0
        if hasattr(rule, "agree_scalar"):
            dur = rule.agree_scalar(dur)  # sharded rule: all ranks follow rank 0's clock, so they stop together
        time_hist.append(time_hist[-1] + dur)  # :57-59
        loss_hist.append(loss)
        if verbose:
            print(".", end="", flush=True)
        if check_convergence and converged(loss_hist, patience, tol):  # :63-66
            print("Converged early.")
            break
    if verbose:
        print(" fit!")

    if device_resident:
        rule.download(W, H)
    return CNMF_results(data, W, H, np.asarray(time_hist), np.asarray(loss_hist))  # :70


# --------------------------------------------------------------------------------------
# public API (src/model.jl)
# --------------------------------------------------------------------------------------
_REG_ALIASES = {"l1_W": "l1W", "l2_W": "l2W", "l1_H": "l1H", "l2_H": "l2H"}  # README.md:44-52 -> mult.jl:23,42
_KNOWN_KW = {"seed", "W_init", "H_init", "check_convergence", "patience", "eval_mode", "tol", "verbose",
             "l1W", "l2W", "l1H", "l2H", "device", "devices", "options",
             "loss_func", "constrW", "constrH", "penaltiesW", "penaltiesH",  # PGDUpdate (pgd.jl:158-202)
             "rhow", "rhoh", "admm_W_maxiter", "admm_H_maxiter", "admm_tol", "nonnegW", "nonnegH",  # ADMMUpdate (admm.jl:24-27,124-127)
             "variant",  # ANLSUpdate (anls.jl:26)
             "thresh", "refit_H", "refit_W", "refit_H_itr", "spectral", "pre",  # alg=:sep (separable.jl:14-18)
             "nnls_large",  # alg=:sep: separable_fit's switch for K*L > 128
             "mask",  # alg=:mult: fit under a 0/1 mask (MultUpdate.set_mask)
             "lambda_xortho", "lambda_ortho_H", "lambda_ortho_W",  # alg=:mult: seqNMF's penalties (MultUpdate.set_xortho)
             "shift",  # alg=:mult: seqNMF's re-centring of motifs inside every iteration (MultUpdate.set_recentre)
             "divergence", "beta"}  # alg=:mult: ":square" (default), ":kl", ":itakura_saito" or ":beta" with beta= (MultUpdate.set_divergence)


def init_rand(data, L, K, seed=None, device=None):
    """Initialize randomly, scaling to minimize square error: src/model.jl:113-125.

    Uses the library's portable counter RNG (Julia's MersenneTwister streams are not
    reproducible across Julia versions); ``seed=None`` draws a fresh seed.
    """
    lib = _lib.load()
    data = farr(data)
    N, T = data.shape
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    W = np.zeros((K, N, L), order="F")
    H = np.zeros((K, T), order="F")
    check(lib.cmf_init_rand(_dev(device), N, T, K, L, int(seed) & (2**64 - 1), ptr(data), ptr(W), ptr(H)))
    return W, H


def fit_cnmf(data, L=10, K=5, alg=MultUpdate, max_itr=100, max_time=math.inf, **kwargs):
    """fit_cnmf(data; L=10, K=5, alg=MultUpdate, max_itr=100, max_time=Inf, kwargs...): src/model.jl:58-85.

    Accepts both HEAD's rule types and the README's symbols (``alg=":mult"``), and both
    spellings of the regularisers (``l1_W`` of README.md:44-52 and ``l1W`` of mult.jl:23,42),
    which HEAD silently drops.

    Sparse counts: an :class:`EventData` (or an object with ``.tocoo()``, e.g. a scipy.sparse matrix) as ``data`` with
    ``alg=":mult", divergence=":kl"`` is fitted at its non-zero entries only (:class:`EventKLUpdate`): the same rule as the dense
    ``divergence=":kl"`` fit in O(nnz K L) work per iteration, without an N x T array on the device.  ``eval_mode``,
    ``check_convergence``, ``max_time``, ``W_init`` / ``H_init`` and both spellings of the regularisers apply; any other rule or
    divergence (the default ``":square"`` included), ``mask=``, the cross-orthogonality weights and ``devices=`` raise
    NotImplementedError.  The initial factors come from :func:`init_rand_events`, so a seeded event fit starts elsewhere than the
    seeded dense fit.  Speed (one MI355X, profiles/mu_kl_events.txt): at N=2000, T=50 000, K=32, L=20 the
    event form takes 1.60 ms per iteration at 1 % density against 3.75 ms for the dense KL rule and the two cross at about 2.5 %;
    at N=250, K=5 it is SLOWER than the dense rule at every density measured (0.39 against 0.20 ms at 1 %: five components use five of
    the 32 lanes of a padded row) -- there the memory footprint is the only reason to use it.
    """
    kw = {}
    for k, v in kwargs.items():
        k2 = _REG_ALIASES.get(k, k)
        if k2 in kw:
            raise TypeError(f"regulariser given twice: {k} and {k2}")
        kw[k2] = v
    unknown = set(kw) - _KNOWN_KW
    if unknown:
        warnings.warn(f"fit_cnmf: ignoring unknown keyword arguments {sorted(unknown)} "
                      "(the reference ignores them silently)", stacklevel=2)
    device = kw.pop("device", None)
    devices = kw.pop("devices", None)  # several GPUs of this node: the T-sharded group form of the :mult rule
    options = kw.pop("options", None)  # {name: value} for cmf_set_option on the rule (include/cmf_hip.h lists them)
    rule_type = _resolve_alg(alg)
    events = _as_events(data)
    shift = bool(kw.pop("shift", False))
    if shift:  # seqNMF's re-centring of motifs: a step of the single-GPU MU rule on dense data (include/cmf_hip.h: cmf_mu_set_recentre)
        if events is not None:
            raise NotImplementedError("shift=True is not available for event data: the event-list rule keeps no dense H to move (the re-centring "
                                      "step runs on the dense MU rule)")
        if rule_type is not MultUpdate:
            raise NotImplementedError("shift=True is implemented for alg=:mult: the re-centring step sits between the H update and the loss conv "
                                      "of the MU iteration; recentre(W, H) moves the result of any other rule")
        if devices is not None:
            raise NotImplementedError("shift=True is not available with devices=[...]: a shift of H crosses the borders of the shards")
        if (options or {}).get("gram", 0):
            raise NotImplementedError("shift=True is not available with the Gram form: its tables of W span the H phase")
    if events is not None:  # sparse counts as an event list: the KL form of the MU rule at the events (EventKLUpdate)
        return _fit_cnmf_events(events, L, K, rule_type, max_itr, max_time, kw, device, devices, options)
    data = farr(data)
    mask = kw.get("mask", None)
    if mask is not None:
        if rule_type is PGDUpdate:
            raise ValueError("alg=:pgd takes its mask through the loss: loss_func=MaskedLoss(SquareLoss(), mask) (pgd.jl:58-70)")
        # (HALS under a mask: the imputed form behind the library option "hals_mask", include/cmf_hip.h)
        if rule_type is not MultUpdate and not (rule_type is HALSUpdate and (options or {}).get("hals_mask", 0)):
            raise NotImplementedError("mask= is implemented for alg=:mult (and, as loss_func=MaskedLoss(...), for :pgd); the HALS, ADMM, "
                                      "ANLS and separable fits have no masked form unless options={'hals_mask': 1} (alg=:hals: HALS on "
                                      "the data with its held-out entries imputed by the current estimate)")
        if devices is not None:
            raise NotImplementedError("mask= is not available with devices=[...]: the masked MU rule runs on one GPU")
        mask = kw["mask"] = farr(mask, data.shape)  # (one object from here on: the rule methods compare by identity)
        if not np.isin(mask, (0.0, 1.0)).all():
            raise ValueError("mask must hold 0 and 1 only (1 = observed)")
    divergence = _divergence_kind(kw.get("divergence", ":square"))
    beta = _check_beta(divergence, kw.get("beta", None))
    if divergence:  # what the divergence forms of the MU rule do not go with (the library refuses the same: csrc/cmf_mu_install.h)
        name, (label, mask_option, yet) = _DIV_NAMES[divergence], _DIV_FIT[divergence]
        if rule_type is not MultUpdate:
            raise NotImplementedError(f"divergence='{name}' is implemented for alg=:mult; the HALS, PGD, ADMM, ANLS and separable "
                                      "fits minimise the squared error (PGD also the absolute error)")
        if mask is not None and not (options or {}).get(mask_option, 0):
            raise NotImplementedError(f"divergence='{name}' is not available with mask=: the {label} form of the MU rule "
                                      f"has no masked form{yet} unless the library option is set: options={{'{mask_option}': 1}}")
        if devices is not None:
            raise NotImplementedError(f"divergence='{name}' is not available with devices=[...]: the {label} form of the "
                                      "MU rule runs on one GPU")
    xortho = _check_xortho(*[kw.get(k, 0.0) for k in _XORTHO_KW])
    if any(xortho):
        if rule_type is not MultUpdate:
            raise NotImplementedError("lambda_xortho / lambda_ortho_H / lambda_ortho_W are implemented for alg=:mult; the HALS, PGD, ADMM, "
                                      "ANLS and separable fits have no cross-orthogonality penalties")
        if mask is not None or divergence or devices is not None or (options or {}).get("gram", 0):
            raise NotImplementedError("the cross-orthogonality penalties run on the squared-error MU rule on one GPU: not with mask=, "
                                      "divergence=, devices=[...] or the Gram form")
    if rule_type is Separable:
        # The separable fit has no iteration and HEAD has no mapping for it (model.jl:3-8 is commented out): the result holds
        # the loss of the fit and the wall time it took; max_itr, max_time, W_init and H_init do not apply.
        if devices is not None:
            raise NotImplementedError("devices=[...] (T sharding) is not available for alg=:sep: the separable fit runs on one GPU")
        sep_kw = {k: kw[k] for k in ("thresh", "verbose", "refit_H", "refit_W", "refit_H_itr", "spectral", "pre", "nnls_large") if k in kw}
        t0 = time.time()
        W, H = separable_fit(data, K, L, device=device, **sep_kw)
        dur = time.time() - t0
        return CNMF_results(data, W, H, np.asarray([dur]), np.asarray([compute_loss(data, W, H, device=device)]))

    seed = kw.get("seed", None)  # :64-67
    # Initialize (:70) -- always runs, like the reference (it consumes the RNG even when inits are given)
    # (under a mask from Xm = select(mask, data, 0): the held-out entries may hold anything)
    W_init, H_init = init_rand(data if mask is None else np.where(mask != 0, data, 0.0), L, K, seed=seed, device=device)
    W_init = kw.get("W_init", W_init)  # :72-73
    H_init = kw.get("H_init", H_init)

    if devices is not None and rule_type is ADMMUpdate:
        raise NotImplementedError("devices=[...] (T sharding) is not available for alg=:admm: the ADMM rule runs on one GPU")
    if devices is not None and rule_type is ANLSUpdate:
        raise NotImplementedError("devices=[...] (T sharding) is not available for alg=ANLSUpdate: the ANLS rule runs on one GPU")
    if devices is not None and rule_type not in (MultUpdate, PGDUpdate):
        raise NotImplementedError("devices=[...] (T sharding) is available for alg=:mult and :pgd; HALS sweeps H sequentially along T")
    if devices is not None:
        rule = rule_type(data, W_init, H_init, devices=devices)
    else:
        rule = (rule_type(data, W_init, H_init, device=device) if issubclass(rule_type, (MultUpdate, _Fp64Rule))
                else rule_type(data, W_init, H_init))
    try:
        for name, value in (options or {}).items():
            rule.set_option(name, value)
        if mask is not None:
            rule.set_mask(mask)  # (before the loop: loss_hist[0] is the masked loss too)
        if divergence:
            rule.set_divergence(_DIV_NAMES[divergence], beta=beta)  # (before the loop: loss_hist[0] is the divergence too)
        if any(xortho):
            rule.set_xortho(*xortho)
        if shift and not kw.get("eval_mode", False):  # (eval mode holds W fixed: nothing is shifted)
            rule.set_recentre(True)
        opt = AlternatingOptimizer(rule, max_itr, max_time)  # :78-82
        loop_kw = {k: v for k, v in kw.items() if k not in ("seed", "W_init", "H_init", "divergence", "beta") + _XORTHO_KW}
        return fit(opt, data, L, K, W_init, H_init, **loop_kw)  # :84
    finally:
        if hasattr(rule, "close"):
            rule.close()


def gen_synthetic(N=100, T=500, K=3, L=20, alpha=0.1, p_h=0.5, sigma=0.2, noise_scale=1.0, seed=1234,
                  return_factors=False, device=None):
    """gen_synthetic(N=, T=) -> data (README.md:14), following synthetic_sequences
    (datasets/synthetic.jl:29-61; same defaults).  ``return_factors=True`` also returns (W, H)."""
    lib = _lib.load()
    data = np.zeros((N, T), order="F")
    W = np.zeros((K, N, L), order="F")
    H = np.zeros((K, T), order="F")
    check(lib.cmf_gen_synthetic(_dev(device), N, T, K, L, float(alpha), float(p_h), float(sigma), float(noise_scale),
                                int(seed) & (2**64 - 1), ptr(data), ptr(W), ptr(H)))
    return (data, W, H) if return_factors else data


# --------------------------------------------------------------------------------------
# callers either side of the path: evaluation, sweeps, results on disk
# --------------------------------------------------------------------------------------
def evaluate_mse(r, device=None):
    """evaluate_mse(r::CNMF_results): src/evaluate.jl:1-5."""
    return compute_loss(r.data, r.W, r.H, device=device)


def evaluate_divergence(r, kind=":kl", device=None, beta=None):
    """The loss of the fitted model ``r`` under ``kind`` (cmf_compute_loss): for ``":kl"`` D(data, est + eps) / sum(data), what
    ``fit_cnmf(divergence=":kl")`` records in ``loss_hist``; for ``":itakura_saito"`` the mean Itakura-Saito divergence per entry
    (what ``fit_cnmf(divergence=":itakura_saito")`` records); for ``":beta"`` with ``beta=`` the mean beta-divergence per entry;
    for ``":square"`` evaluate_mse's value."""
    beta = _check_beta(_divergence_kind(kind), beta)
    if _as_events(r.data) is not None:  # a fit of an event list: the KL loss at the events
        if _divergence_kind(kind) != _DIV_KL:
            raise NotImplementedError(f"a model fitted to event data is evaluated with kind=':kl' only (got {kind!r})")
        return compute_loss(r.data, r.W, r.H, device=device)
    rule = MultUpdate(r.data, r.W, r.H, device=device)
    try:
        rule.set_divergence(kind, beta=beta)
        return rule.compute_loss()
    finally:
        rule.close()


def evaluate_xortho(r, device=None):
    """(xortho, ortho_H, ortho_W) of the fitted model ``r``: seqNMF's three penalty sums without their weights and without the 1/2
    (MultUpdate.xortho_cost)."""
    rule = MultUpdate(r.data, r.W, r.H, device=device)
    try:
        return rule.xortho_cost()
    finally:
        rule.close()


def recentre(W, H):
    """seqNMF's re-centring of motifs on host arrays, for results of any rule: ``(W', H', shifts)`` with every motif's centre of mass
    moved back to the middle of the L-lag window, ``W'[k, n, l] = W[k, n, l - s_k]`` and ``H'[k, t] = H[k, t + s_k]``, vacated entries
    at the MU clamp floor eps(Float64).  The shifts are the library's (cmf_recentre_shifts); no device is used."""
    lib = _lib.load()
    W = farr(W)
    if W.ndim != 3:
        raise ValueError("W must be a K x N x L tensor")
    K, N, L = W.shape
    H = farr(H)
    if H.ndim != 2 or H.shape[0] != K:
        raise ValueError(f"H must be a {K} x T matrix")
    T = H.shape[1]
    s = np.zeros(K, dtype=np.int32)
    check(lib.cmf_recentre_shifts(ptr(W), K, N, L, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    floor = float(np.finfo(np.float64).eps)
    W2, H2 = np.full(W.shape, floor, order="F"), np.full(H.shape, floor, order="F")
    for k in range(K):
        sk = int(s[k])
        lo, hi = max(sk, 0), min(L + sk, L)  # destination lags l with 0 <= l - s < L
        if hi > lo:
            W2[k, :, lo:hi] = W[k, :, lo - sk:hi - sk]
        lo, hi = max(-sk, 0), min(T - sk, T)  # destination columns t with 0 <= t + s < T
        if hi > lo:
            H2[k, lo:hi] = H[k, lo + sk:hi + sk]
    return W2, H2, s


def null_shifts(seed, draws, K, N, L):
    """The circular shifts of seqNMF's null motifs (cmf_null_shifts): an integer (N, K, len(draws)) array, ``[n, k, j]`` the number
    of lags row (k, n) of the motif is rotated by in draw ``draws[j]``.  Draw 0 is the identity; every other entry is a pure
    function of (seed, draw, k, n) in [0, L).  ``draws``: an int (draws 0 .. draws - 1) or a sequence of draw numbers.  No device."""
    lib = _lib.load()
    ds = np.arange(int(draws), dtype=np.int64) if np.isscalar(draws) else np.asarray(list(draws), dtype=np.int64)
    out = np.zeros((int(N), int(K), len(ds)), dtype=np.int32, order="F")
    p32 = ctypes.POINTER(ctypes.c_int32)
    consecutive = len(ds) > 0 and bool(np.all(np.diff(ds) == 1))
    if consecutive:
        check(lib.cmf_null_shifts(int(seed) & (2**64 - 1), int(ds[0]), len(ds), int(K), int(N), int(L), out.ctypes.data_as(p32)))
        return out
    for j, d in enumerate(ds):
        one = np.zeros((int(N), int(K), 1), dtype=np.int32, order="F")
        check(lib.cmf_null_shifts(int(seed) & (2**64 - 1), int(d), 1, int(K), int(N), int(L), one.ctypes.data_as(p32)))
        out[:, :, j] = one[:, :, 0]
    return out


class SignificanceResult:
    """What ``evaluate_significance`` returns: ``pvals`` (K; inf for an excluded component), ``is_significant`` (K booleans),
    ``skew`` (K: the skewness of each component's own overlap), ``skewnull`` (K x nnull) and ``excluded`` (K booleans)."""

    def __init__(self, pvals, is_significant, skew, skewnull, excluded, p, nnull):
        self.pvals, self.is_significant, self.skew, self.skewnull, self.excluded = pvals, is_significant, skew, skewnull, excluded
        self.p, self.nnull = p, nnull

    def __repr__(self):
        return f"SignificanceResult(pvals={self.pvals!r}, is_significant={self.is_significant!r})"


def _skew_from_sums(sums, T):
    """MATLAB's biased skewness(., 1, 2) from the raw power sums (S1, S2, S3) along axis 0 over T samples; m2 <= 0 gives NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = sums[0] / T
        m2 = sums[1] / T - mu * mu
        m3 = sums[2] / T - 3.0 * mu * (sums[1] / T) + 2.0 * mu * mu * mu
        return np.where(m2 > 0.0, m3 / np.where(m2 > 0.0, m2, 1.0) ** 1.5, np.nan), m2


def significance_from_sums(W, sums, T, p=0.05):
    """The host half of seqNMF's test: ``sums`` is the (3, K, 1 + nnull) array of ``MultUpdate.null_moments(seed, 0, 1 + nnull)``
    for the K x N x L motifs ``W`` on ``T`` held-out columns.  Excluded before counting (pval = inf): components whose every entry
    is at or below the MU floor eps(Float64); components with one unit carrying the motif (max_n Wflat^2 > 0.999 sum_n Wflat^2);
    and -- a deviation from seqNMF, where MATLAB's NaN would count as significant -- components whose own overlap has no variance.
    pval = (1 + #{null skewness > own}) / nnull (a NaN null compares false); significant where pval <= p / K_kept."""
    W = np.asarray(W, dtype=np.float64)
    K = W.shape[0]
    nnull = sums.shape[2] - 1
    if nnull < 1:
        raise ValueError("at least one null draw is needed")
    sk, m2 = _skew_from_sums(np.asarray(sums, dtype=np.float64), float(T))
    skew, skewnull = sk[:, 0].copy(), sk[:, 1:].copy()
    wflat2 = W.sum(axis=2) ** 2
    excluded = (W.reshape(K, -1).max(axis=1) <= EPSILON) | (wflat2.max(axis=1) > 0.999 * wflat2.sum(axis=1)) | ~(m2[:, 0] > 0.0)
    kept = int(K - excluded.sum())
    pvals = np.full(K, np.inf)
    counts = (skewnull > skew[:, None]).sum(axis=1)
    pvals[~excluded] = (1.0 + counts[~excluded]) / nnull
    is_sig = np.zeros(K, dtype=bool)
    if kept:
        is_sig[~excluded] = pvals[~excluded] <= p / kept
    return SignificanceResult(pvals, is_sig, skew, skewnull, excluded, p, nnull)


def evaluate_significance(r_or_W, test, p=0.05, nnull=None, seed=0, device=None, options=None):
    """seqNMF's test_significance on held-out data: which of the K motifs of a fitted model (a ``CNMF_results`` or a K x N x L array)
    are sequences?  For each component the skewness of its overlap with ``test`` (N x T'), tensor_transconv(W, test)[k, :], is
    compared with the skewness under ``nnull`` null motifs whose rows are circularly shifted along the lag axis, each
    (component, unit) by a random amount of its own (``null_shifts``); default nnull = 2 ceil(K / p).  Returns a
    ``SignificanceResult``.  The overlap drops terms beyond the last column (common.jl:71-81) where seqNMF's helper wraps around;
    the two agree on ``test`` followed by L zero columns.  ``options``: library options of the handle, e.g. {"signif_batch": 8}."""
    W = farr(r_or_W.W if hasattr(r_or_W, "W") else r_or_W)
    if W.ndim != 3:
        raise ValueError("W must be a K x N x L tensor")
    test = farr(test)
    K = W.shape[0]
    if test.ndim != 2 or test.shape[0] != W.shape[1]:
        raise ValueError(f"test must be N x T' with N={W.shape[1]}, got {test.shape}")
    if not (0.0 < p <= 1.0):
        raise ValueError("p must lie in (0, 1]")
    nnull = 2 * int(math.ceil(K / p)) if nnull is None else int(nnull)
    if nnull < 1:
        raise ValueError("nnull must be at least 1")
    rule = MultUpdate(test, W, np.zeros((K, test.shape[1]), order="F"), device=device)
    try:
        for name, value in (options or {}).items():
            rule.set_option(name, value)
        sums = rule.null_moments(seed, 0, 1 + nnull)
    finally:
        rule.close()
    return significance_from_sums(W, sums, test.shape[1], p=p)


def xortho_sweep(data, lambdas, L, K, **fit_kw):
    """One ``fit_cnmf(data, L=L, K=K, alg=":mult", lambda_xortho=lam, **fit_kw)`` per ``lam`` in ``lambdas``, all from the same
    initial factors (``seed=`` or ``W_init`` / ``H_init`` of ``fit_kw``; without either one seed is drawn for the whole sweep).
    Returns ``{lam: {"loss": final loss, "xortho": cross-orthogonality cost, "res": CNMF_results}}``: the two curves whose
    crossover seqNMF's procedure picks lambda from."""
    if "alg" in fit_kw or "lambda_xortho" in fit_kw:
        raise TypeError("xortho_sweep fits with alg=':mult' and its own lambda_xortho")
    fit_kw = dict(fit_kw)
    if "seed" not in fit_kw and not ("W_init" in fit_kw and "H_init" in fit_kw):
        fit_kw["seed"] = int.from_bytes(os.urandom(4), "little")
    out = {}
    for lam in lambdas:
        r = fit_cnmf(data, L=L, K=K, alg=":mult", lambda_xortho=lam, **fit_kw)
        out[lam] = {"loss": float(r.loss_hist[-1]), "xortho": evaluate_xortho(r, device=fit_kw.get("device", None))[0], "res": r}
    return out


def evaluate_test(r, test, num_iter=30, device=None):
    """evaluate_test(r, test; num_iter=30): src/evaluate.jl:8-25 -- refit H on held-out data with the
    motifs fixed (HALS H sweeps from H = 0, no regularisation), then the normalised loss.  (The
    reference's version calls a `HALS` module that no longer exists at HEAD; this is its intent.)"""
    test = farr(test)
    K = r.W.shape[0]
    rule = HALSUpdate(test, r.W, np.zeros((K, test.shape[1])), device=device)
    try:
        for _ in range(int(num_iter)):
            rule.update_feature_maps()
        return rule.compute_loss()
    finally:
        rule.close()


def holdout_mask(N, T, frac=0.1, block=1, seed=None):
    """An N x T mask of 0 and 1 (1 = observed) that holds out about ``frac`` of the entries in runs of exactly ``block``
    consecutive samples of one unit (a run that reaches T is cut there).  A convolutive model interpolates an isolated entry
    from its neighbours in time, so ``block=L`` is the useful setting for choosing K and L.  Along every unit, runs alternate
    with observed stretches of at least one sample whose lengths are geometric with mean block (1 - frac) / frac, which makes
    the expected held-out share ``frac``.  ``block=1`` is plain speckle: every entry is held out independently with probability
    ``frac`` (single entries may touch).  Deterministic in ``seed`` (numpy's default_rng), pure numpy."""
    N, T, block = int(N), int(T), int(block)
    if not (0.0 <= frac < 1.0):
        raise ValueError("frac must be in [0, 1)")
    if block < 1:
        raise ValueError("block must be >= 1")
    rng = np.random.default_rng(seed)
    if frac == 0.0:
        return np.ones((N, T), order="F")
    if block == 1:
        return np.asfortranarray(np.where(rng.random((N, T)) < frac, 0.0, 1.0))
    p = frac / (block * (1.0 - frac))  # 1 / mean observed stretch
    if p > 1.0:
        raise ValueError(f"frac={frac} cannot be reached with separated runs of block={block}: at most block / (block + 1)")
    ncyc = T // (block + 1) + 2  # a cycle (stretch + run) is at least block + 1 long
    gaps = rng.geometric(p, size=(N, ncyc)).astype(np.int64)
    gaps[:, 0] -= 1  # (a run may start at the first sample)
    starts = np.cumsum(gaps + block, axis=1) - block
    diff = np.zeros((N, T + 1), dtype=np.int32)
    rows = np.broadcast_to(np.arange(N)[:, None], starts.shape)
    live = starts < T
    np.add.at(diff, (rows[live], starts[live]), 1)
    np.add.at(diff, (rows[live], np.minimum(starts[live] + block, T)), -1)
    held = np.cumsum(diff[:, :T], axis=1) > 0
    return np.asfortranarray(np.where(held, 0.0, 1.0))


def evaluate_heldout(r, mask, device=None, divergence=":square", beta=None, options=None):
    """(train, test) = sqrt(sum of (est - data)^2 / sum of data^2) over the entries with ``mask == 1`` and over those with
    ``mask == 0``, for the fitted model ``r`` (cmf_masked_loss: one loss-only conv each, sums by select).
    ``divergence=":kl"``: D / sum(data) over the same two sets of entries, D the sum of the divergence terms there (no square
    root): what ``fit_cnmf(divergence=":kl", mask=...)`` records in ``loss_hist``, and its held-out counterpart.
    ``divergence=":itakura_saito"`` or ``":beta"`` (with ``beta=``) under ``options={"pq_mask": 1}``: the mean divergence per entry
    over the same two sets (sum of the terms / number of entries): what such a fit under the mask records, and its counterpart."""
    kl = _divergence_kind(divergence)
    pq = kl in (_DIV_IS, _DIV_BETA)
    if kl == _DIV_BETA and not (options or {}).get("pq_mask", 0):
        raise NotImplementedError("divergence=':beta' has no held-out score: the beta-divergence form of the MU rule has no masked form "
                                  "unless the library option is set: options={'pq_mask': 1}")
    if kl == _DIV_IS and not (options or {}).get("pq_mask", 0):
        raise NotImplementedError("divergence=':itakura_saito' has no held-out score: the Itakura-Saito form of the MU rule has no "
                                  "masked form unless the library option is set: options={'pq_mask': 1}")
    beta = _check_beta(kl, beta)
    mask = farr(mask, np.shape(r.data))
    rule = MultUpdate(r.data, r.W, r.H, device=device)
    try:
        if pq:
            rule.set_option("pq_mask", 1)
        elif kl:
            rule.set_option("kl_mask", 1)
        rule.set_mask(mask)
        if kl:
            rule.set_divergence(_DIV_NAMES[kl], beta=beta)
        out = []
        for comp in (False, True):
            resid, dat = rule.masked_loss(complement=comp)
            out.append((resid / dat if kl else math.sqrt(resid / dat)) if dat > 0 else math.nan)
        return out[0], out[1]
    finally:
        rule.close()


def _process_group(group):
    """(dist module or None, rank, world) of an initialised torch.distributed process group (parameter_sweep's rule: torch is
    never imported from here)."""
    import sys

    dist = None
    if "torch" in sys.modules:
        import torch.distributed as _dist

        if _dist.is_available() and _dist.is_initialized():
            dist = _dist
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if dist else (0, 1)
    return dist, rank, world


def cross_validate(data, L_vals, K_vals, frac=0.1, block=None, repeats=1, seed=None, group=None, **fit_kw):
    """Held-out scores for choosing L and K: for every (L, K) and every repeat, draw ``holdout_mask(N, T, frac, block, seed')``,
    fit ``fit_cnmf(data, L=L, K=K, alg=":mult", mask=mask, seed=seed', **fit_kw)`` and score it with ``evaluate_heldout``.
    ``divergence=":kl"`` (for counts) fits the KL form under the mask -- the library option "kl_mask" is set here, beside whatever
    ``options=`` holds -- and scores with the same divergence.  ``divergence=":itakura_saito"`` or ``":beta"`` (for power
    spectrograms) proceed when ``options`` carries ``pq_mask=1`` and score by the mean divergence per entry.
    ``alg=":hals"`` with ``options={"hals_mask": 1}`` fits with the HALS rule under the mask (HALS on the data with its held-out
    entries imputed by the current estimate) and scores the same way; any other ``alg`` raises TypeError.
    Returns ``{(L, K): {"train": array(repeats), "test": array(repeats)}}``.  ``block`` defaults to the combination's L.
    seed' = seed + index of the (combination, repeat) pair (fresh draws when ``seed`` is None), so that a result can be redone
    by hand.  Under an initialised torch.distributed process group the pairs are dealt to the ranks like parameter_sweep's
    combinations and the scores gathered on all ranks."""
    pq_mask = bool((fit_kw.get("options") or {}).get("pq_mask", 0))
    if _divergence_kind(fit_kw.get("divergence", ":square")) == _DIV_BETA and not pq_mask:
        raise NotImplementedError("cross_validate(divergence=':beta') is not available: the beta-divergence form of the MU rule "
                                  "has no masked form, so nothing can be held out (unless options={'pq_mask': 1})")
    if _divergence_kind(fit_kw.get("divergence", ":square")) == _DIV_IS and not pq_mask:
        raise NotImplementedError("cross_validate(divergence=':itakura_saito') is not available: the Itakura-Saito form of the MU rule "
                                  "has no masked form, so nothing can be held out (unless options={'pq_mask': 1})")
    data = farr(data)
    N, T = data.shape
    # (the one other rule with a masked form: HALS behind the library option "hals_mask")
    hals = "alg" in fit_kw and (fit_kw.get("options") or {}).get("hals_mask", 0) and _is_hals(fit_kw["alg"])
    if "mask" in fit_kw or ("alg" in fit_kw and not hals):
        raise TypeError("cross_validate draws its own masks and fits with alg=':mult' (or alg=':hals' with options={'hals_mask': 1})")
    alg = fit_kw.pop("alg", ":mult")
    combos = [(L, K) for L in L_vals for K in K_vals]
    jobs = [(c, rep) for c in combos for rep in range(int(repeats))]
    dist, rank, world = _process_group(group)
    device = fit_kw.get("device", None)
    divergence = fit_kw.get("divergence", ":square")
    if _divergence_kind(divergence) == _DIV_KL:
        fit_kw["options"] = dict(fit_kw.get("options") or {}, kl_mask=1)
    mine = {}
    for idx, ((L, K), rep) in enumerate(jobs):
        if idx % world != rank:
            continue
        s = None if seed is None else int(seed) + idx
        mask = holdout_mask(N, T, frac=frac, block=L if block is None else block, seed=s)
        r = fit_cnmf(data, L=L, K=K, alg=alg, mask=mask, seed=s, **fit_kw)
        mine[idx] = evaluate_heldout(r, mask, device=device, divergence=divergence, beta=fit_kw.get("beta", None),
                                     options={"pq_mask": 1} if pq_mask else None)
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, mine, group=group)
        mine = {k: v for part in parts for k, v in part.items()}
    out = {c: {"train": np.zeros(int(repeats)), "test": np.zeros(int(repeats))} for c in combos}
    for idx, (c, rep) in enumerate(jobs):
        out[c]["train"][rep], out[c]["test"][rep] = mine[idx]
    return out


def evaluate_convergence(r, thresh=0.01):
    """evaluate_convergence(r; thresh=0.01): src/evaluate.jl:29-44 -- first iteration whose loss is within
    `thresh` (relative) of the final loss."""
    min_loss = r.loss_hist[-1]
    for i, loss in enumerate(r.loss_hist):
        if loss / min_loss < 1 + thresh:
            return i
    return len(r.loss_hist)


def parameter_sweep(data, L_vals=(7,), K_vals=(3,), alg_vals=(":mult",), max_itr=100, max_time=math.inf, group=None, **kwargs):
    """parameter_sweep(data; L_vals, K_vals, alg_vals, max_itr, max_time): src/model.jl:132-145.
    Returns {(L, K, alg): CNMF_results}; other keywords go to every fit_cnmf call (HEAD passes stale
    `lambda1/initW` names that fit_cnmf ignores; here they would be reported as unknown).

    Multi-GPU: the fits are independent, so when a torch.distributed process group is up
    (one process per GPU) each rank runs every world-th combination on its own device and the results are gathered
    on all ranks -- replicas, no data-path collective.  A `seed` keyword is used as given by every fit."""
    combos = [(L, K, alg) for L in L_vals for K in K_vals for alg in alg_vals]
    dist = None
    import sys

    if "torch" in sys.modules:  # a process group can only be up if torch is already imported: never import it from here
        # (importing torch AFTER libcmf_hip.so maps PyTorch's bundled HIP / HSA runtime next to the system one this
        # library is already bound to, and RCCL then picks the uninitialised copy)
        import torch.distributed as _dist

        if _dist.is_available() and _dist.is_initialized():
            dist = _dist
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if dist else (0, 1)
    mine = {}
    for idx, (L, K, alg) in enumerate(combos):
        if idx % world == rank:
            mine[(L, K, alg)] = fit_cnmf(data, L=L, K=K, alg=alg, max_itr=max_itr, max_time=max_time, **kwargs)
    if world == 1:
        return mine
    # results travel without their copy of `data` (every rank holds it already)
    packed = {k: (r.W, r.H, r.time_hist, r.loss_hist) for k, r in mine.items()}
    parts = [None] * world
    dist.all_gather_object(parts, packed, group=group)
    data_f = np.asarray(data, dtype=np.float64)
    results = {}
    for key in combos:  # the reference's insertion order
        for part in parts:
            if key in part:
                W, H, th, lh = part[key]
                results[key] = CNMF_results(data_f, W, H, th, lh)
    return results


_MODEL_KEYS = ("W", "H", "data", "loss_hist", "time_hist")


_META_KEYS = ("l1_H", "l2_H", "l1_W", "l2_W", "alg", "lambda_xortho", "lambda_ortho_H", "lambda_ortho_W")


def _is_hdf5_path(path):
    return str(path).lower().endswith((".h5", ".hdf5", ".hdf"))


def save_model(results, path, **meta):
    """save_model(results, path): src/model.jl:149-163.  The reference's schema: datasets W, H, data, loss_hist,
    time_hist plus whatever of l1_H, l2_H, l1_W, l2_W, alg is passed as keywords (CNMF_results itself does not carry
    them, which is why the reference's own save_model is broken at HEAD).  A path ending in .h5 / .hdf5 is written as
    a real HDF5 file in HDF5.jl's conventions (cmf.jl_amd/_hdf5.py over the system libhdf5), readable by the
    reference's load_model; any other path is a NumPy .npz container with the same names."""
    if _as_events(results.data) is not None:
        raise NotImplementedError("save_model: results.data is an event list (EventData); persistence of event data is not implemented "
                                  "-- save W, H and the events yourself, or results with data=events.todense()")
    arrays = {k: np.asarray(getattr(results, k)) for k in _MODEL_KEYS}
    if _is_hdf5_path(path):
        from . import _hdf5

        items = dict(arrays)
        for k, v in meta.items():
            items[k] = str(v).lstrip(":") if k == "alg" or isinstance(v, str) else np.asarray(v, dtype=np.float64)
        _hdf5.write_file(path, items)
        return
    for k, v in meta.items():  # (`alg` without the colon of a Julia symbol, in both containers)
        arrays[k] = np.asarray(str(v).lstrip(":") if k == "alg" else v)
    np.savez_compressed(path, **arrays)


def load_model(path):
    """load_model(path): src/model.jl:167-181 -> (CNMF_results, meta dict); .h5 / .hdf5 files as written by either
    side, otherwise the .npz container."""
    if _is_hdf5_path(path):
        from . import _hdf5

        d = _hdf5.read_file(path, _MODEL_KEYS + _META_KEYS)
        missing = [k for k in _MODEL_KEYS if k not in d]
        if missing:
            raise KeyError(f"{path}: datasets {missing} are missing")
        r = CNMF_results(d["data"], d["W"], d["H"], d["time_hist"], d["loss_hist"])
        return r, {k: d[k] for k in _META_KEYS if k in d}
    with np.load(path, allow_pickle=False) as f:
        r = CNMF_results(f["data"], f["W"], f["H"], f["time_hist"], f["loss_hist"])
        meta = {k: f[k][()] for k in f.files if k not in _MODEL_KEYS}
    return r, meta
