"""The walk over the MU rule's forms, gate options and requests that tools/record_mu_transitions.py records and
tests/test_gpu_mu_form_transitions.py repeats (tests/golden/mu_form_transitions.json).

A cell is (data set, start, form, gates, request): a fresh handle is put into `form` with the three gate options set as `gates`
says, the request is made through the C ABI, and the cell's outcome is the return code and the name of the form the handle is in
afterwards -- found by uploading the initial factors again and matching compute_loss() bitwise against the losses of fresh handles
put directly into each form.  Two data sets: "pos" is strictly positive, "holed" is the same with one entry of -1 that the mask
holds out, so it passes the divergences' data checks under that mask only.
"""
import numpy as np

import cmf_jl_amd as cmf
from cmf_jl_amd import _lib

N, T, K, L = 12, 40, 3, 4
GATES = ("kl_mask", "pq_mask", "is_div")
DIV_SQUARE, DIV_KL, DIV_IS, DIV_BETA = 0, 1, 2, 3
# the eight forms the walk starts from: name, divergence kind, beta, masked, the gate options the form cannot be installed without
FORMS = [("square", DIV_SQUARE, None, False, ()), ("square+mask", DIV_SQUARE, None, True, ()),
         ("kl", DIV_KL, None, False, ()), ("kl+mask", DIV_KL, None, True, ("kl_mask",)),
         ("is", DIV_IS, None, False, ("is_div",)), ("is+mask", DIV_IS, None, True, ("is_div", "pq_mask")),
         ("beta(0.5)", DIV_BETA, 0.5, False, ()), ("beta(0.5)+mask", DIV_BETA, 0.5, True, ("pq_mask",))]
# ... and the two more a request can lead to
NAMED = FORMS + [("beta(1.5)", DIV_BETA, 1.5, False, ()), ("beta(1.5)+mask", DIV_BETA, 1.5, True, ("pq_mask",))]
STARTS = ("plain", "gram", "xortho")  # the last two: the plain square form with gram = 1 / active cross-orthogonality weights set first
DATA_SETS = ("pos", "holed")

_PROBLEM = {}


def problem():
    """data ("pos" / "holed"), the initial factors, the mask, a mask that observes the bad entry of "holed", PGD weights."""
    if not _PROBLEM:
        pos = np.maximum(cmf.gen_synthetic(N=N, T=T, K=K, L=L, seed=77), 0.0) + 0.05
        mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=5)
        assert 0.1 < 1.0 - mask.mean() < 0.3
        i, j = [int(v[0]) for v in np.nonzero(mask == 0)]
        holed = pos.copy()
        holed[i, j] = -1.0
        seeing = mask.copy()
        seeing[i, j] = 1.0
        W0, H0 = cmf.init_rand(pos, L=L, K=K, seed=3)
        weights = np.asfortranarray(0.25 + 0.5 * ((np.arange(N)[:, None] + np.arange(T)[None, :]) % 3))
        _PROBLEM.update(pos=np.asfortranarray(pos), holed=np.asfortranarray(holed), W0=W0, H0=H0, mask=np.asfortranarray(mask),
                        seeing=np.asfortranarray(seeing), weights=weights)
    return _PROBLEM


def _opt(rule, name, value):
    return rule._lib.cmf_set_option(rule._h, name.encode(), int(value))


def _mask(rule, m):
    return rule._lib.cmf_mu_set_mask(rule._h, None if m is None else _lib.ptr(m))


def _beta(b):
    return lambda rule, p: rule._lib.cmf_mu_set_beta_divergence(rule._h, float(b))


def _kind(k):
    return lambda rule, p: rule._lib.cmf_mu_set_divergence(rule._h, k)


# every request of the walk: name -> f(rule, problem) -> return code
REQUESTS = {
    "set_mask": lambda rule, p: _mask(rule, p["mask"]),
    "clear_mask": lambda rule, p: _mask(rule, None),
    "kind_square": _kind(DIV_SQUARE), "kind_kl": _kind(DIV_KL), "kind_is": _kind(DIV_IS),
    "beta_0.5": _beta(0.5), "beta_1.5": _beta(1.5), "beta_1.0": _beta(1.0), "beta_0.005": _beta(0.005),
    "gram_1": lambda rule, p: _opt(rule, "gram", 1),
    "kl_mask_0": lambda rule, p: _opt(rule, "kl_mask", 0),
    "pq_mask_0": lambda rule, p: _opt(rule, "pq_mask", 0),
    "is_div_0": lambda rule, p: _opt(rule, "is_div", 0),
    "pgd_set_mask": lambda rule, p: rule._lib.cmf_set_mask(rule._h, _lib.ptr(p["weights"])),
    "hals_update_motifs": lambda rule, p: rule._lib.cmf_hals_update_motifs(rule._h, 0.0, 0.0),
    "pgd_update_motifs": lambda rule, p: rule._lib.cmf_pgd_update_motifs(rule._h, 0.0, 0.0, 1),
    "xortho_1_0_0": lambda rule, p: rule._lib.cmf_mu_set_xortho(rule._h, 1.0, 0.0, 0.0),
}


def gate_settings(required):
    """The gate settings (a string of three 0/1 in the order of GATES) under which a form with these required gates can exist."""
    return [s for s in (format(i, "03b") for i in range(8)) if all(s[GATES.index(g)] == "1" for g in required)]


def reachable(data_set, form):
    """"holed" passes no divergence's data check without its mask."""
    return data_set == "pos" or form[3] or form[1] == DIV_SQUARE


def cells():
    """(data set, start, form name, gates, request) of every cell, in recording order."""
    out = []
    for ds in DATA_SETS:
        for start in STARTS:
            for form in (FORMS if start == "plain" else FORMS[:1]):
                if reachable(ds, form):
                    out += [(ds, start, form[0], g, r) for g in gate_settings(form[4]) for r in REQUESTS]
    return out


def key(cell):
    return "|".join(cell)


def install(data_set, form, gates="111", start="plain", W=None, H=None):
    """A fresh handle in `form`: the gates as asked, then the mask, then the divergence (the order "holed" needs)."""
    p = problem()
    _, kind, beta, masked, required = form
    rule = cmf.MultUpdate(p[data_set], p["W0"] if W is None else W, p["H0"] if H is None else H)
    try:
        for g, v in zip(GATES, gates):
            _lib.check(_opt(rule, g, int(v)))
        if start == "gram":
            _lib.check(_opt(rule, "gram", 1))
        if start == "xortho":
            _lib.check(rule._lib.cmf_mu_set_xortho(rule._h, 1.0, 0.0, 0.0))
        if masked:
            _lib.check(_mask(rule, p["mask"]))
        if kind == DIV_BETA:
            _lib.check(_beta(beta)(rule, p))
        elif kind != DIV_SQUARE:
            _lib.check(_kind(kind)(rule, p))
    except Exception:
        rule.close()
        raise
    return rule


def loss_bits(rule):
    """compute_loss() of the initial factors under whatever form the handle is in, as the bytes of the double."""
    p = problem()
    _lib.check(_opt(rule, "gram", 0))  # (the Gram forms take another path to the same quantity; which form is installed does not depend on it)
    rule.upload(p["W0"], p["H0"])
    return np.float64(rule.compute_loss()).tobytes()


def form_losses(data_set):
    """{loss bytes: form name} of fresh handles put directly into every form `data_set` reaches; the losses are pairwise distinct."""
    table = {}
    for form in NAMED:
        if reachable(data_set, form):
            rule = install(data_set, form)
            try:
                bits = loss_bits(rule)
            finally:
                rule.close()
            assert bits not in table, f"{data_set}: the losses of {table[bits]} and {form[0]} are the same bits"
            table[bits] = form[0]
    return table


def walk_cell(cell, table):
    """(return code, form afterwards) of one cell."""
    ds, start, name, gates, request = cell
    form = next(f for f in FORMS if f[0] == name)
    rule = install(ds, form, gates, start)
    try:
        rc = int(REQUESTS[request](rule, problem()))
        after = table.get(loss_bits(rule), "unknown")
    finally:
        rule.close()
    return rc, after
