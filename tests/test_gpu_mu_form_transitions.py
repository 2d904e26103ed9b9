"""Every form of the MU rule (square, KL, Itakura-Saito, beta; each with and without a mask) is installed, left and refused through one
transition (mu_set_form, csrc/cmf_api.hip; csrc/cmf_mu_install.h).  Three things are held here:

1. the matrix of tests/golden/mu_form_transitions.json (tools/record_mu_transitions.py, recorded through the hand-written installers this
   transition replaced): return code and resulting form of every request in every form under every gate setting, cell for cell;
2. all 56 ordered pairs of forms on one handle: after the switch W, H and the losses are bitwise those of a fresh handle put directly
   into the second form -- nothing of the first form (est, the speculation, a deferred loss, its buffers) leaks into the second;
3. a request whose data check fails leaves the form the handle had, working, for every form: the next iterations are bitwise those of
   an undisturbed handle.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mu_form_walk as walk  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mu_form_transitions.json")


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def test_the_recorded_matrix_cell_for_cell(cmf):
    with open(GOLDEN) as f:
        golden = json.load(f)["cells"]
    tables = {ds: walk.form_losses(ds) for ds in walk.DATA_SETS}  # (asserts that the losses of the forms are pairwise distinct)
    assert len(tables["pos"]) == 10 and len(tables["holed"]) == 6
    cells = walk.cells()
    assert sorted(walk.key(c) for c in cells) == sorted(golden)
    wrong = []
    for cell in cells:
        rc, after = walk.walk_cell(cell, tables[cell[0]])
        if [rc, after] != golden[walk.key(cell)][:2]:
            wrong.append((walk.key(cell), (rc, after), golden[walk.key(cell)][:2]))
    assert not wrong, f"{len(wrong)} of {len(cells)} cells differ from the recorded matrix, first: {wrong[:5]}"


# ---- all ordered pairs of forms on one handle ---------------------------------------------------------------------------------
def put(rule, form, mask, divergence_first):
    """From whatever form the handle is in to `form`, in either order of the two requests (all gates are on)."""
    _, kind, beta, masked, _ = form

    def divergence():
        rule.set_divergence({0: ":square", 1: ":kl", 2: ":itakura_saito", 3: ":beta"}[kind], beta=beta)

    def masking():
        rule.set_mask(mask if masked else None)

    for step in ((divergence, masking) if divergence_first else (masking, divergence)):
        step()


def segment(rule):
    rule.update_motifs()  # at once: an est, a speculated contraction or a carried loss of the form just left would be consumed here
    lh = [rule.update_feature_maps()] + list(rule.iterate(2))
    return rule.download() + (np.asarray(lh),)


@pytest.mark.parametrize("shape", [(48, 300, 4, 8), (40, 200, 32, 5)], ids=["few_components", "k32"])
def test_all_ordered_pairs_of_forms(cmf, shape):
    N, T, K, L = shape
    data = np.maximum(cmf.gen_synthetic(N=N, T=T, K=3, L=L, seed=1234 + N), 0.0) + 0.05
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=T)
    mask = cmf.holdout_mask(N, T, frac=0.2, block=L, seed=K)

    def handle(W, H):
        rule = cmf.MultUpdate(data, W, H)
        for g in walk.GATES:
            rule.set_option(g, 1)
        return rule

    pairs = [(a, b) for a in walk.FORMS for b in walk.FORMS if a is not b]
    assert len(pairs) == 56
    for n, (a, b) in enumerate(pairs):
        rule = handle(W0, H0)
        try:
            put(rule, a, mask, divergence_first=False)
            rule.update_motifs()
            rule.update_feature_maps()
            W, H = rule.download()
            put(rule, b, mask, divergence_first=bool(n % 2))
            got = segment(rule)
        finally:
            rule.close()
        fresh = handle(W, H)
        try:
            put(fresh, b, mask, divergence_first=False)
            want = segment(fresh)
        finally:
            fresh.close()
        for x, y, name in zip(got, want, ("W", "H", "losses")):
            assert np.isfinite(x).all(), (a[0], b[0], name)
            np.testing.assert_array_equal(x, y, err_msg=f"{a[0]} -> {b[0]}: {name}")


# ---- a failed request leaves the form the handle had ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [f for f in walk.FORMS if f[3]], ids=lambda f: f[0])
def test_a_refused_mask_or_unmasking_leaves_the_form_working(cmf, form):
    """On the data set that is valid only under its mask: a mask that observes the bad entry, then (every form but square, whose rule
    takes any data) clearing the mask, are refused with CMF_ERR_ARG by the form's data check; two more iterations are bitwise those
    of a handle nobody disturbed."""
    p = walk.problem()
    rule, calm = walk.install("holed", form), walk.install("holed", form)
    try:
        for r in (rule, calm):
            r.update_motifs()
            r.update_feature_maps()
        refusals = [] if form[1] == walk.DIV_SQUARE else [p["seeing"], None]
        for m in refusals:
            with pytest.raises(cmf.CMFError, match="needs") as ei:
                rule.set_mask(m)
            assert ei.value.code == 1, (form[0], "seeing" if m is not None else "unmasking")
        if form[1] == walk.DIV_SQUARE:  # (nothing is refused: the transition to another mask and back is exact instead)
            rule.set_mask(p["seeing"])
            rule.set_mask(p["mask"])
        got = (list(rule.iterate(2)),) + rule.download()
        want = (list(calm.iterate(2)),) + calm.download()
        for x, y in zip(got, want):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=form[0])
    finally:
        rule.close()
        calm.close()
