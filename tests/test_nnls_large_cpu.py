"""CPU checks for the NNLS solver of 129 .. 1024 unknowns (option "nnls_large"): the inputs of tests/test_gpu_nnls_large.py satisfy
on the CPU what the project asks of every committed shape (anls_restatement.check_step, sep_restatement.check_problem), so that a
change of a restatement cannot silently void them; and the option is wired through every layer that can be looked at without a
device.  (kl640's restatement takes most of a minute; the GPU file runs check_step on it in its cached reference.)
"""
import ctypes
import os
import re

import numpy as np
import pytest

import anls_restatement as R
import sep_restatement as S
import test_gpu_nnls_large as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# pivoting rounds of the restatement, default mode, summed over the N problems
EXCHANGES = {"kl129": 49, "song_kl150": 79, "speech_kl240": 109, "kl320": 91}


@pytest.mark.parametrize("name", sorted(EXCHANGES))
def test_the_single_call_shapes_pass_check_step(name):
    data, W0, H0, W, near, floor, exchanges = G.reference(name)  # (asserts check_step)
    N, T, K, L = G.SHAPES[name]
    assert K * L > 128 and W.shape == (K, N, L)
    print(f"{name}: floor {floor:.2e}, near-degenerate {int(near.sum())} of {W.size}, exchanges {exchanges}")
    assert exchanges == EXCHANGES[name]
    if name in ("kl129", "song_kl150", "speech_kl240"):  # the shapes the GPU also runs under anls_backup_only
        sb = {}
        Wb = R.update_motifs(data, H0, L, backup_only=True, stats=sb)
        assert sb["capped"] == 0 and sb["backup"] > 0 and np.array_equal(Wb > 0, W > 0) and R.rel(Wb, W) <= R.bar(floor, 1e-8)


def test_the_fit_passes_check_step_at_every_half_step():
    N, T, K, L = G.SHAPES["song_kl150"]
    data, W0, H0 = R.problem(N, T, K, L, seed=G.FIT_SEED)
    W, H, hist, nearW, nearH, floor = G.restated_fit(data, W0, H0, L, G.FIT_ITERS, "block")
    print(f"fit: floor {floor:.2e}, loss_hist {hist.tolist()}")
    assert 0 < floor <= 1e-10 and (np.diff(hist) <= 1e-12).all()
    assert nearW.sum() <= 0.01 * W.size and nearH.sum() <= 0.01 * H.size


@pytest.mark.parametrize("case", sorted(G.SEP_CASES))
def test_the_separable_inputs_pass_check_problem(case):
    data, K, L, thresh, ref, floors = G.sep_reference(case)  # (asserts check_problem)
    assert K * L > 128 and ref["G"].shape == (K * L, data.shape[1])
    assert max(floors.values()) <= 1e-10


def test_the_option_is_wired_through_every_layer():
    import __graft_entry__

    __graft_entry__.build()
    import cmf_jl_amd as cmf

    lib = ctypes.CDLL(cmf.LIB_PATH)
    assert lib.cmf_set_option(None, b"nnls_large", 1) == 1  # a NULL handle is CMF_ERR_ARG
    buf = ctypes.create_string_buffer(1024)
    assert lib.cmf_option_names(buf, 1024) == 0 and b"nnls_large" not in buf.value  # not a path of the listed rules
    build = __import__("importlib").import_module(cmf.__name__ + ".build")
    assert "cmf_nnls_large.h" in [os.path.basename(p) for p in build.DEPS]
    hdr = open(os.path.join(ROOT, "include", "cmf_hip.h")).read()
    assert '"nnls_large"' in hdr and "cmf_nnls_large.h" in hdr
    host = __import__("importlib").import_module(cmf.__name__ + ".host")
    assert "nnls_large" in host._KNOWN_KW
    assert "nnls_large" in cmf.separable_fit.__doc__ and "nnls_large" in cmf.ANLSUpdate.__doc__
    table = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_options.h")).read()
    assert re.search(r'OPT_FLAG\(nnls_large, "[^\n"]*", 0\)', table)  # (a 0/1 row of cmf_set_option's table: single-GPU handles, not a gate)
    large = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_nnls_large.h")).read()
    assert re.search(r"constexpr int WLARGE = 1024;", large) and "nnls_large_kernel" in large
    for unit in ("cmf_anls.hip", "cmf_sep.hip"):
        assert '#include "cmf_nnls_large.h"' in open(os.path.join(ROOT, "cmf.jl_amd", "csrc", unit)).read(), unit
    jl = open(os.path.join(ROOT, "cmf.jl_amd", "julia", "CMFHip.jl")).read()
    assert re.search(r"set_option!\(rule::HIPANLSUpdate, name::AbstractString, value::Integer\)", jl) and "nnls_large::Bool=false" in jl
