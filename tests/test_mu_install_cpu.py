"""cmf.jl_amd/csrc/cmf_mu_install.h (free of HIP) against tests/golden/mu_form_transitions.json, the matrix recorded through the library
before the forms' installers became one transition: tests/mu_install_matrix.cpp (its own main, under ASan and UBSan) evaluates the
refusal function at every cell; every code must be the recorded one wherever the data did not decide, and every text must name the form
it is about and the way out."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"kl": "KL", "is": "Itakura-Saito", "beta": "beta-divergence"}
TARGETS = {"kind_kl": "KL", "kind_is": "Itakura-Saito", "beta_0.5": "beta-divergence", "beta_1.5": "beta-divergence"}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "mu_form_transitions.json")) as f:
        return json.load(f)["cells"]


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("mu_install") / "mu_install_matrix")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "cmf.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "mu_install_matrix.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    assert p.stderr.startswith("ok "), p.stderr
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    cells = {}
    for line in p.stdout.splitlines():
        key, code, msg = line.split("\t")
        cells[key] = (int(code), msg)
    return cells


def test_the_golden_file_is_the_whole_walk(golden):
    """8 forms under the gate settings each can exist under, gram = 1 and active weights beside the plain square form, both data sets."""
    assert len(golden) == 1768
    states = {k.rsplit("|", 1)[0] for k in golden}
    assert len({s for s in states if s.startswith("pos|plain|")}) == 8 + 8 + 8 + 4 + 4 + 2 + 8 + 4
    assert all(v[0] in (0, 1, 3, 4) and isinstance(v[2], bool) for v in golden.values())
    # the data decides only where a divergence's check meets the entry the mask holds out: always CMF_ERR_ARG, the handle as it was
    dd = {k: v for k, v in golden.items() if v[2]}
    assert dd and all(k.startswith("holed|") and v[0] == 1 and v[1] == k.split("|")[2] for k, v in dd.items())
    # ... and a refused request never changes the form
    assert all(v[1] == k.split("|")[2] for k, v in golden.items() if v[0] != 0)


def test_every_code_is_the_recorded_one(golden, matrix):
    checked = 0
    for key, (code, after, data_dependent) in golden.items():
        if data_dependent:
            continue
        got = matrix[key.split("|", 1)[1]][0]
        assert got == code, (key, got, code)
        checked += 1
    assert checked == len(golden) - sum(v[2] for v in golden.values()) >= 1700


def expected_words(start, form, request, code):
    """What the text of a refusal must hold: the name of the form it is about and the way out."""
    div, masked = form.split("+")[0].split("(")[0], form.endswith("+mask")
    if code == 1:  # an argument the call never takes
        return ["kind must be", "CMF_DIV_SQUARE"] if request == "kind_is" else ["beta", "CMF_DIV_IS", "CMF_DIV_KL"]
    if code == 3:
        if request.endswith("_0"):  # a gate that cannot go
            return [request[:-2] + ":", NAMES[div], "CMF_DIV_SQUARE"]
        if masked and request.startswith("hals"):
            return ["cmf_mu_set_mask", "HALS rule has no masked form", "clear it first"]
        return [NAMES[div], "is installed", "squared error only", "CMF_DIV_SQUARE"]
    assert code == 4
    if request == "set_mask":
        return {"gram": ["Gram", "no masked form", "gram = 0"], "xortho": ["cmf_mu_set_xortho", "no masked form", "weights to 0"]}.get(
            start, [NAMES.get(div), "no masked form", "CMF_DIV_SQUARE"])
    if request in TARGETS:
        return {"gram": [TARGETS[request], "Gram", "gram = 0"], "xortho": ["cmf_mu_set_xortho", "divergence", "weights to 0"]}.get(
            start, [TARGETS[request], "no masked form", "cmf_mu_set_mask"])
    if request == "gram_1":
        return ([NAMES[div], "Gram", "CMF_DIV_SQUARE"] if div != "square" else ["Gram", "no masked form", "cmf_mu_set_mask"] if masked
                else ["Gram", "cmf_mu_set_xortho", "weights to 0"])
    assert request == "xortho_1_0_0"
    return (["cross-orthogonality", "no masked form", "cmf_mu_set_mask"] if masked else ["cross-orthogonality", "divergence", "CMF_DIV_SQUARE"] if div != "square"
            else ["cross-orthogonality", "Gram", "gram = 0"])


def test_every_text_names_its_form_and_the_way_out(golden, matrix):
    refused = 0
    for key, (code, msg) in matrix.items():
        start, form, gates, request = key.split("|")
        if "pos|" + key not in golden:
            continue
        if code == 0:
            assert msg == ""
            continue
        for word in expected_words(start, form, request, code):
            assert word in msg, (key, word, msg)
        refused += 1
    assert refused > 300


def test_the_header_is_free_of_hip_and_in_the_source_digest():
    text = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_mu_install.h")).read()
    assert "hip/" not in text and "hipError" not in text and "__global__" not in text
    import importlib.util

    spec = importlib.util.spec_from_file_location("cmf_build_for_mu_install", os.path.join(ROOT, "cmf.jl_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert any(p.endswith("cmf_mu_install.h") for p in build.DEPS)
