"""cmf.jl_amd/csrc/cmf_options.h (free of HIP) against tests/golden/option_walk.json, recorded through the strcmp chains the table
replaced: tests/option_table_driver.cpp (its own main, under ASan and UBSan) evaluates opt_decide at every "opt" cell of the recording.
Unknown names, values outside the accepted ranges and the refusals by kind of handle are settled by the decision alone: code and text
must be the recorded ones.  What the decision lets through is either recorded as accepted or refused by an effect that looks at the
handle's state (EFFECT_REFUSALS)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"few": "lone", "k32": "lone", "hals": "lone", "group": "group", "shard": "shard"}
# refusals that come from applying a row, not from deciding about it: hals_ensure on a shard
EFFECT_REFUSALS = {"HALS needs an unsharded handle (the H sweep is sequential along T)"}
LISTED = ["reuse_est", "speculate", "gram", "conv_kernel", "conv_split", "small_k", "small_k_fuse", "hals_prepare", "hals_gram", "hals_persist",
          "hals_general", "hals_seg", "hals_lag", "hals_debug", "hals_chase", "profile", "profile_mask", "allreduce_overlap", "enqueue_threads",
          "halo_in_allreduce"]
ON_NOTHING, ON_HANDLE, ON_GROUP, ON_SHARDS = range(4)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "option_walk.json")) as f:
        cells = json.load(f)["cells"]
    out = {}
    for key, cell in cells.items():
        section, kind, name, value = key.split("|")
        if section == "opt":
            out[(kind, name, int(value.split(":")[1]))] = (cell[0], cell[1])
    return out


@pytest.fixture(scope="module")
def decisions(golden, tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("option_table") / "option_table_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "cmf.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "option_table_driver.cpp"), "-o", exe])
    requests = sorted({(KINDS[kind], name, value) for kind, name, value in golden} | {("short_group", "gram", v) for v in (0, 1, 2)})
    env = {k: v for k, v in os.environ.items() if k != "CMF_TEST_HOOKS"}
    p = subprocess.run([exe], input="".join(f"{k}\t{n}\t{v}\n" for k, n, v in requests), env=dict(env, ASAN_OPTIONS="detect_leaks=1"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    assert p.stderr == f"ok {len(requests)} cells\n", p.stderr
    lines = p.stdout.splitlines()
    assert lines[0].split("\t")[0] == "names"
    out = {"names": lines[0].split("\t")[1].split(",")}
    for line in lines[1:]:
        key, code, msg, target = line.split("\t")
        kind, name, value = key.split("|")
        out[(kind, name, int(value))] = (int(code), msg, int(target))
    return out


def test_the_recording_holds_every_kind_of_refusal(golden):
    assert len(golden) >= 300 and {k[0] for k in golden} == set(KINDS)
    texts = {msg for code, msg in golden.values() if code}
    for part in ("unknown option 'no_such_option'", "must be 0 or 1", "on single-GPU handles only", "must be >= 0", "is a percentage",
                 "needs CMF_TEST_HOOKS=1", "gram must be 0, 1 or 2", "sharded handles take gram = 0 or 1", "not available on sharded handles",
                 "conv_kernel must be", "small_k_fuse must be", "signif_batch must be at least 0"):
        assert any(part in t for t in texts), part


def test_every_decision_is_the_recorded_one(golden, decisions):
    settled = 0
    for (kind, name, value), (code, msg) in golden.items():
        got_code, got_msg, target = decisions[(KINDS[kind], name, value)]
        if msg in EFFECT_REFUSALS:
            assert got_code == 0 and target != ON_NOTHING, (kind, name, value, got_code, got_msg)
            continue
        assert (got_code, got_msg) == (code, msg), (kind, name, value)
        settled += code != 0
    assert settled == sum(code != 0 and msg not in EFFECT_REFUSALS for code, msg in golden.values()) == 143  # (the recording's 145 refused options but hals_prepare on the group and on the shard)


def test_a_group_too_short_for_the_gram_form(decisions):
    """T < 4 L on a group of more than one rank: no shape of the recorded walk reaches this refusal, so its text is held to the one
    cmf_set_option had before the table (the accepted values are checked first; gram = 0 is always taken)."""
    assert decisions[("short_group", "gram", 0)] == (0, "", ON_GROUP)
    assert decisions[("short_group", "gram", 1)] == (4, "the Gram form on a sharded handle needs T >= 4 L (got T=30, L=8)", ON_NOTHING)
    assert decisions[("short_group", "gram", 2)] == (4, "sharded handles take gram = 0 or 1 (the loss of gram = 2 is not exact to 1e-4)", ON_NOTHING)


def test_what_a_row_is_applied_to(golden, decisions):
    """A lone handle takes the row itself; a group takes the group-level rows and "gram" as a group, every other row shard by shard; the
    group-level rows are nothing to a lone handle."""
    for (kind, name, value), (code, msg, target) in ((k, v) for k, v in decisions.items() if k != "names"):
        if code:
            assert target == ON_NOTHING
        elif name in ("allreduce_overlap", "enqueue_threads", "halo_in_allreduce"):
            assert target == (ON_GROUP if kind == "group" else ON_NOTHING), (kind, name)
        elif kind in ("group", "short_group"):
            assert target == (ON_GROUP if name == "gram" else ON_SHARDS), name
        else:
            assert target == ON_HANDLE, (kind, name)


def test_the_listed_names_are_the_listed_rows_in_order(decisions):
    assert decisions["names"] == LISTED


def test_the_header_is_free_of_hip_and_in_the_source_digest():
    text = open(os.path.join(ROOT, "cmf.jl_amd", "csrc", "cmf_options.h")).read()
    assert "hip/" not in text and "hipError" not in text and "__global__" not in text
    import importlib.util

    spec = importlib.util.spec_from_file_location("cmf_build_for_option_table", os.path.join(ROOT, "cmf.jl_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert any(p.endswith("cmf_options.h") for p in build.DEPS) and any(p.endswith("cmf_options.hip") for p in build.SOURCES)
