"""The walk over the string-keyed surface of the C ABI -- every option of cmf_set_option, every counter of cmf_get_counter and
cmf_events_get_counter, every timed kernel name of cmf_time_kernel -- that tools/record_option_walk.py records and
tests/test_gpu_option_walk.py repeats (tests/golden/option_walk.json).

A cell is "section|handle kind|name|value".  Sections:

  opt       a fresh handle per (kind, name), the values of the name set one after the other.  Per value: the return code, the text of
            cmf_last_error when refused, and -- after uploading the initial factors again -- the SHA-256 of W, H and the losses of
            iterate(2), with the non-zero "launches:*" counters of the handle so far.  The digests show that an accepted value still
            selects the same launches.  Kinds: "few" and "k32" (lone handles on the two shapes of tests/test_gpu_mu_form_transitions.py:
            few components, K % 32 == 0), "group" (devices=[0, 0] on the first shape), "shard" (a per-process shard that has no
            communicator yet: code and text only, no rule call runs on it), "hals" (after hals_prepare, on a shape of the HALS parity
            tests; one HALS iteration instead of iterate(2)).
  counter   on a lone handle, the group and an event-list handle after a fixed script (small_k = 2, iterate(2), update_motifs,
            cmf_arm_writeback, update_feature_maps): code and value of every counter name, every "launches:" path and an unknown name
            of each kind.  The counters that hold host times are recorded by their code alone.
  time      cmf_time_kernel with reps = 1: code, text when refused, the flops value, and the digest of iterate(1) run straight after
            the call on freshly uploaded factors -- what the call leaves marked as the content of est decides whether the iteration
            recomputes it.  No time is compared.
  profile   cmf_kernel_times after set_option("profile", 1) and iterate(2): code and launch count per kernel class.

The values of an option are the ones the tests set on that kind of handle plus the first value on either side of each accepted range.
Nothing here sets CMF_TEST_HOOKS: "hals_debug" is walked with 0 and with the refusal of 1, and no bounded wait is made to run out.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

import cmf_jl_amd as cmf
from cmf_jl_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_problems as ep  # noqa: E402  (LAUNCH_PATHS, HALS_LAUNCH_PATHS: kept equal to the C++ tables by tests/test_exact_problems.py)

SHAPES = {"few": (48, 300, 4, 8), "k32": (40, 200, 32, 5), "group": (48, 300, 4, 8), "shard": (48, 300, 4, 8), "hals": (130, 900, 32, 20),
          "events": (24, 160, 3, 6)}
FLAG = [-1, 0, 1, 2]
# every listed name (cmf_option_names, in its order), the unlisted ones, one unknown name
VALUES = {
    "reuse_est": [0, 1], "speculate": [0, 1], "gram": [-1, 0, 1, 2, 3, 0], "conv_kernel": [-1, 0, 1, 2, 3, 4], "conv_split": [0, 1],
    "small_k": [0, 2, 1], "small_k_fuse": [-1, 0, 2, 3, 1], "hals_prepare": [1], "hals_gram": [0, 1, 3, 2],
    "hals_persist": [-1, 0, 2, 1], "hals_general": [-1, 3, 0], "hals_seg": [-1, 256, 1024], "hals_lag": [-1, 3, 2], "hals_debug": [-1, 0, 1],
    "hals_chase": [-2, -1, 0, 65, 100, 101], "profile": [1, 4, 0], "profile_mask": [1, 0],
    "allreduce_overlap": [1, 0], "enqueue_threads": [0, 1], "halo_in_allreduce": [0, 1],
    "signif_batch": [-1, 0, 7], "anls_backup_only": FLAG, "nnls_large": FLAG, "kl_mask": FLAG, "pq_mask": FLAG, "is_div": FLAG,
    "no_such_option": [1],
}
LISTED = list(VALUES)[:20]
HALS_NAMES = [n for n in VALUES if n.startswith("hals_")]
COUNTERS = ["hals_pipeline_reruns", "plan:n_cu", "writeback_calls", "speculated_contractions", "liveness_checks", "pow_update_launches",
            "xortho_launches", "signif_launches", "admm_W_reverts", "admm_H_reverts", "sep_nnls_exchanges", "anls_W_exchanges",
            "anls_H_exchanges", "anls_backup", "anls_capped", "small_k_fused_h_updates", "writeback_overlapped", "allreduce_calls",
            "allgather_calls", "halo_in_allreduce", "enqueue_ns", "enqueue_iters", "worker_ns", "no_such_counter"]
TIMING_DEPENDENT = ("liveness_checks", "enqueue_ns", "enqueue_iters", "worker_ns")  # (the code alone is recorded)
LAUNCHES = ["launches:" + p for p in ep.LAUNCH_PATHS + ep.HALS_LAUNCH_PATHS]
EVENT_COUNTERS = ["device_bytes", "launches", "ratio_passes", "nnz", "unit_chunk", "time_chunk", "keep_ratio", "unit_items", "time_items",
                  "unit_split", "time_split", "w_block_units", "h_block_columns", "ratio_waves", "no_such_counter", "launches:conv_kernel"]
TIMED = ["conv", "hxt", "transconv", "conv_t", "conv_loss", "conv_loss_store", "allreduce", "allreduce_gram", "allreduce_lane1", "allgather_halo",
         "signif_draw", "transconv1_sum", "no_such_kernel"]
PROFILED = ["conv", "conv_t", "conv_loss", "conv_loss_store", "hxt", "transconv", "hxt_num", "hxt_den", "other", "hals_h_pipeline", "hals_w_sweep",
            "conv_resid", "hxt_resid", "hxt_hh", "transconv_1src", "gram_denom_h", "gram_tables", "gram_w", "no_such_class"]

_PROBLEMS = {}
handles_made = 0


def problem(kind):
    """(data, W0, H0) of a kind's shape: computed once, shared and left unchanged."""
    shape = SHAPES[kind]
    if shape not in _PROBLEMS:
        N, T, K, L = shape
        data = np.maximum(cmf.gen_synthetic(N=N, T=T, K=3, L=L, seed=1234 + N), 0.0) + 0.05
        W0, H0 = cmf.init_rand(data, L=L, K=K, seed=T)
        for a in (data, W0, H0):
            a.setflags(write=False)
        _PROBLEMS[shape] = (np.asfortranarray(data), W0, H0)
    return _PROBLEMS[shape]


class Shard:
    """A handle of cmf_create_shard (the first half of the columns) that no communicator was attached to."""

    def __init__(self):
        data, _, _ = problem("shard")
        N, T, K, L = SHAPES["shard"]
        self._lib, self._h = _lib.load(), ctypes.c_void_p()
        local = _lib.farr(data[:, :T // 2 + L - 1])
        _lib.check(self._lib.cmf_create_shard(ctypes.byref(self._h), 0, N, T // 2, K, L, _lib.ptr(local), 0, T))

    def close(self):
        if self._h:
            self._lib.cmf_destroy(self._h)
            self._h = ctypes.c_void_p()


def make(kind):
    global handles_made
    handles_made += 1
    if kind == "shard":
        return Shard()
    data, W0, H0 = problem(kind)
    if kind == "hals":
        return cmf.HALSUpdate(data, W0, H0)
    if kind == "events":
        rng = np.random.default_rng(5)
        counts = rng.poisson(0.3, size=data.shape).astype(np.float64)
        return cmf.EventKLUpdate(cmf.EventData.from_dense(counts), W0, H0)
    return cmf.MultUpdate(data, W0, H0, devices=[0, 0] if kind == "group" else None)


def outcome(rc):
    """[return code, the text of cmf_last_error when refused]"""
    return [int(rc), "" if rc == 0 else _lib.load().cmf_last_error().decode("utf-8", "replace")]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def launches(rule):
    out = {}
    for name in LAUNCHES:
        v = rule.counter(name)
        if v:
            out[name[9:]] = v
    return out


def run_digest(rule, kind, n=2):
    """The digest of n iterations (HALS: one call-by-call iteration) from the initial factors, and the handle's launch counters."""
    _, W0, H0 = problem(kind)
    rule.upload(W0, H0)
    if kind == "hals":
        rule.update_motifs()
        losses = [rule.update_feature_maps()]
    else:
        losses = rule.iterate(n)
    W, H = rule.download()
    return [digest(W, H, losses), launches(rule)]


def option_names(kind):
    return HALS_NAMES if kind == "hals" else list(VALUES)


def walk_options(kind, name):
    """{key: cell} of one (kind, name): a fresh handle, the values in their order."""
    cells = {}
    rule = make(kind)
    try:
        for i, value in enumerate(VALUES[name]):
            cell = outcome(rule._lib.cmf_set_option(rule._h, name.encode(), int(value)))
            if kind != "shard":
                cell += run_digest(rule, kind)
            cells[f"opt|{kind}|{name}|{i}:{value}"] = cell
    finally:
        rule.close()
    return cells


def walk_counters(kind):
    cells = {}
    rule = make(kind)
    try:
        _, W0, H0 = problem(kind)
        if kind != "events":  # (the few-component C3 form whatever T is: its fused H updates make the counter that is summed over shards non-zero)
            rule.set_option("small_k", 2)
        rule.iterate(2)
        rule.update_motifs()
        if kind != "events":
            W, H = np.array(W0, order="F", copy=True), np.array(H0, order="F", copy=True)
            _lib.check(rule._lib.cmf_arm_writeback(rule._h, _lib.ptr(W), _lib.ptr(H)))
        rule.update_feature_maps()
        get = rule._lib.cmf_events_get_counter if kind == "events" else rule._lib.cmf_get_counter
        for name in (EVENT_COUNTERS if kind == "events" else COUNTERS + LAUNCHES + ["launches:no_such_path"]):
            v = ctypes.c_int64(-1)
            cell = outcome(get(rule._h, name.encode(), ctypes.byref(v)))
            cells[f"counter|{kind}|{name}|"] = cell + ([] if name in TIMING_DEPENDENT and kind != "events" else [v.value])
    finally:
        rule.close()
    return cells


def walk_timed(kind):
    cells = {}
    rule = make(kind)
    try:
        _, W0, H0 = problem(kind)
        for name in TIMED:
            rule.upload(W0, H0)
            ms, fl = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
            cell = outcome(rule._lib.cmf_time_kernel(rule._h, name.encode(), 1, ctypes.byref(ms), ctypes.byref(fl)))
            losses = rule.iterate(1)
            W, H = rule.download()
            cells[f"time|{kind}|{name}|"] = cell + [fl.value, digest(W, H, losses)]
    finally:
        rule.close()
    return cells


def walk_profile(kind):
    cells = {}
    rule = make(kind)
    try:
        rule.set_option("profile", 1)
        rule.iterate(2)
        for name in PROFILED:
            ms, n = ctypes.c_double(-1.0), ctypes.c_int64(-1)
            cell = outcome(rule._lib.cmf_kernel_times(rule._h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
            cells[f"profile|{kind}|{name}|"] = cell + [n.value]
    finally:
        rule.close()
    return cells


def walk():
    """Every cell, in recording order."""
    assert "CMF_TEST_HOOKS" not in os.environ, "the walk records the library without its test hooks"
    buf = ctypes.create_string_buffer(4096)
    _lib.check(_lib.load().cmf_option_names(buf, 4096))
    assert buf.value.decode().split(",") == LISTED, "VALUES must begin with the names of cmf_option_names, in its order"
    cells = {}
    for kind in ("few", "k32", "group", "shard", "hals"):
        for name in option_names(kind):
            cells.update(walk_options(kind, name))
    for kind in ("few", "group", "events"):
        cells.update(walk_counters(kind))
    for kind in ("few", "k32", "group"):
        cells.update(walk_timed(kind))
    cells.update(walk_profile("few"))
    return cells
