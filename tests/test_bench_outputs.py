"""bench.py's plain run, --full and --dump-outputs: what a plain line carries, what moved behind --full, and that the dumped
arrays are what the timed steps computed (CPU: the options and the size limit of the dump; GPU: whole runs on a short T)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "kernels_standalone", "cpu_baseline")


def test_steps_and_warmup_are_checked():
    import bench

    for argv in (["--steps", "0"], ["--steps", "-1"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)
    args = bench.parse_args(["--steps", "7", "--warmup", "0"])
    assert args.steps == 7 and args.warmup == 0 and not args.full and args.dump_outputs == ""


def test_children_get_full_and_an_absolute_dump_dir(tmp_path, monkeypatch):
    """The supervisor's children run in the repository root: a relative DIR must still mean the caller's directory."""
    import bench

    monkeypatch.chdir(tmp_path)
    args = bench.parse_args(["--gpus", "2", "--full", "--dump-outputs", "out"])
    cmd = bench.child_command(args, "multi")
    assert "--full" in cmd and cmd[cmd.index("--dump-outputs") + 1] == str(tmp_path / "out")
    cmd = bench.child_command(bench.parse_args(["--gpus", "2"]), "multi")
    assert "--full" not in cmd and "--dump-outputs" not in cmd


def test_dump_outputs_stays_within_its_limit(tmp_path, monkeypatch):
    import bench

    rng = np.random.default_rng(1)
    arrays = {"W": rng.random((4, 50, 3)), "H": rng.random((4, 900)), "loss": [1.25]}
    bench.dump_outputs(str(tmp_path / "a"), arrays)  # small: float64, whole arrays
    for name, a in arrays.items():
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, np.asarray(a))
    # float32 when float64 would not fit, and a fixed sample when float32 would not either
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 4096 + 4 * 5000)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert np.array_equal(np.load(tmp_path / "b" / "H.npy"), arrays["H"].astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 4096 + 4 * 1000)
    for d in ("c", "d"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    sizes = 0
    for name, a in arrays.items():
        got = np.load(tmp_path / "c" / f"{name}.npy")
        assert got.dtype == np.float32 and got.size >= 1 and np.array_equal(got, np.load(tmp_path / "d" / f"{name}.npy"))
        assert np.isin(got, np.asarray(a, dtype=np.float32)).all()
        sizes += got.nbytes
    assert sizes <= 4 * 1000


def run_bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path, oracle):
    """A plain run of config 2 on 2000 columns: the headline fields and nothing that moved behind --full; the dumped W, H and
    loss are the oracle's after warm-up + timed steps (so --warmup and --steps set how many steps ran).  Then the same
    arguments with --full: the side measurements are back, and the dumped arrays are still those of the timed steps."""
    import cmf_jl_amd as cmf

    N, T, K, L, warmup, steps = 2000, 2000, 32, 20, 2, 4
    common = ["--T", str(T), "--steps", str(steps), "--warmup", str(warmup)]
    line = run_bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    for k in HEADLINE:
        assert line[k] is not None, k
    assert line["steps"] == steps and line["warmup"] == warmup and line["value"] > 0 and line["dtype"] == "f32"
    assert abs(line["ms_per_step"] - 1e3 / line["value"]) <= 1e-9 * line["ms_per_step"]
    assert not [k for k in FULL_ONLY if k in line] and line["sustained"] is None and line["call_by_call"] is None

    W = np.load(tmp_path / "plain" / "W.npy")
    H = np.load(tmp_path / "plain" / "H.npy")
    loss = np.load(tmp_path / "plain" / "loss.npy")
    assert W.dtype == H.dtype == loss.dtype == np.float64 and W.shape == (K, N, L) and H.shape == (K, T) and loss.shape == (1,)
    assert loss[0] == line["config"]["loss_last"]
    data = cmf.gen_synthetic(N=N, T=T, seed=1234, device=0)
    W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0, device=0)
    Wr, Hr, lr, _ = oracle.fit_mult(data, W0, H0, max_itr=warmup + steps, check_convergence=False)
    assert rel(W, Wr) < 1e-4 and rel(H, Hr) < 1e-4 and abs(loss[0] - lr[-1]) <= 1e-4 * lr[-1]

    full = run_bench(common + ["--full", "--cpu-seconds", "0", "--sustain", "0.2", "--dump-outputs", str(tmp_path / "full")])
    assert full["roofline"]["frac"] > 0 and full["kernels_standalone"] and full["kernels"] and full["sustained"]["steps"] > 0
    assert full["ms_per_step_no_reuse"] > 0 and full["call_by_call"]["ms_per_step_call_by_call"] > 0 and full["ms_per_step_gram"] > 0
    assert rel(np.load(tmp_path / "full" / "W.npy"), W) < 1e-6 and rel(np.load(tmp_path / "full" / "H.npy"), H) < 1e-6
