"""A / B of the PGD rule in two builds of the library on the SAME GPU box, in alternating child processes (tools/ab_small_k.py's pattern):
    python tools/ab_pgd.py <other tree root> [N T K L]
Call-by-call iterations (update_motifs + update_feature_maps) on a lone handle and as devices=[0, 0]: two warm-up iterations, then the
median of 20, three alternations per build; last the median of medians per build and form and the other tree's max - min."""
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time, statistics
sys.path.insert(0, sys.argv[1])
import cmf_jl_amd as cmf
N, T, K, L = (int(a) for a in sys.argv[2:6])
data = cmf.gen_synthetic(N=N, T=T, seed=1234)
W0, H0 = cmf.init_rand(data, L=L, K=K, seed=0)
for devices in (None, [0, 0]):
    rule = cmf.PGDUpdate(data, W0, H0, devices=devices)
    ms = []
    for it in range(22):
        t0 = time.perf_counter()
        rule.update_motifs()
        rule.update_feature_maps()  # (returns the loss: synchronises)
        ms.append(1e3 * (time.perf_counter() - t0))
    rule.close()
    print(f"{statistics.median(ms[2:]):.4f}")
'''
other = os.path.abspath(sys.argv[1])
shape = sys.argv[2:6] or ["2000", "50000", "32", "20"]
meds = {}
for rep in range(3):
    for name, root in (("this tree", HERE), ("other tree", other)):
        out = subprocess.run([sys.executable, "-c", CHILD, root] + shape, capture_output=True, text=True, timeout=280)
        vals = [float(x) for x in out.stdout.split()]
        if out.returncode != 0 or len(vals) != 2:
            sys.exit(f"{name}: child ended with {out.returncode}: {out.stderr[-400:]}")
        for form, v in zip(("lone", "devices=[0, 0]"), vals):
            meds.setdefault((name, form), []).append(v)
        print(f"N,T,K,L={','.join(shape)} run {rep + 1} {name:10s}: ms per iteration (median of 20) lone {vals[0]:.4f}  devices=[0, 0] {vals[1]:.4f}", flush=True)
ok = True
for form in ("lone", "devices=[0, 0]"):
    a, b = meds[("this tree", form)], meds[("other tree", form)]
    over, spread = statistics.median(a) - statistics.median(b), max(b) - min(b)
    ok &= over <= spread
    print(f"{form}: median of medians this tree {statistics.median(a):.4f} ms, other tree {statistics.median(b):.4f} ms; "
          f"this - other {over:+.4f} ms, other tree's max - min {spread:.4f} ms: {'within' if over <= spread else 'OVER'}")
sys.exit(0 if ok else 1)
