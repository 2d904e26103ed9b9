#!/usr/bin/env python3
"""What the event form of the KL rule costs against the dense KL rule (profiles/mu_kl_events.txt): ms per iteration of cmf_iterate
under divergence=":kl" and of cmf_events_iterate on the SAME data, in one process, at BASELINE config 2 (N=2000, T=50000, K=32, L=20)
and at the shape of the reference's loss-vs-time figure (N=250, T=50000, K=5, L=20), for counts at 1 %, 5 %, 25 % and 85 % density
(uniformly placed events with counts 1 .. 5; 85 % is about the density of the mu_kl_* fixtures).  Two warm-up runs, then the median, the
smallest and the largest of 7 runs (the run's wall time divided by its iterations; both entries return when the last loss has
arrived).  The last line per shape gives the density at which the two paths cross, interpolated in log density between the
measured points either side.

    python3 tools/time_events_kl.py [--shape config2|figure] [--out FILE]
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import cmf_jl_amd as cmf  # noqa: E402

SHAPES = {"config2": (2000, 50000, 32, 20), "figure": (250, 50000, 5, 20)}
DENSITIES = (0.01, 0.05, 0.25, 0.85)


def timed(rule, iters):
    for _ in range(2):
        rule.iterate(iters)
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        rule.iterate(iters)
        ts.append(1e3 * (time.perf_counter() - t0) / iters)
    return float(np.median(ts)), min(ts), max(ts)


def main():
    which = [sys.argv[sys.argv.index("--shape") + 1]] if "--shape" in sys.argv else list(SHAPES)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mu_kl_events.txt")
    lines = ["# ms per iteration: the dense KL rule (cmf_iterate) and the event form (cmf_events_iterate) on the same data, same process",
             "# shape | density | nnz | dense median min max | events median min max | dense / events | device bytes dense-data-copy vs events handle"]
    for name in which:
        N, T, K, L = SHAPES[name]
        rng = np.random.default_rng(1234)
        ratios = []
        for density in DENSITIES:
            data = (rng.random((N, T), dtype=np.float32) < density) * rng.integers(1, 6, (N, T), dtype=np.int8)
            data = np.asfortranarray(data, dtype=np.float64)
            events = cmf.EventData.from_dense(data)
            W0, H0 = cmf.init_rand_events(events, L, K, seed=0)
            dense = cmf.MultUpdate(data, W0, H0)
            dense.set_divergence(":kl")
            d_iters = 10 if name == "config2" else 50
            d = timed(dense, d_iters)
            dense.close()
            del data
            rule = cmf.EventKLUpdate(events, W0, H0)
            per = max(d[0], 1e-3) * max(density / 0.01, 1.0)  # (a guess that only sizes the run)
            e = timed(rule, int(min(50, max(2, round(200.0 / per)))))
            used = rule.counter("device_bytes")
            rule.close()
            ratios.append(d[0] / e[0])
            lines.append(f"{name} N={N} T={T} K={K} L={L} | {100 * density:g} % | {events.nnz} | {d[0]:.4f} {d[1]:.4f} {d[2]:.4f} | "
                         f"{e[0]:.4f} {e[1]:.4f} {e[2]:.4f} | {d[0] / e[0]:.2f} | {4 * N * T} vs {used}")
            print(lines[-1], flush=True)
        cross = None
        for i in range(len(DENSITIES) - 1):
            a, b = math.log(ratios[i]), math.log(ratios[i + 1])
            if a >= 0 > b:
                x = math.log(DENSITIES[i]) + a / (a - b) * (math.log(DENSITIES[i + 1]) - math.log(DENSITIES[i]))
                cross = math.exp(x)
        if cross is not None:
            lines.append(f"{name} | the two paths cross at about {100 * cross:.1f} % density")
        elif ratios[0] < 1:
            lines.append(f"{name} | the event form is slower than the dense rule at every density measured (from {100 * DENSITIES[0]:g} % up)")
        else:
            lines.append(f"{name} | the event form is faster than the dense rule at every density measured (up to {100 * DENSITIES[-1]:g} %)")
        print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
