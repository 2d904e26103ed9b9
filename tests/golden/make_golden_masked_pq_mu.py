"""Generates the fixtures of the Itakura-Saito and beta forms of the MU rule under a 0/1 mask in tests/golden/
(mu_masked_is_*.npz, mu_masked_beta_*_bNNN.npz) from tests/masked_pq_mu_restatement.py.

A fixture holds NO inputs: data, the mask and the initial factors are regenerated from seeds by
masked_pq_mu_restatement.synthetic_case(shape, kind), and the fit runs on data with NaN under mask == 0, which is also how the
fixture is loaded.  Stored: the shape, the mask kind, beta (0: Itakura-Saito), the regularisers, max_itr, loss_hist and the float32
roundings of W and H of the fp64 restatement (6e-8 relative, against a bar of 1e-4).  Where the two together would pass the 250 000
bytes of a golden file, W32 goes into a companion file <stem>_W.npz that the fixture names (`W_file`).

    (48, 300, 4, 8)      blocks of L; the same with all four regularisers; for beta = 0.25, 2, 3 too
    (250, 2000, 5, 20)   50 % speckle           (37, 150, 33, 7)  blocks + one unit and one sample never observed
    (96, 1000, 32, 12)   blocks                 (20, 200, 6, 40)  blocks
    (6, 3, 2, 5)         blocks, T < L          (20, 7, 2, 10)    blocks + a unit and a sample never observed, T < L
    (250, 2000, 5, 20) and (96, 1000, 32, 12) also under every mask kind x with / without regularisers x beta 0, 0.5, 1.5, two
    iterations each; the same combinations of the small shapes have no fixture (LIVE: the tests run the restatement themselves)

The iteration count of a case is the one asked for here, cut to what profiles/mu_masked_pq_precision.txt admits
(tools/mu_masked_pq_precision.py, which reads CASES from here).

Run from the repo root:  python tests/golden/make_golden_masked_pq_mu.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import masked_pq_mu_restatement as pm  # noqa: E402

_EVERY = (((48, 300, 4, 8), "blocks", False, 20), ((48, 300, 4, 8), "blocks", True, 20), ((250, 2000, 5, 20), "speckle", False, 10),
          ((96, 1000, 32, 12), "blocks", False, 10), ((37, 150, 33, 7), "dead", False, 20), ((20, 200, 6, 40), "blocks", False, 20),
          ((6, 3, 2, 5), "blocks", False, 5), ((20, 7, 2, 10), "dead", False, 5))
# (shape, mask kind, regularised, beta, iterations asked for)
CASES = tuple((s, k, r, b, n) for b in pm.BETAS for s, k, r, n in _EVERY) + tuple((_EVERY[0][0], "blocks", False, b, 20) for b in pm.BETAS_FIRST)
# the two large shapes, whose fp64 restatement costs seconds per iteration, under EVERY mask kind, with and without the regularisers,
# for every beta of pm.BETAS: two iterations each (the long runs are the two above)
LARGE = ((250, 2000, 5, 20), (96, 1000, 32, 12))
CASES += tuple((s, k, r, b, 2) for s in LARGE for k in pm.MASKS for r in (False, True) for b in pm.BETAS
               if (s, k, r, b) not in {c[:4] for c in CASES})
# every other (shape, mask kind, regularised, beta of pm.BETAS): no fixture, the GPU test runs the restatement itself (it is quick on
# these shapes); listed here so that the precision profile admits their counts too
LIVE = tuple((s, k, r, b, 5) for s in pm.SHAPES if s not in LARGE for k in pm.MASKS for r in (False, True) for b in pm.BETAS
             if (s, k, r, b) not in {c[:4] for c in CASES})
PROFILE = os.path.join(ROOT, "profiles", "mu_masked_pq_precision.txt")
LIMIT = 250_000


def admitted(path=PROFILE):
    """{case name: admitted iteration count} of the `admit` lines."""
    out = {}
    for line in open(path):
        if line.startswith("admit "):
            _, name, n = line.split()
            out[name] = int(n)
    return out


def count_of(case, adm):
    shape, kind, reg, beta, want = case
    return min(want, adm[pm.case_name(shape, kind, reg, beta)])


def main():
    adm = admitted()
    for case in CASES:
        shape, kind, with_reg, beta, _ = case
        itr = count_of(case, adm)
        assert itr >= 1, case
        data, _, mask, W0, H0 = pm.synthetic_case(shape, kind)
        reg = dict(pm.REG) if with_reg else dict(l1W=0.0, l2W=0.0, l1H=0.0, l2H=0.0)
        W, H, lh = pm.fit_masked_pq(data, mask, W0, H0, beta, max_itr=itr, **reg)
        name = pm.fixture_name(shape, kind, with_reg, beta)
        path = os.path.join(HERE, name)
        meta = dict(shape=np.asarray(shape), kind=kind, beta=beta, loss_hist=lh, max_itr=itr, **reg)
        np.savez_compressed(path, W32=W.astype(np.float32), H32=H.astype(np.float32), **meta)
        if os.path.getsize(path) > LIMIT:
            wname = name[:-4] + "_W.npz"
            np.savez_compressed(os.path.join(HERE, wname), W32=W.astype(np.float32))
            np.savez_compressed(path, W_file=wname, H32=H.astype(np.float32), **meta)
            assert os.path.getsize(os.path.join(HERE, wname)) <= LIMIT
        print(name, shape, kind, "beta", beta, "itr", itr, "observed", float(mask.mean()), "loss", lh[0], "->", lh[-1], os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= LIMIT


if __name__ == "__main__":
    main()
