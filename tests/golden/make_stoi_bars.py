#!/usr/bin/env python
"""Writes tests/golden/stoi_bars.json: how far the fp64 restatement of STOI / ESTOI (tests/stoi_ref.py) is from the same chain run in
np.longdouble (with a DFT matrix, numpy's FFT being double only), per stage, on the inputs of tests/test_stoi_gpu.py.  Runs on the
CPU and touches neither the kernels nor the package:

    python tests/golden/make_stoi_bars.py

Per stage the largest elementwise distance over all test pairs is recorded; the test's bar is FACTOR = 16 times that distance.  The
margin: the kernels sum in another order than either run (up to 256 terms per sum), so their rounding error is of the same size as
the fp64 restatement's but not the same value.  The end-to-end inputs at 22 050 Hz reach the restatement through the GPU resampler in
the test; here scipy's resample_poly (the same filter in fp64, rounded to float32) stands in for it: the signal differs in the last
float32 bit, the size of the chain's rounding error does not."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import stoi_ref as ref  # noqa: E402

FACTOR = 16
STAGES = {"energy": ("e",), "overlap_add": ("xo", "yo"), "bands": ("X", "Y"), "segments": ("seg",), "final": ("stoi", "estoi")}


def distances(pairs):
    worst = {k: 0.0 for k in STAGES}
    for x, y in pairs:
        a, b = ref.chain(x, y, np.float64), ref.chain(x, y, np.longdouble)
        assert np.array_equal(a["mask"], b["mask"]) and ref.threshold_margin(a) > 1e-6
        for stage, keys in STAGES.items():
            for k in keys:
                u, v = np.asarray(a[k], np.longdouble), np.asarray(b[k], np.longdouble)
                if u.size and not (stage == "final" and a["too_short"]):
                    worst[stage] = max(worst[stage], float(np.abs(u - v).max()))
    return worst


def main():
    from scipy.signal import resample_poly
    d10 = distances(ref.pairs())
    down = [(resample_poly(x.astype(np.float64), 200, 441).astype(np.float32), resample_poly(y.astype(np.float64), 200, 441).astype(np.float32))
            for x, y in ref.pairs_22k()]
    d22 = distances(down)
    out = {"seed": ref.SEED, "lengths": list(ref.LENGTHS), "lengths_22k": list(ref.LENGTHS_22K), "factor": FACTOR,
           "distance": {k: max(d10[k], d22[k]) if k == "final" else d10[k] for k in STAGES},
           "distance_10k": d10, "distance_22k_scipy_resampled": d22, "longdouble_eps": float(np.finfo(np.longdouble).eps)}
    path = os.path.join(ROOT, "tests", "golden", "stoi_bars.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
