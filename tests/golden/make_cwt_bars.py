#!/usr/bin/env python
"""Writes tests/golden/cwt_bars.json: how far the fp64 restatement of the wavelet prosody scores (tests/cwt_ref.py: explicit loops,
numpy sums, an FFT convolution) is from the same stage in np.longdouble (direct sums), per case and per floating output, on the
inputs of tests/test_cwt_gpu.py.  Runs on the CPU, for about a minute, and touches neither the kernels nor the package:

    python tests/golden/make_cwt_bars.py

Every stage is measured alone, as the kernels are tested: the longdouble stage is fed the fp64 restatement's own upstream values
(the contour the F0 track, the transform the fp64 z, the path sums the fp64 W).  Per case and output the largest elementwise
distance over the case's rows is recorded; a test's bar is FACTOR = 16 times that distance, the margin of modspec_bars.json and
for the same reason: the kernels sum in another order than either run, and all three sit within a small multiple of fp64 rounding
of the true value.  Where a distance is exactly 0 the kernel has to match exactly; that happens only for outputs that are 0 by
definition (the z, W and power of a flat row).  Nothing a kernel produced enters the file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import cwt_ref as ref  # noqa: E402

FACTOR = 16
LD = np.longdouble


def _dist(u, v):
    return float(np.abs(np.asarray(u, LD) - np.asarray(v, LD)).max())


def _fold(worst, key, d):
    worst[key] = max(worst.get(key, 0.0), d)


def track_distances(rows):
    worst = {}
    for f0 in rows:
        a, b = ref.contour(f0), ref.contour(f0, LD)
        assert a["flat"] == b["flat"] and a["n_voiced"] == b["n_voiced"]
        for k in ("z", "m", "sd"):
            _fold(worst, k, _dist(a[k], b[k]))
        for sr, hop in ref.RATES:
            (W, p), (Wl, pl) = ref.transform(a["z"], sr, hop), ref.transform(a["z"], sr, hop, LD)
            _fold(worst, f"W_{sr}_{hop}", _dist(W, Wl))
            _fold(worst, f"power_{sr}_{hop}", _dist(p, pl))
    return worst


def path_distance(name):
    f0a, f0b, pi, pj = ref.path_case(name)
    sr, hop = ref.RATES[0]
    Wa, Wb = ref.transform(ref.contour(f0a)["z"], sr, hop)[0], ref.transform(ref.contour(f0b)["z"], sr, hop)[0]
    return {"sums": _dist(ref.path_sums(pi, pj, Wa, Wb), ref.path_sums(pi, pj, Wa, Wb, LD))}


def main():
    out = {"factor": FACTOR, "longdouble_eps": float(np.finfo(LD).eps), "distance": {},
           "cases": {k: {"seed": v[0], "rows": [list(r) for r in v[1]]} for k, v in ref.CASES.items()},
           "path_cases": {k: list(v) for k, v in ref.PATH_CASES.items()}}
    for name in ref.CASES:
        out["distance"][name] = track_distances(ref.case_input(name))
        print(name, out["distance"][name], flush=True)
    for name in ref.PATH_CASES:
        out["distance"][name] = path_distance(name)
        print(name, out["distance"][name], flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "cwt_bars.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
