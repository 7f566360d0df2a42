#!/usr/bin/env python
"""Writes tests/golden/postfilter_bars.json: how far the fp64 restatement of the modulation-spectrum postfilter
(tests/postfilter_ref.py: two-pass statistics, np.fft.rfft / irfft) is from the same chain in np.longdouble (direct sums against
extended-precision twiddles), per case and per floating output, on the inputs of tests/test_postfilter_gpu.py and
tests/test_postfilter_cpu.py.  Runs on the CPU, for a few minutes, and touches neither the kernels nor the package:

    python tests/golden/make_postfilter_bars.py

Per case and output the largest elementwise distance over the case's rows is recorded; a test's bar is FACTOR = 16 times that
distance, the margin of modspec_bars.json and for the same reason: the kernels sum in another order than either run, and all three
sit within a small multiple of fp64 rounding of the true value.  For a known answer the distance of the longdouble run to the
closed form is recorded as well (`to_expected`): what the closed form itself is good for.  Nothing a kernel produced enters the file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import postfilter_ref as ref  # noqa: E402

FACTOR = 16


def _dist(a, b):
    return float(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble)).max())


def stats_distance(rows):
    a, b = ref.statistics(rows, np.float64), ref.statistics(rows, np.longdouble)
    return {"mean": _dist(a[0], b[0]), "sd": _dist(a[1], b[1])}


def filter_distance(rows, tab, k):
    return {"y": max(_dist(ref.apply(c, tab, k, np.float64), ref.apply(c, tab, k, np.longdouble)) for c in rows)}


def main():
    cases = lambda d: {k: {"seed": v[0], "K": v[1], "frames": list(v[2])} for k, v in d.items()}    # noqa: E731
    out = {"factor": FACTOR, "stats_cases": cases(ref.STATS_CASES), "filter_cases": cases(ref.FILTER_CASES), "filter_k": ref.FILTER_K,
           "known": [ref.KNOWN_SEED, ref.KNOWN_T, ref.KNOWN_COEF, list(ref.GAINS), list(ref.KNOWN_K), ref.CLAMP_BIN, ref.CLAMP_DB],
           "longdouble_eps": float(np.finfo(np.longdouble).eps), "distance": {}}
    for name, (c, tab, k, expected) in ref.known_cases().items():
        exact = ref.apply(c, tab, k, np.longdouble)
        out["distance"][name] = {"y": _dist(ref.apply(c, tab, k, np.float64), exact), "to_expected": _dist(exact, expected)}
        print(name, out["distance"][name], flush=True)
    for name in ref.STATS_CASES:
        out["distance"][name] = stats_distance(ref.stats_input(name))
        print(name, out["distance"][name], flush=True)
    for name in ref.FILTER_CASES:
        rows, tab = ref.filter_input(name)
        out["distance"][name] = filter_distance(rows, tab, ref.FILTER_K[name])
        print(name, out["distance"][name], flush=True)
    path = os.path.join(ROOT, "tests", "golden", "postfilter_bars.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
