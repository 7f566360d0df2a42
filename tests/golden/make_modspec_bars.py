#!/usr/bin/env python
"""Writes tests/golden/modspec_bars.json: how far the fp64 restatement of the over-smoothing scores (tests/modspec_ref.py: numpy
sums, np.fft.rfft) is from the same chain in np.longdouble (a direct sum against extended-precision twiddles), per case and per
floating output, on the inputs of tests/test_modspec_gpu.py and tests/test_modspec_cpu.py.  Runs on the CPU, for about a minute,
and touches neither the kernels nor the package:

    python tests/golden/make_modspec_bars.py

Per case and output the largest elementwise distance over the case's rows is recorded; a test's bar is FACTOR = 16 times that
distance, the margin of stoi_bars.json and for the same reason: the kernels sum in another order than either run, and all three
sit within a small multiple of fp64 rounding of the true value.  Nothing a kernel produced enters the file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import modspec_ref as ref  # noqa: E402

FACTOR = 16


def distances(rows, tables):
    worst = {}
    for c in rows:
        a, b = ref.chain(c, tables, np.float64), ref.chain(c, tables, np.longdouble)
        pairs = [(k, a[k], b[k]) for k in ("mean", "m2", "gv", "logms")]
        pairs += [(f"bands_{sr}_{hop}", u, v) for (sr, hop), u, v in zip(ref.RATES, a["bands"], b["bands"])]
        for k, u, v in pairs:
            worst[k] = max(worst.get(k, 0.0), float(np.abs(np.asarray(u, np.longdouble) - v).max()))
    return worst


def main():
    tables = [ref.band_bins(sr, hop)[0] for sr, hop in ref.RATES]
    out = {"factor": FACTOR, "cases": {k: {"seed": v[0], "K": v[1], "frames": list(v[2])} for k, v in ref.CASES.items()},
           "cosine": [ref.COSINE_A, ref.COSINE_T, ref.COSINE_CYCLES], "constant": [ref.CONSTANT, ref.CONSTANT_T],
           "longdouble_eps": float(np.finfo(np.longdouble).eps), "distance": {}}
    for name in list(ref.CASES) + ["cosine", "constant"]:
        out["distance"][name] = distances(ref.case_input(name), tables)
        print(name, out["distance"][name], flush=True)
    path = os.path.join(ROOT, "tests", "golden", "modspec_bars.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
