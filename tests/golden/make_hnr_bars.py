#!/usr/bin/env python
"""Writes tests/golden/hnr_bars.json: how far the fp64 restatement of the harmonics-to-noise ratio (tests/hnr_ref.py: explicit
indexing, np.correlate, numpy sums) is from the same stage in np.longdouble (its own tables, dot products), per case and per
floating output, on the inputs of tests/test_hnr_gpu.py.  Runs on the CPU, for well under a minute, and touches neither the kernels
nor the package:

    python tests/golden/make_hnr_bars.py

Every stage is measured alone, as the kernels are tested: the frames from the audio and the track (the longdouble chain at the fp64
chain's lag, so that the two are the same function), the per-side moments and the path sums from the fp64 frames.  Per case and
output the largest elementwise distance over the case's rows is recorded; a test's bar is FACTOR = 16 times that distance, the
margin of cwt_bars.json and for the same reason: the kernels sum in another order than either run, and all three sit within a small
multiple of fp64 rounding of the true value.  Nothing a kernel produced enters the file.

The lag tau* is an argmax, which rounding can move where two lags tie: a test compares it only at frames whose best lag leads the
runner-up by more than the bar of r'.  `left_out` counts the valid frames of a case where the restatement's own margin is not above
that bar; this script refuses to write a file in which they are more than 1 % of the valid frames of all cases together."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import hnr_ref as ref  # noqa: E402

FACTOR = 16
LD = np.longdouble


def _dist(u, v):
    d = np.abs(np.asarray(u, LD) - np.asarray(v, LD))
    return float(np.nanmax(d)) if d.size and not np.isnan(d).all() else 0.0


def case_distances(name):
    fs, hop, rows = ref.case_input(name)
    worst = {"r": 0.0, "hnr": 0.0, "rprime": 0.0, "side_mean": 0.0, "side_m2": 0.0}
    margins = []
    for y, f0 in rows:
        fr, lag, rp, margin = ref.frames(y, f0, fs, hop)
        frl, lagl, rpl, _ = ref.frames(y, f0, fs, hop, LD, lags=lag)
        assert np.array_equal(fr[:, 2], frl[:, 2]) and np.array_equal(lag, lagl)
        for key, d in (("r", _dist(fr[:, 0], frl[:, 0])), ("hnr", _dist(fr[:, 1], frl[:, 1])), ("rprime", _dist(rp, rpl))):
            worst[key] = max(worst[key], d)
        s, sl = ref.side(fr), ref.side(fr, LD)
        worst["side_mean"], worst["side_m2"] = max(worst["side_mean"], _dist(s[1], sl[1])), max(worst["side_m2"], _dist(s[2], sl[2]))
        margins.append(margin[fr[:, 2] != 0])
    margins = np.concatenate(margins)
    return worst, len(margins), int((margins <= FACTOR * worst["rprime"]).sum())


def path_distance(name):
    fa, fb, pi, pj = ref.path_case(name)
    s, sl = ref.path_sums(pi, pj, fa, fb), ref.path_sums(pi, pj, fa, fb, LD)
    return {"path_mean": _dist(s[1:3], sl[1:3]), "path_sums": _dist(s[3:], sl[3:])}


def main():
    out = {"factor": FACTOR, "longdouble_eps": float(np.finfo(LD).eps), "distance": {}, "valid_frames": {}, "left_out": {},
           "cases": {k: {"fs": v[0], "hop": v[1], "seed": v[2], "rows": [list(r) for r in v[3]]} for k, v in ref.CASES.items()},
           "path_cases": list(ref.PATH_CASES)}
    for name in ref.CASES:
        out["distance"][name], out["valid_frames"][name], out["left_out"][name] = case_distances(name)
        print(name, out["distance"][name], out["valid_frames"][name], out["left_out"][name], flush=True)
    for name in ref.PATH_CASES:
        out["distance"][name] = path_distance(name)
        print(name, out["distance"][name], flush=True)
    assert 100 * sum(out["left_out"].values()) <= sum(out["valid_frames"].values()), "more than 1 % of the valid frames tie"
    with open(os.path.join(ROOT, "tests", "golden", "hnr_bars.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
