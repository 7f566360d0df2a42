#!/usr/bin/env python
"""Times STOI / ESTOI (fastspeech2_amd/stoi.py) on synthetic time-aligned pairs (tests/stoi_ref.py's signals):

    python tools/bench_stoi.py [--pairs 64] [--seconds 6] [--sr 22050] [--repeat 5] [--ref_pairs 2]

Prints one JSON line: milliseconds of `measure` over a resident ragged batch (resampling to 10 kHz included; best of `--repeat`),
audio seconds scored per second, and the numpy restatement's time on the first `--ref_pairs` pairs (fed scipy's resample_poly).
An instrument: no bar is set."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastspeech2_amd import resample, stoi  # noqa: E402
from tests import stoi_ref  # noqa: E402


def main(args):
    rng = np.random.default_rng(0)
    lengths = [int(args.sr * args.seconds * f) for f in rng.uniform(0.5, 1.0, args.pairs)]
    pairs = stoi_ref.pairs_22k(lengths, seed=1) if args.sr == 22050 else stoi_ref.pairs(lengths, seed=1)
    dev = torch.device("cuda")
    N = max(lengths)
    x, y = (torch.zeros(len(pairs), N, device=dev) for _ in range(2))
    for b, (a, c) in enumerate(pairs):
        x[b, :len(a)], y[b, :len(c)] = torch.from_numpy(a).to(dev), torch.from_numpy(c).to(dev)
    out = stoi.measure(x, lengths, y, lengths, args.sr)                    # tables to the device, first launches
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        out = stoi.measure(x, lengths, y, lengths, args.sr)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    up, down = resample.ratio(args.sr, stoi.FS)
    from scipy.signal import resample_poly
    t0 = time.perf_counter()
    for a, c in pairs[:args.ref_pairs]:
        stoi_ref.chain(resample_poly(a.astype(np.float64), up, down), resample_poly(c.astype(np.float64), up, down))
    ref_s = time.perf_counter() - t0
    audio = sum(lengths) / args.sr
    print(json.dumps({"pairs": len(pairs), "sr": args.sr, "audio_seconds": round(audio, 1), "measure_ms": round(best * 1e3, 3),
                      "audio_seconds_per_second": round(audio / best, 1), "stoi_mean": float(out["stoi"].nanmean()),
                      "estoi_mean": float(out["estoi"].nanmean()), "too_short": int(out["too_short"].sum()),
                      "reference_pairs": min(args.ref_pairs, len(pairs)),
                      "reference_audio_seconds_per_second": round(sum(lengths[:args.ref_pairs]) / args.sr / ref_s, 1)}))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=64)
    parser.add_argument("--seconds", type=float, default=6.0)
    parser.add_argument("--sr", type=int, default=22050)
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--ref_pairs", type=int, default=2)
    main(parser.parse_args())
