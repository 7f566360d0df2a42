#!/usr/bin/env python
"""Times the wavelet prosody scores (fastspeech2_amd/cwt.py) at one shape: 32 pairs of about 800 frames, synthetic tracks:

    python tools/bench_cwt.py [--pairs 32] [--frames 800] [--warmup 3] [--windows 7] [--iters 5]

Prints one JSON line: ms per launch of the three kernels (fs2_cwt_contour and fs2_cwt_transform on the 2 x 32 rows of both sides,
fs2_cwt_on_path on the 32 paths of `metrics.dtw` over random cepstra) and ms per `metrics.score_pairs` batch of 32
tone-sequence pairs with and without `wavelet`.  HIP events around windows of back-to-back calls after a warm-up, the median over
the windows with their minimum and maximum.  An instrument: no bar is set.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastspeech2_amd import audio, cwt, metrics  # noqa: E402
from tests import cwt_ref, f0_signals  # noqa: E402


def timed(fn, warmup, windows, iters):
    """(median, min, max) ms per call over `windows` windows of `iters` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return [round(v, 4) for v in (statistics.median(ms), min(ms), max(ms))]


def tones(rng, frames):
    """a sequence of harmonic tones with short silences, `frames` hops long"""
    parts, n = [], 0
    while n < frames * f0_signals.HOP:
        parts.append(f0_signals.tone(float(rng.uniform(90, 330)), float(rng.uniform(0.15, 0.5))))
        parts.append(np.zeros(int(rng.uniform(0.02, 0.12) * f0_signals.FS), np.float32))
        n += len(parts[-2]) + len(parts[-1])
    return np.concatenate(parts)[:frames * f0_signals.HOP]


def main(args):
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    sr, hop, B = f0_signals.FS, f0_signals.HOP, args.pairs
    lens = [int(v) for v in rng.integers(args.frames - 100, args.frames + 101, 2 * B)]
    f0 = torch.zeros(2 * B, max(lens), dtype=torch.float64, device=dev)
    for b, T in enumerate(lens):
        f0[b, :T] = torch.from_numpy(cwt_ref.track(rng, T, "runs"))
    z, _ = cwt.contour(f0, lens)
    W, _ = cwt.transform(z, lens, sr, hop)
    al, bl = lens[:B], lens[B:]
    a = torch.from_numpy(rng.standard_normal((B, max(al), 13)).cumsum(axis=1)).to(dev)
    b = torch.from_numpy(rng.standard_normal((B, max(bl), 13)).cumsum(axis=1)).to(dev)
    _, plen, pi, pj = metrics.dtw(a, al, b, bl)
    Wa, Wb = W[:B, :, :max(al)], W[B:, :, :max(bl)]
    t = lambda fn: timed(fn, args.warmup, args.windows, args.iters)         # noqa: E731
    out = {"pairs": B, "frames_mean": round(float(np.mean(lens)), 1), "path_len_mean": round(float(plen.double().mean()), 1),
           "contour_ms": t(lambda: cwt.contour(f0, lens, out=z)), "transform_ms": t(lambda: cwt.transform(z, lens, sr, hop, out=W)),
           "on_path_ms": t(lambda: cwt.on_path(pi, pj, plen, Wa, al, Wb, bl))}
    stft = audio.TacotronSTFT(1024, hop, 1024, 80, sr, 0, 8000)
    refs, syns = [tones(rng, T) for T in al], [tones(rng, T) for T in bl]
    for key, flag in (("score_pairs_ms", False), ("score_pairs_wavelet_ms", True)):
        out[key] = timed(lambda: metrics.score_pairs(refs, syns, stft, sr, hop, device=dev, wavelet=flag), 1, args.windows, 1)
    out["ms"] = "median, min, max"
    print(json.dumps(out))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--pairs", type=int, default=32)
    parser.add_argument("--frames", type=int, default=800)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--windows", type=int, default=7)
    parser.add_argument("--iters", type=int, default=5)
    main(parser.parse_args())
