#!/usr/bin/env python
"""Times the harmonics-to-noise ratio (fastspeech2_amd/hnr.py) at one shape: 32 pairs of about 800 frames of tone sequences:

    python tools/bench_hnr.py [--pairs 32] [--frames 800] [--warmup 3] [--windows 7] [--iters 5]

Prints one JSON line: ms per launch of the three kernels (fs2_hnr_frames and fs2_hnr_side on the 2 x 32 rows of both sides at 22050
Hz, hop 256, with a synthetic F0 track voiced on about two frames in three; fs2_hnr_on_path on the 32 paths of `metrics.dtw` over
random cepstra) and ms per `metrics.score_pairs` batch of the 32 pairs with and without `hnr`.  HIP events around windows of
back-to-back calls after a warm-up, the median over the windows with their minimum and maximum.  An instrument: no bar is set.
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
from fastspeech2_amd import audio, hnr, metrics  # noqa: E402
from tests import f0_signals  # noqa: E402


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
    """a sequence of harmonic tones with short silences, `frames` hops long -> (audio, the true F0 per frame, 0 in the silences)"""
    parts, f0, n = [], [], 0
    while n < frames * f0_signals.HOP:
        f = float(rng.uniform(90, 330))
        parts.append(f0_signals.tone(f, float(rng.uniform(0.15, 0.5))))
        parts.append(np.zeros(int(rng.uniform(0.02, 0.12) * f0_signals.FS), np.float32))
        f0 += [f] * len(parts[-2]) + [0.0] * len(parts[-1])
        n += len(parts[-2]) + len(parts[-1])
    y = np.concatenate(parts)[:frames * f0_signals.HOP]
    y = (y + 0.01 * rng.standard_normal(len(y))).astype(np.float32)
    return y, np.asarray(f0, np.float64)[:len(y):f0_signals.HOP]


def main(args):
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    sr, hop, B = f0_signals.FS, f0_signals.HOP, args.pairs
    frames = [int(v) for v in rng.integers(args.frames - 100, args.frames + 101, 2 * B)]
    sides = [tones(rng, T) for T in frames]
    lens = [len(y) for y, _ in sides]
    y = torch.zeros(2 * B, max(lens), dtype=torch.float32, device=dev)
    f0 = torch.zeros(2 * B, max(frames), dtype=torch.float64, device=dev)
    for b, (w, f) in enumerate(sides):
        y[b, :len(w)], f0[b, :len(f)] = torch.from_numpy(w), torch.from_numpy(f)
    fr, lag = hnr.frames(y, lens, f0, frames, sr, hop)
    stats = hnr.side(fr, frames)
    al, bl = frames[:B], frames[B:]
    a = torch.from_numpy(rng.standard_normal((B, max(al), 13)).cumsum(axis=1)).to(dev)
    b = torch.from_numpy(rng.standard_normal((B, max(bl), 13)).cumsum(axis=1)).to(dev)
    _, plen, pi, pj = metrics.dtw(a, al, b, bl)
    fa, fb = fr[:B, :max(al)], fr[B:, :max(bl)]
    t = lambda fn: timed(fn, args.warmup, args.windows, args.iters)         # noqa: E731
    out = {"pairs": B, "frames_mean": round(float(np.mean(frames)), 1), "valid_frames_mean": round(float(stats[:, 0].mean()), 1),
           "path_len_mean": round(float(plen.double().mean()), 1),
           "frames_ms": t(lambda: hnr.frames(y, lens, f0, frames, sr, hop, out=fr, out_lag=lag)),
           "side_ms": t(lambda: hnr.side(fr, frames, out=stats)), "on_path_ms": t(lambda: hnr.on_path(pi, pj, plen, fa, al, fb, bl))}
    stft = audio.TacotronSTFT(1024, hop, 1024, 80, sr, 0, 8000)
    refs, syns = [s[0] for s in sides[:B]], [s[0] for s in sides[B:]]
    for key, flag in (("score_pairs_ms", False), ("score_pairs_hnr_ms", True)):
        out[key] = timed(lambda: metrics.score_pairs(refs, syns, stft, sr, hop, device=dev, hnr=flag), 1, args.windows, 1)
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
