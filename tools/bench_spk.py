#!/usr/bin/env python
"""Times the speaker-similarity contractions (fastspeech2_amd/speaker.py, csrc/fs2_spk.hip) on random frames:

    python tools/bench_spk.py [--frames 16384] [--dim 38] [--components 256] [--groups 1 218 2456] [--reps 5]

Prints one JSON line: for fs2_spk_loglik at every G, and for fs2_spk_accum at G = 1, the median time of `--reps` launches after a
warm-up (device events) and the achieved fp64 TFLOP/s, counting 2 N G M 2D for the scores and 2 N M (1 + 2D) for the statistics
(the exp and log of the epilogue are not counted).  The vendor's published peak for the MI355X fp64 matrix path, 78.6 TFLOP/s,
is printed beside them; the microarchitecture notes this project works from state no measured f64 MFMA rate.  An instrument: no
bar is set."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastspeech2_amd import speaker as S  # noqa: E402

PEAK_F64_MATRIX_TF = 78.6


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


def main(args):
    dev = torch.device("cuda")
    N, D, M = args.frames, args.dim, args.components
    gen = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(N, D, dtype=torch.float64, generator=gen).to(dev)
    out = {"frames": N, "dim": D, "components": M, "peak_f64_matrix_tflops_published": PEAK_F64_MATRIX_TF, "loglik": {}}
    for G in args.groups:
        mu, var = torch.randn(G * M, D, dtype=torch.float64, generator=gen), 0.5 + torch.rand(G * M, D, dtype=torch.float64, generator=gen)
        a, b = (mu / var).to(dev), (-0.5 / var).to(dev)
        c = (-0.5 * (torch.log(2 * np.pi * var) + mu * mu / var).sum(1) - np.log(M)).to(dev)
        lse = torch.empty(N, G, dtype=torch.float64, device=dev)
        s = timed(lambda: S.loglik(x, a, b, c, G, out=lse), args.reps)
        out["loglik"][str(G)] = {"seconds": s, "tflops": 2.0 * N * G * M * 2 * D / s * 1e-12}
        if G == 1:
            post = torch.empty(N, M, dtype=torch.float64, device=dev)
            s = timed(lambda: S.loglik(x, a, b, c, 1, post=post, out=lse), args.reps)
            out["loglik_with_posteriors"] = {"seconds": s, "tflops": 4.0 * N * M * 2 * D / s * 1e-12}
            stats = torch.zeros(M, 1 + 2 * D, dtype=torch.float64, device=dev)
            ws = torch.empty(max(S.accum_ws(N, D, M), 1), dtype=torch.float64, device=dev)
            s = timed(lambda: S.accumulate(post, x, stats, ws), args.reps)
            out["accum"] = {"seconds": s, "tflops": 2.0 * N * M * (1 + 2 * D) / s * 1e-12}
        del a, b, c, lse
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=38)
    ap.add_argument("--components", type=int, default=256)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 218, 2456])
    ap.add_argument("--reps", type=int, default=5)
    main(ap.parse_args())
