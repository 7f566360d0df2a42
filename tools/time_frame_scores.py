"""Times fs2_align_frame_scores alone on the GPU (the hot kernel of the aligner's confidence scores, csrc/fs2_align_score.hip) at
N = 65 536 frames for the two table shapes DESIGN.md section 3 records: (C = 160, M = 1, D = 160), monophone states on the raw
features, and (C = 2000, M = 4, D = 40), tied triphone leaves with mixtures after LDA.

    python tools/time_frame_scores.py [--frames 65536] [--warmup 3] [--repeats 10]

Each shape is warmed up, then timed `repeats` times with device events around `inner` back-to-back calls (the preparation kernel
included); the line reports the median time of one call and the spread, the fp64 operations the direct form needs (3 N C M D: a subtraction, a multiplication and
a fused multiply-add per frame, component and dimension, counted as 4 flop) over the median, and that rate as a share of the
MI355X's 78.6 TFLOP/s fp64 vector peak.  A measurement needs the GPU: without one the script fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastspeech2_amd import align as A  # noqa: E402

PEAK_FP64_VECTOR = 78.6e12
SHAPES = ((160, 1, 160), (2000, 4, 40))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=64, help="utterances the frames are split into")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="calls inside one timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_frame_scores.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    B, T = args.batch, args.frames // args.batch
    for C, M, D in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(C)
        w = torch.rand(C, M, generator=g, dtype=torch.float64) + 0.1
        w = (w / w.sum(1, keepdim=True)).to(dev)
        mu = torch.randn(C, M, D, generator=g, dtype=torch.float64).to(dev)
        var = (torch.rand(C, M, D, generator=g, dtype=torch.float64) + 0.5).to(dev)
        f = torch.randn(B, T, D, generator=g, dtype=torch.float64).to(dev)
        cls = torch.randint(0, C, (B, T), generator=g, dtype=torch.int32).to(dev)
        lens = [T] * B
        out = (torch.empty(B, T, dtype=torch.float64, device=dev), torch.empty(B, T, dtype=torch.float64, device=dev),
               torch.empty(B, T, dtype=torch.int32, device=dev))
        for _ in range(args.warmup):
            A.frame_scores(f, lens, cls, w, mu, var, out=out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                A.frame_scores(f, lens, cls, w, mu, var, out=out)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / args.inner)
        med = float(np.median(ms))
        flop = 4.0 * B * T * C * M * D
        print(json.dumps({"kernel": "fs2_align_frame_scores", "frames": B * T, "C": C, "M": M, "D": D, "ms_median": round(med, 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "tflops": round(flop / med / 1e9, 3),
                          "share_of_fp64_vector_peak": round(flop / (med * 1e-3) / PEAK_FP64_VECTOR, 4)}))
