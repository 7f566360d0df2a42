"""`python loudness.py DIR_OR_WAV... [--true_peak] [--out FILE]` — integrated loudness (ITU-R BS.1770-4) of wav files that exist
already: a `raw_path`, a `result_path` of synthesized audio.  Files are read as mono float32 at their own rate by a host thread pool,
grouped by rate into ragged batches and measured on the GPU (fastspeech2_amd/loudness.py).  One JSON object per file (`wav`, `fs` and
the keys of `loudness.measure`) goes to stdout or `--out`, then one summary line."""
import argparse
import json
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def find_wavs(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += sorted(os.path.join(d, f) for d, _, fs in os.walk(p) for f in fs if f.lower().endswith(".wav"))
        else:
            out.append(p)
    return out


def measure_files(paths, device="cuda", true_peak=False, batch_seconds=1500.0, num_workers=8):
    """[wav paths] -> [dict per file], in the order given"""
    from fastspeech2_amd import loudness as L, ragged
    from fastspeech2_amd.preprocess import load_wav
    device = ragged.require_device(torch.device(device), "loudness.py")
    with ThreadPoolExecutor(max_workers=max(1, num_workers)) as pool:
        loaded = list(pool.map(lambda p: load_wav(p, resample=False), paths))
    staging, rows = ragged.Staging(), [None] * len(paths)
    for sr, ks in ragged.keyed_batches([sr for _, sr in loaded], [(len(w),) for w, _ in loaded], lambda sr: int(batch_seconds * sr),
                                       ragged.padded_samples):
        staging.pack([loaded[k][0] for k in ks])
        for k, m in zip(ks, L.measure(staging.to(device), [len(loaded[k][0]) for k in ks], sr, true_peak=true_peak)):
            rows[k] = dict(wav=paths[k], fs=int(sr), **{key: (v if not isinstance(v, float) or math.isfinite(v) else None)
                                                        for key, v in m.items()})
    return rows


def summary(rows):
    v = np.array([r["lufs"] for r in rows if r["lufs"] is not None], dtype=np.float64)
    s = {"files": len(rows), "measured": len(v)}
    if len(v):
        s.update(lufs_mean=float(v.mean()), lufs_std=float(v.std()), lufs_min=float(v.min()), lufs_max=float(v.max()))
    return s


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("paths", nargs="+", help="wav files, or directories searched for *.wav")
    parser.add_argument("--true_peak", action="store_true",
                        help="also report the peak of the x 4 oversampled signal (this project's resampler, not BS.1770 Annex 2's filter)")
    parser.add_argument("--out", type=str, default=None, help="write the rows to this file instead of stdout")
    parser.add_argument("--batch_seconds", type=float, default=1500.0, help="audio per ragged batch on the GPU")
    parser.add_argument("--num_workers", type=int, default=8, help="host threads reading wav files")
    args = parser.parse_args()

    rows = measure_files(find_wavs(args.paths), true_peak=args.true_peak, batch_seconds=args.batch_seconds, num_workers=args.num_workers)
    f = open(args.out, "w") if args.out else sys.stdout
    for r in rows:
        f.write(json.dumps(r) + "\n")
    if args.out:
        f.close()
    print(json.dumps({"summary": summary(rows)}))
