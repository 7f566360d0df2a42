"""Throughput of GPU F0 extraction (fastspeech2_amd.pitch.dio_stonemask) on one hour of synthetic speech-like audio, in
ragged batches packed as the preprocessor packs them (longest first, batch_seconds=1800), and of one build_from_path pass
with pitch="gpu" over a generated raw corpus.  Prints one JSON line per measurement.

FLOP count (fp64, counted from shapes, not measured): per row of N samples
  low-cut      2 (2R + 1) (N + 1 + 4 h_0)             R = round(fs / 50)
  band FIRs    2 passes x sum_j 2 (4 h_j) (N + 1)      (count pass + emit pass recompute the band signal)
  StoneMask    per frame with f0 > 0: (2 + 6) bins x (2 hw + 1) x 8   (4 FMAs per sample and bin; sincos and windows not counted)
Peak: 78.6 TFLOP/s fp64 vector, the MI355X datasheet figure (not measured here).
There is no CPU pyworld baseline on this image; the numpy oracle (tests/f0_ref.py) is a test oracle, not a baseline."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastspeech2_amd import pitch  # noqa: E402

FS, HOP = 22050, 256
PEAK_FP64 = 78.6e12


def utterances(total_seconds, seed=0):
    """speech-like rows: 1.5-10 s, voiced stretches with gliding F0 (90-300 Hz, 8 harmonics) between noise and pauses"""
    rng = np.random.RandomState(seed)
    out, acc = [], 0.0
    while acc < total_seconds:
        n = int(rng.uniform(1.5, 10.0) * FS)
        t = np.arange(n) / FS
        f = rng.uniform(90, 300) * np.exp(0.25 * np.sin(2 * np.pi * rng.uniform(0.2, 2.0) * t + rng.uniform(0, 6)))
        ph = 2 * np.pi * np.cumsum(f) / FS
        x = sum(np.sin(k * ph) / k for k in range(1, 9)) * 0.2
        gate = (np.sin(2 * np.pi * rng.uniform(1.0, 4.0) * t + rng.uniform(0, 6)) > -0.3).astype(np.float64)
        x = x * gate + 0.01 * rng.randn(n)
        out.append(x.astype(np.float32))
        acc += n / FS
    return out


def batches(wavs, batch_seconds):
    order = sorted(range(len(wavs)), key=lambda i: -len(wavs[i]))
    cap, cur, longest = int(batch_seconds * FS), [], 0
    for i in order:
        n = len(wavs[i])
        if cur and (len(cur) + 1) * max(longest, n) > cap:
            yield cur
            cur, longest = [], 0
        cur.append(i)
        longest = max(longest, n)
    if cur:
        yield cur


def flops(lens, f0, frames):
    R = pitch.matlab_round(FS / 50.0)
    hs = [pitch.matlab_round(FS / b / 2.0) for b in pitch.bands()]
    total = 0.0
    for n in lens:
        total += 2 * (2 * R + 1) * (n + 1 + 4 * hs[0]) + 2 * sum(2 * 4 * h * (n + 1) for h in hs)
    v = f0[f0 > 0]
    total += float(np.sum(8 * (2 * (1.5 * FS / v + 1).astype(np.int64) + 1) * 8))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--batch_seconds", type=float, default=1800.0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--corpus", action="store_true", help="also time build_from_path(pitch='gpu') on a generated raw corpus")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0 needs the GPU")
    dev = torch.device("cuda:0")
    fp = HOP / FS * 1000
    wavs = utterances(args.seconds)
    plan = list(batches(wavs, args.batch_seconds))
    dev_batches = []
    for bt in plan:
        lens = [len(wavs[i]) for i in bt]
        y = torch.zeros(len(bt), max(lens))
        for r, i in enumerate(bt):
            y[r, :lens[r]] = torch.from_numpy(wavs[i])
        dev_batches.append((y.to(dev), lens))
    f0s = [pitch.dio_stonemask(y, lens, FS, fp) for y, lens in dev_batches]            # warm-up: every shape once
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        for y, lens in dev_batches:
            pitch.dio_stonemask(y, lens, FS, fp)                                       # ends in a D2H copy (synchronising)
        times.append(time.perf_counter() - t0)
    sec = min(times)
    audio = sum(len(w) for w in wavs) / FS
    fl = sum(flops(lens, f0[0], f0[2]) for (_, lens), f0 in zip(dev_batches, f0s))
    voiced = np.mean(np.concatenate([f[0][b, :f[2][b]] for f in f0s for b in range(len(f[2]))]) > 0)
    print(json.dumps({"bench": "dio_stonemask", "audio_seconds": round(audio, 1), "batches": len(plan), "rows": len(wavs),
                      "seconds": round(sec, 4), "runs_seconds": [round(t, 4) for t in times],
                      "audio_seconds_per_second": round(audio / sec, 1), "voiced_fraction": round(float(voiced), 3),
                      "fp64_flop": fl, "fp64_tflops": round(fl / sec / 1e12, 3),
                      "fraction_of_fp64_vector_peak": round(fl / sec / PEAK_FP64, 4),
                      "peak_source": "MI355X datasheet 78.6 TFLOP/s fp64 vector (not measured)"}), flush=True)
    if args.corpus:
        corpus(dev)


def corpus(dev):
    """build_from_path with pitch="gpu" on a generated raw corpus (2 speakers x 40 utterances), split into host and device time"""
    from scipy.io import wavfile
    from fastspeech2_amd import preprocess as P
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    root = tempfile.mkdtemp()
    wavs = utterances(600.0, seed=1)
    raw, pre = os.path.join(root, "raw"), os.path.join(root, "pre")
    for k, w in enumerate(wavs):
        spk = "s%d" % (k % 2)
        os.makedirs(os.path.join(raw, spk), exist_ok=True)
        os.makedirs(os.path.join(pre, "TextGrid", spk), exist_ok=True)
        wavfile.write(os.path.join(raw, spk, "u%d.wav" % k), FS, (np.clip(w, -1, 1) * 32767).astype(np.int16))
        with open(os.path.join(raw, spk, "u%d.lab" % k), "w") as f:
            f.write("text\n")
        dur = len(w) / FS
        cuts = np.linspace(0.0, dur, 12)
        with open(os.path.join(pre, "TextGrid", spk, "u%d.TextGrid" % k), "w") as f:
            f.write('File type = "ooTextFile"\nObject class = "TextGrid"\n\nxmin = 0\nxmax = %r\ntiers? <exists>\nsize = 1\n'
                    'item []:\n    item [1]:\n        class = "IntervalTier"\n        name = "phones"\n        xmin = 0\n'
                    '        xmax = %r\n        intervals: size = %d\n' % (dur, dur, len(cuts) - 1))
            for j in range(len(cuts) - 1):
                f.write('        intervals [%d]:\n            xmin = %r\n            xmax = %r\n            text = "AH0"\n'
                        % (j + 1, float(cuts[j]), float(cuts[j + 1])))
    cfg = {"dataset": "Bench", "path": {"raw_path": raw, "preprocessed_path": pre},
           "preprocessing": {"val_size": 2, "text": {"text_cleaners": ["english_cleaners"], "language": "en"},
                             "audio": {"sampling_rate": FS, "max_wav_value": 32768.0},
                             "stft": {"filter_length": 1024, "hop_length": HOP, "win_length": 1024},
                             "mel": {"n_mel_channels": 80, "mel_fmin": 0, "mel_fmax": 8000},
                             "pitch": {"feature": "phoneme_level", "normalization": True},
                             "energy": {"feature": "phoneme_level", "normalization": True}}}
    prep = P.Preprocessor(cfg, device=dev, seed=0, pitch="gpu")
    t_pitch, t_mel = [0.0], [0.0]
    real_p, real_m = prep._extract_pitch, prep._extract_mels

    def timed(fn, acc):
        def w(wavs):
            t0 = time.perf_counter()
            r = fn(wavs)
            acc[0] += time.perf_counter() - t0
            return r
        return w
    prep._extract_pitch, prep._extract_mels = timed(real_p, t_pitch), timed(real_m, t_mel)
    t0 = time.perf_counter()
    prep.build_from_path()
    total = time.perf_counter() - t0
    print(json.dumps({"bench": "build_from_path_pitch_gpu", "audio_seconds": round(sum(len(w) for w in wavs) / FS, 1),
                      "utterances": len(wavs), "seconds": round(total, 3), "f0_seconds": round(t_pitch[0], 3),
                      "mel_seconds": round(t_mel[0], 3), "f0_fraction": round(t_pitch[0] / total, 4),
                      "stats_pitch": json.load(open(os.path.join(pre, "stats.json")))["pitch"]}), flush=True)


if __name__ == "__main__":
    main()
