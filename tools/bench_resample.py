"""Throughput of GPU sample-rate conversion (fastspeech2_amd.resample.resample_poly) on one ragged batch of 25 minutes of audio, packed
as prepare_align packs it (longest first), at 24 000 -> 22 050 Hz and 44 100 -> 22 050 Hz.  One JSON line per rate pair, all from one
run on one box:

  (a) resident     the batch already on the device: output samples / s, and bytes moved (float32 input read once + float32 output
                   written once; the L2-resident tap table not counted) / time against this box's HBM copy rate, measured in the same
                   run with the calibration kernel bench.py --full uses (fs2_hbm_calibrate, 1 GiB read + 1 GiB written)
  (b) with copies  pinned host batch -> H2D -> resample -> D2H of the float32 rows into pinned memory
  (b') product     prepare_align's device stage as it runs: packing into the staging buffer, H2D, resample, peak, normalise + int16
                   cast, D2H, per-row slices
  (c) host         what load_wav does today: scipy.signal.resample_poly on each float32 utterance, over a 16-thread pool

The gate is (b) not slower than (c); the script exits non-zero otherwise."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastspeech2_amd import _lib, ops, resample as R  # noqa: E402
from fastspeech2_amd.prepare_align import _DeviceAudio  # noqa: E402


def utterances(total_seconds, sr, seed=0):
    """rows of 1.5 - 10 s: a few harmonics plus noise (the resampler's cost does not depend on the content)"""
    rng = np.random.RandomState(seed)
    out, acc = [], 0.0
    while acc < total_seconds:
        n = int(rng.uniform(1.5, 10.0) * sr)
        t = np.arange(n) / sr
        f = rng.uniform(90, 300)
        out.append((0.2 * sum(np.sin(2 * np.pi * f * k * t) / k for k in range(1, 5)) + 0.02 * rng.randn(n)).astype(np.float32))
        acc += n / sr
    return sorted(out, key=lambda w: -len(w))


def hbm_copy_rate(dev):
    src = torch.empty(1 << 30, device=dev, dtype=torch.uint8).fill_(3)
    dst = torch.empty_like(src)
    ts = []
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("fs2_hbm_calibrate", src.data_ptr(), dst.data_ptr(), src.numel(), ops._stream())
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return 2 * src.numel() / (sorted(ts[1:])[1] * 1e-3)


def best(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1500.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sr_out", type=int, default=22050)
    ap.add_argument("--sr_in", type=int, nargs="+", default=[24000, 44100])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs the GPU")
    dev = torch.device("cuda:0")
    hbm = hbm_copy_rate(dev)
    ok = True
    for sr_in in args.sr_in:
        wavs = utterances(args.seconds, sr_in)
        lens = [len(w) for w in wavs]
        B, N = len(wavs), max(lens)
        up, down = R.ratio(sr_in, args.sr_out)
        host = torch.zeros(B, N).pin_memory()
        for b, w in enumerate(wavs):
            host[b, :lens[b]] = torch.from_numpy(w)
        x = host.to(dev)
        y, out_lens = R.resample_poly(x, lens, sr_in, args.sr_out)                         # warm-up: tap table, code object
        torch.cuda.synchronize()
        n_out = int(out_lens.sum())
        back = torch.empty(y.shape, dtype=torch.float32).pin_memory()

        # (a) resident, timed with device events around the launch
        ts = []
        for _ in range(args.repeat + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            R.resample_poly(x, lens, sr_in, args.sr_out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        t_a = min(ts[1:])
        moved = 4 * (sum(lens) + n_out)

        # (b) H2D + resample + D2H of the float32 rows
        def with_copies():
            yy, _ = R.resample_poly(host.to(dev, non_blocking=True), lens, sr_in, args.sr_out)
            back.copy_(yy, non_blocking=True)
            torch.cuda.synchronize()
        with_copies()
        t_b, runs_b = best(with_copies, args.repeat)

        # (b') the product's device stage, end to end
        stage = _DeviceAudio(dev)
        stage(wavs, sr_in, args.sr_out, 32768.0)
        t_p, _ = best(lambda: stage(wavs, sr_in, args.sr_out, 32768.0), args.repeat)

        # (c) the host path of load_wav: scipy's polyphase resampler per float32 utterance, thread pool
        from scipy.signal import resample_poly

        def host_path():
            with ThreadPoolExecutor(max_workers=args.threads) as pool:
                return list(pool.map(lambda w: resample_poly(w, up, down).astype(np.float32), wavs))
        ref = host_path()
        t_c, runs_c = best(host_path, args.repeat)

        got = back.numpy()
        worst = max(float(np.abs(got[b, :len(r)] - r).max()) for b, r in enumerate(ref))    # float32-tap scipy vs fp64-tap kernel
        ok = ok and t_b <= t_c
        print(json.dumps({
            "bench": "resample_poly", "device": torch.cuda.get_device_name(0), "sr_in": sr_in, "sr_out": args.sr_out, "up": up,
            "down": down, "audio_seconds": round(sum(lens) / sr_in, 1), "rows": B, "padded_row": N, "output_samples": n_out,
            "a_resident_seconds": round(t_a, 6), "a_output_samples_per_second": round(n_out / t_a, 0),
            "a_bytes_moved": moved, "a_tb_per_s": round(moved / t_a / 1e12, 4), "hbm_copy_tb_per_s": round(hbm / 1e12, 3),
            "a_fraction_of_hbm_copy": round(moved / t_a / hbm, 4),
            "b_with_copies_seconds": round(t_b, 5), "b_runs": [round(t, 5) for t in runs_b],
            "b_output_samples_per_second": round(n_out / t_b, 0),
            "b_product_stage_seconds": round(t_p, 5),
            "c_host_seconds": round(t_c, 5), "c_runs": [round(t, 5) for t in runs_c], "c_threads": args.threads,
            "c_output_samples_per_second": round(n_out / t_c, 0), "b_speedup_over_c": round(t_c / t_b, 2),
            "max_abs_diff_vs_host_float32_path": worst, "gate_b_not_slower_than_c": bool(t_b <= t_c)}), flush=True)
    if not ok:
        raise SystemExit("gate failed: the GPU path with copies is slower than the host path")


if __name__ == "__main__":
    main()
