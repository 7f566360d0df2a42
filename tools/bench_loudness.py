"""Time of the K-weighted block energies (fastspeech2_amd.loudness.block_energy) over one ragged batch of 25 minutes of audio at
22 050 Hz, packed as prepare_align packs it (longest first).  One JSON line: milliseconds per call with the batch resident on the
device, and GB/s of the 4 bytes per sample the measurement must read at least (the kernels read every sample twice and keep 32
bytes of state per 64 samples, so the traffic they cause is higher).  The number to set it beside is the HBM copy rate of the same
box, measured in the same run with the calibration kernel bench.py --full uses.  No bar is set on either."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastspeech2_amd import loudness as L  # noqa: E402
from tools.bench_resample import hbm_copy_rate, utterances  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1500.0)
    ap.add_argument("--fs", type=int, default=22050)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loudness needs the GPU")
    dev = torch.device("cuda:0")
    hbm = hbm_copy_rate(dev)
    wavs = utterances(args.seconds, args.fs)
    lens = [len(w) for w in wavs]
    host = torch.zeros(len(wavs), max(lens))
    for b, w in enumerate(wavs):
        host[b, :lens[b]] = torch.from_numpy(w)
    x = host.to(dev)
    L.block_energy(x, lens, args.fs)                                          # warm-up: tables, code object
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        z, nb = L.block_energy(x, lens, args.fs)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = sorted(ts)[len(ts) // 2]
    loud = L.integrated(z, nb)[:, 0]
    print(json.dumps({
        "bench": "loudness.block_energy", "device": torch.cuda.get_device_name(0), "fs": args.fs, "rows": len(wavs),
        "padded_row": max(lens), "audio_seconds": round(sum(lens) / args.fs, 1), "samples": sum(lens),
        "ms_median": round(ms, 4), "ms_runs": [round(t, 4) for t in ts], "gb_per_s_of_4_bytes_per_sample": round(4 * sum(lens) / ms / 1e6, 1),
        "hbm_copy_gb_per_s": round(hbm / 1e9, 1), "audio_seconds_per_second": round(sum(lens) / args.fs / (ms * 1e-3), 0),
        "lufs_mean": round(float(loud.mean()), 3)}), flush=True)


if __name__ == "__main__":
    main()
