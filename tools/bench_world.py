"""Cost of `metrics.score_pairs(cepstra="world")` on the LJSpeech-shaped ragged batch of tools/bench_metrics.py (256 pairs, the same
frame-count mix): each side a harmonic tone with vibrato plus noise, hop 256 at 22050 Hz.  One JSON line from one run on one box:

  gpu       ms of one `score_pairs` pass (device events, best of `--repeat`), and of the envelope + mel-cepstra launches alone on the
            batch's reference side; this box's HBM copy rate from fs2_hbm_calibrate in the same run
  host      the numpy oracle tests/world_ref.py (envelope + mel-cepstra) for `--host_rows` of the same utterances over a pool of
            `--threads` processes (16 at most), scaled to the batch by frames

Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_world.py` for the per-kernel table.  No threshold: the numbers
go to DESIGN.md."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS, HOP = 22050, 256


def voice(frames, rng):
    n = (frames - 1) * HOP + rng.randint(1, HOP)
    f0 = rng.uniform(90.0, 260.0) * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * np.arange(n) / FS))
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = sum(np.sin(k * ph) / k for k in range(1, 9)) * 0.2 + 0.01 * rng.randn(n)
    return x.astype(np.float32)


def _host_row(x):
    from tests import world_ref as W
    F = 1 + int(len(x) / FS / (HOP / FS))
    W.world_cepstra(x, np.full(F, 150.0), FS, HOP / FS * 1000)
    return F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host_rows", type=int, default=16)
    args = ap.parse_args()
    from tools.bench_metrics import make_batch
    rng = np.random.RandomState(1)
    shape = [(len(p[0]), len(p[1])) for p in make_batch(args.pairs)]
    refs, syns = [voice(a, rng) for a, _ in shape], [voice(b, rng) for _, b in shape]
    frames = sum(a + b for a, b in shape)

    pick = np.linspace(0, len(refs) - 1, min(args.host_rows, len(refs))).astype(int)
    with ProcessPoolExecutor(max_workers=min(args.threads, 16)) as pool:              # forks before this process touches the GPU
        t0 = time.perf_counter()
        done = sum(pool.map(_host_row, [refs[i] for i in pick]))
        t_host = (time.perf_counter() - t0) * frames / done

    import torch
    from fastspeech2_amd import _lib, envelope as E, metrics as M, ops, pitch as Pitch
    dev = torch.device("cuda:0")
    src = torch.empty(1 << 30, device=dev, dtype=torch.uint8).fill_(3)
    dst = torch.empty_like(src)

    def timed(fn):
        ts = []
        for _ in range(args.repeat + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return min(ts[1:]), out
    t_cal, _ = timed(lambda: _lib.call("fs2_hbm_calibrate", src.data_ptr(), dst.data_ptr(), src.numel(), ops._stream()))
    del src, dst
    t_pass, rows = timed(lambda: M.score_pairs(refs, syns, None, FS, HOP, device=dev, cepstra="world", budget=16 << 30))
    st = __import__("fastspeech2_amd.ragged", fromlist=["Staging"]).Staging()
    st.pack(refs)
    y, lens = st.to(dev), [len(w) for w in refs]
    f0, _, fr = Pitch.dio(y, lens, FS, HOP / FS * 1000)
    f0 = Pitch.stonemask(y, lens, f0, fr, FS, HOP / FS * 1000)
    fr = [min(a, int(b)) for (a, _), b in zip(shape, fr)]
    t_env, env = timed(lambda: E.envelope(y, lens, f0, fr, FS, HOP / FS * 1000))
    t_mc, _ = timed(lambda: E.mel_cepstra(env, fr, 1024, 0.455))
    print(json.dumps({"bench": "world", "device": torch.cuda.get_device_name(0), "pairs": len(shape), "frames_both_sides": frames,
                      "frames_ref_side": sum(fr), "score_pairs_ms": round(t_pass, 2), "envelope_ref_side_ms": round(t_env, 3),
                      "mel_cepstra_ref_side_ms": round(t_mc, 3), "us_per_frame_envelope": round(t_env * 1e3 / sum(fr), 4),
                      "mcd_db_mean": round(float(np.mean([r["mcd_db"] for r in rows])), 3),
                      "hbm_copy_tb_per_s": round(2 * (1 << 30) / (t_cal * 1e-3) / 1e12, 3), "host_threads": min(args.threads, 16),
                      "host_rows_run": len(pick), "host_seconds_for_the_batch": round(t_host, 1)}), flush=True)


if __name__ == "__main__":
    main()
