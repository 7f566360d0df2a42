"""Cost of the scoring kernels (fastspeech2_amd.metrics, csrc/fs2_dtw.hip) on one LJSpeech-shaped ragged batch: 256 pairs whose
reference frame counts follow the phone counts of fastspeech2_amd/workloads/ljspeech_val_phonemes.json (4-12 frames per phone, as
tools/bench_align.py draws them), the synthesized side 0.9-1.1 times as long, cepstra of a random walk and a warped noisy copy.
One JSON line, all from one run on one box:

  kernels   ms per kernel (mcep of both sides, cost, scan, backtrack, f0), device events around each launch, best of `--repeat`;
            per kernel the bytes it must move as a fraction of this box's HBM copy rate (measured in the same run with
            fs2_hbm_calibrate); for the scan and the backtrack the time per anti-diagonal / per path cell of the longest pair
  host      the same pairs (local cost, DTW, backtrack, F0 sums) with the numpy oracle tests/dtw_ref.py over a pool of `--threads`
            processes (16 at most)

  prosody   with `--prosody` also the kernels that switch adds: the path sums (fs2_dtw_prosody), the compaction and moments of both
            sides (fs2_prosody_voiced) and the pitch-contour DTW (cost, scan and backtrack with K = 1 on the voiced frames, with the
            D2H copy of the voiced counts it waits for), and their sum `prosody_ms` next to `batch_ms`

There is no earlier implementation to compare with and no threshold: the numbers go to DESIGN.md."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N_MEL = 13, 80


def make_batch(n_pairs, seed=0):
    with open(os.path.join(ROOT, "fastspeech2_amd", "workloads", "ljspeech_val_phonemes.json")) as f:
        counts = json.load(f)["counts"][:n_pairs]
    rng = np.random.RandomState(seed)
    pairs = []
    for n in counts:
        T1 = int(sum(rng.randint(4, 13) for _ in range(n)) + rng.randint(0, 17))
        T2 = max(1, int(round(T1 * rng.uniform(0.9, 1.1))))
        base = np.cumsum(rng.randn(max(T1, T2) + 8, K), axis=0) * 0.3
        a = base[np.sort(rng.randint(0, len(base), T1))] + 0.05 * rng.randn(T1, K)
        b = base[np.sort(rng.randint(0, len(base), T2))] + 0.05 * rng.randn(T2, K)
        f0a = np.where(np.repeat(rng.rand(T1 // 5 + 1) < 0.7, 5)[:T1], 120.0 * 2.0 ** rng.uniform(-0.5, 1.0, T1), 0.0)
        f0b = np.where(np.repeat(rng.rand(T2 // 5 + 1) < 0.7, 5)[:T2], 120.0 * 2.0 ** rng.uniform(-0.5, 1.0, T2), 0.0)
        pairs.append((a, b, f0a, f0b))
    pairs.sort(key=lambda p: (-len(p[0]), -len(p[1])))
    return pairs


def _host_pair(p):
    from tests import dtw_ref as R
    a, b, f0a, f0b = p
    total, pi, pj = R.dtw(a, b)
    R.f0_sums(pi, pj, f0a, f0b)
    return total, len(pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host_pairs", type=int, default=256, help="pairs the host oracle runs (scaled to the batch)")
    ap.add_argument("--prosody", action="store_true", help="also time what score.py --prosody adds")
    args = ap.parse_args()
    pairs = make_batch(args.pairs)
    al, bl = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]

    # host first: the pool forks before this process touches the GPU
    n_host = min(args.host_pairs, len(pairs))
    pick = np.linspace(0, len(pairs) - 1, n_host).astype(int)
    with ProcessPoolExecutor(max_workers=min(args.threads, 16)) as pool:
        t0 = time.perf_counter()
        host = list(pool.map(_host_pair, [pairs[i] for i in pick]))
        t_host = (time.perf_counter() - t0) * len(pairs) / n_host

    import torch
    from fastspeech2_amd import _lib, metrics as M, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the GPU")
    dev = torch.device("cuda:0")
    src = torch.empty(1 << 30, device=dev, dtype=torch.uint8).fill_(3)
    dst = torch.empty_like(src)

    def timed(fn):
        ts, out = [], None
        for _ in range(args.repeat + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return min(ts[1:]), out
    t_cal, _ = timed(lambda: _lib.call("fs2_hbm_calibrate", src.data_ptr(), dst.data_ptr(), src.numel(), ops._stream()))
    hbm = 2 * src.numel() / (t_cal * 1e-3)
    del src, dst

    def pack(rows, T, width=None):
        out = torch.zeros((len(rows), T) + ((width,) if width else ()), dtype=torch.float64)
        for r, v in enumerate(rows):
            out[r, :len(v)] = torch.from_numpy(v)
        return out.to(dev)
    B, T1, T2 = len(pairs), max(al), max(bl)
    a, b = pack([p[0] for p in pairs], T1, K), pack([p[1] for p in pairs], T2, K)
    f0a, f0b = pack([p[2] for p in pairs], T1), pack([p[3] for p in pairs], T2)
    mel_a = torch.randn(B, N_MEL, T1, device=dev) * 2 - 5
    mel_b = torch.randn(B, N_MEL, T2, device=dev) * 2 - 5
    ms = {}
    ms["mcep"], _ = timed(lambda: (M.cepstra(mel_a, al), M.cepstra(mel_b, bl)))
    cost = torch.empty(B, T2, T1, dtype=torch.float64, device=dev)
    bp = torch.empty(B, T2, T1, dtype=torch.uint8, device=dev)
    ms["cost"], _ = timed(lambda: M.local_cost(a, al, b, bl, out=cost))
    ms["scan"], (_, total) = timed(lambda: M.scan(cost, al, bl, out=bp))
    ms["backtrack"], (plen, pi, pj) = timed(lambda: M.backtrack(bp, al, bl))
    ms["f0"], sums = timed(lambda: M.f0_on_path(pi, pj, plen, f0a, al, f0b, bl))
    extra = {}
    if args.prosody:
        ea, eb = torch.rand(B, T1, device=dev) * 40, torch.rand(B, T2, device=dev) * 40
        pms = {}
        pms["path_sums"], _ = timed(lambda: M.prosody_on_path(pi, pj, plen, f0a, al, f0b, bl, ea, eb))
        pms["voiced"], ((u, nu, _), (w, nw, _)) = timed(lambda: (M.voiced_contours(f0a, al), M.voiced_contours(f0b, bl)))
        pms["contour_dtw"], (_, cplen, _, _, launched) = timed(lambda: M.contour_dtw(u, nu.cpu(), w, nw.cpu()))
        nu, nw = nu.cpu().numpy(), nw.cpu().numpy()
        extra = {"prosody_ms_each": {k: round(v, 4) for k, v in pms.items()}, "prosody_ms": round(sum(pms.values()), 3),
                 "contour_pairs": len(launched), "contour_cells": int((nu.astype(np.int64) * nw).sum()),
                 "contour_path_len_max": int(cplen.max())}
    total, plen, sums = total.cpu().numpy(), plen.cpu().numpy(), sums.cpu().numpy()
    for k, i in enumerate(pick):                                             # the oracle's answers for the pairs it ran
        assert abs(total[i] - host[k][0]) <= 1e-6 * host[k][0] and plen[i] == host[k][1], (i, total[i], plen[i], host[k])

    cells = sum(x * y for x, y in zip(al, bl))
    frames = sum(al) + sum(bl)
    need = {"mcep": 4 * N_MEL * frames + 8 * K * frames, "cost": 8 * K * frames + 8 * cells, "scan": 9 * cells,
            "backtrack": int(plen.sum()) * 9, "f0": int(plen.sum()) * 24}
    t_all = sum(ms.values())
    steps = max(x + y - 1 for x, y in zip(al, bl))
    lanes = 256 if T1 <= 256 else 512 if T1 <= 512 else 1024
    print(json.dumps({
        "bench": "metrics", "device": torch.cuda.get_device_name(0), "pairs": B, "frames_ref_max": T1, "frames_syn_max": T2,
        "frames_ref_mean": round(float(np.mean(al)), 1), "frames_syn_mean": round(float(np.mean(bl)), 1), "n_mcep": K,
        "cells": cells, "path_len_max": int(plen.max()), "anti_diagonals_max": steps, "scan_lanes": lanes,
        "scan_rows_per_lane": 2 if T1 > 1024 else 1,
        "ms": {k: round(v, 4) for k, v in ms.items()}, "batch_ms": round(t_all, 3), "pairs_per_s": round(B / t_all * 1e3, 0),
        "hbm_copy_tb_per_s": round(hbm / 1e12, 3),
        "fraction_of_hbm_copy": {k: round(need[k] / (ms[k] * 1e-3) / hbm, 4) for k in ms},
        "us_per_anti_diagonal": round(ms["scan"] * 1e3 / steps, 4),
        "us_per_path_cell": round(ms["backtrack"] * 1e3 / int(plen.max()), 4),
        "host_threads": min(args.threads, 16), "host_pairs_run": n_host, "host_seconds": round(t_host, 3),
        "host_pairs_per_s": round(B / t_host, 1),
        "gpu_dtw_ms": round(ms["cost"] + ms["scan"] + ms["backtrack"] + ms["f0"], 3),
        "speedup_over_host": round(t_host * 1e3 / (ms["cost"] + ms["scan"] + ms["backtrack"] + ms["f0"]), 1), **extra}), flush=True)


if __name__ == "__main__":
    main()
