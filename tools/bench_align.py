"""Cost of the forced aligner's kernels (fastspeech2_amd.align, csrc/fs2_align.hip) on one LJSpeech-shaped ragged batch: 256 utterances
with the phone counts of fastspeech2_amd/workloads/ljspeech_val_phonemes.json (one word per four phones, two states per phone, 4-12
frames per phone, 0-8 per silence), features drawn around random class means.  One JSON line, all from one run on one box:

  kernels   ms per kernel of one Baum-Welch pass (emit, forward, backward, stats, reduce) and one decoding pass (emit, viterbi,
            backtrack), device events around each launch, best of `--repeat`; utterances / s of either pass; per kernel the bytes
            it must move and the flops it must do, as fractions of this box's HBM copy rate (measured in the same run with
            fs2_hbm_calibrate) and of the time; per scan the time per frame-step of the longest utterance (the scans are serial in t)
  host      the same two passes with the numpy oracle tests/align_ref.py over a pool of `--threads` processes (16 at most)

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

S, D = 2, 160


def make_batch(n_utt, seed=0):
    from fastspeech2_amd import align as A
    with open(os.path.join(ROOT, "fastspeech2_amd", "workloads", "ljspeech_val_phonemes.json")) as f:
        counts = json.load(f)["counts"][:n_utt]
    rng = np.random.RandomState(seed)
    phones = [f"P{i:02d}" for i in range(70)]
    ids = {p: i for i, p in enumerate(phones + [A.SIL, A.SP, A.SPN])}
    means = rng.randn(len(ids) * S, D)
    graphs, xs = [], []
    for n in counts:
        lex, words = {}, []
        for w in range(-(-n // 4)):
            lex[f"w{w}"] = [phones[k] for k in rng.randint(0, len(phones), min(4, n - 4 * w))]
            words.append(f"w{w}")
        g = A.utterance_graph(words, lex, ids, S)
        path = []
        for k, (p, _, opt) in enumerate(g["blocks"]):
            d = rng.randint(0, 9) if opt else rng.randint(4, 13)
            path += [g["sid"][k * S]] * (d - d // 2) + [g["sid"][k * S + 1]] * (d // 2)
        xs.append(means[path] + rng.randn(len(path), D))
        graphs.append(g)
    order = sorted(range(len(xs)), key=lambda i: -len(xs[i]))
    return [graphs[i] for i in order], [xs[i] for i in order], len(ids) * S


def _host_pass(args):
    from tests import align_ref as R
    x, g, mu, var = args
    E = R.emissions(x, g["sid"], mu, var)
    gamma, _, _ = R.posteriors(E, g)
    R.partials(gamma, x)
    R.viterbi(E, g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host_utterances", type=int, default=256, help="utterances the host oracle runs (scaled to the batch)")
    args = ap.parse_args()
    graphs, xs, n_classes = make_batch(args.utterances)
    lens = [len(x) for x in xs]
    rng = np.random.RandomState(1)
    mu, var = rng.randn(n_classes, D), np.full((n_classes, D), 2.0)

    # host first: the pool forks before this process touches the GPU
    n_host = min(args.host_utterances, len(xs))
    pick = np.linspace(0, len(xs) - 1, n_host).astype(int)
    with ProcessPoolExecutor(max_workers=min(args.threads, 16)) as pool:
        t0 = time.perf_counter()
        list(pool.map(_host_pass, [(xs[i], graphs[i], mu, var) for i in pick]))
        t_host = (time.perf_counter() - t0) * len(xs) / n_host

    import torch
    from fastspeech2_amd import _lib, align as A, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_align needs the GPU")
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

    B, Tmax = len(xs), max(lens)
    G = A.Graphs(graphs, dev)
    x = torch.zeros(B, Tmax, D, dtype=torch.float64)
    for b, v in enumerate(xs):
        x[b, :lens[b]] = torch.from_numpy(v)
    x = x.to(dev)
    mu_d, var_d = torch.from_numpy(mu).to(dev), torch.from_numpy(var).to(dev)
    index = G.index(n_classes, G.ldg)
    ms = {}
    ms["emit"], E = timed(lambda: A.emit(x, lens, G, mu_d, var_d))
    alpha = torch.empty_like(E)
    ms["forward"], (_, loglik) = timed(lambda: A.forward(E, lens, G, out=alpha))
    gamma = torch.empty_like(E)
    ms["backward"], _ = timed(lambda: A.backward(E, lens, G, alpha, loglik, out=gamma))
    ms["stats"], parts = timed(lambda: A.stats(gamma, x, lens, G))
    ms["reduce"], _ = timed(lambda: A.reduce(parts, G, n_classes, index=index))
    ms["viterbi"], (bp, end, _) = timed(lambda: A.viterbi(E, lens, G))
    ms["backtrack"], frames = timed(lambda: A.backtrack(bp, lens, G, end))
    assert bool((frames.sum(dim=1).cpu() == torch.tensor(lens)).all())

    cells = sum(t * j for t, j in zip(lens, G.jl))                          # (frame, state) pairs of the batch
    rows = sum(G.jl)
    need = {                                                                # bytes each kernel must move, flops it must do
        "emit": (8 * (sum(lens) * D + cells), 4 * cells * D), "forward": (16 * cells, 0), "backward": (24 * cells, 0),
        "stats": (8 * (cells + sum(lens) * D + rows * (1 + 2 * D)), 4 * cells * D), "reduce": (8 * rows * (1 + 2 * D), 0),
        "viterbi": (9 * cells, 0), "backtrack": (sum(lens), 0)}
    t_em = sum(ms[k] for k in ("emit", "forward", "backward", "stats", "reduce"))
    t_dec = sum(ms[k] for k in ("emit", "viterbi", "backtrack"))
    print(json.dumps({
        "bench": "align", "device": torch.cuda.get_device_name(0), "utterances": B, "frames_max": Tmax, "frames_mean": round(np.mean(lens), 1),
        "states_max": G.Jmax, "states_mean": round(np.mean(G.jl), 1), "classes": n_classes, "dim": D,
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "em_pass_ms": round(t_em, 3), "em_utterances_per_s": round(B / t_em * 1e3, 0),
        "decode_pass_ms": round(t_dec, 3), "decode_utterances_per_s": round(B / t_dec * 1e3, 0),
        "hbm_copy_tb_per_s": round(hbm / 1e12, 3),
        "fraction_of_hbm_copy": {k: round(need[k][0] / (ms[k] * 1e-3) / hbm, 4) for k in ms},
        "fp64_tflops": {k: round(need[k][1] / (ms[k] * 1e-3) / 1e12, 3) for k in ("emit", "stats")},
        "us_per_frame_step": {k: round(ms[k] * 1e3 / Tmax, 4) for k in ("forward", "backward", "viterbi", "backtrack")},
        "host_threads": min(args.threads, 16), "host_utterances_run": n_host,
        "host_em_plus_decode_seconds": round(t_host, 3),
        "host_utterances_per_s": round(B / t_host, 1),
        "gpu_em_plus_decode_ms": round(t_em + t_dec - ms["emit"], 3),
        "speedup_over_host": round(t_host * 1e3 / (t_em + t_dec - ms["emit"]), 1)}), flush=True)


if __name__ == "__main__":
    main()
