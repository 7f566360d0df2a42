"""Time of the MelGAN generator's `infer_pcm` at the batch-synthesis shape (B = 8 mels of T frames, bf16, random weights): the narrow
stages fused (one launch per stage, fs2_melgan_stage_fwd) against the chain of single launches, and - for scale, same process, same
shape - HiFi-GAN V1's `infer_pcm`.  Warm-up, then the median over timed windows of `--iters` back-to-back calls each (HIP events
around a window).  Also the isolated narrow stages (C = 64 / 32 at their row counts), fused against chain.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, windows, iters):
    """median ms per call over `windows` windows of `iters` calls"""
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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from fastspeech2_amd import hifigan, melgan, ops, utils
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, T = args.batch, args.frames
    x = (-5.0 * torch.rand(B, 80, T)).to(dev)
    res = {"bench": "melgan", "B": B, "T": T, "dtype": "bf16", "device": torch.cuda.get_device_name(0)}
    mg = melgan.Generator(compute_dtype="bf16").eval()
    mg.remove_weight_norm()
    mg.to(dev)
    mg.prepare(dev)
    with torch.no_grad():
        for name, fuse in (("fused", True), ("chain", False)):
            mg.fuse_stages = fuse
            med, lo, hi = timed(lambda: mg.infer_pcm(x), args.warmup, args.windows, args.iters)
            res[f"melgan_infer_pcm_{name}_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        hg = hifigan.Generator(hifigan.AttrDict(utils.HIFIGAN_V1), compute_dtype="bf16").eval()
        hg.remove_weight_norm()
        hg.to(dev)
        hg.prepare(dev)
        med, lo, hi = timed(lambda: hg.infer_pcm(x), args.warmup, args.windows, args.iters)
        res["hifigan_infer_pcm_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        # the narrow stages alone: rows of stage 2 (C = 64, S = 128 T) and stage 3 (C = 32, S = 256 T)
        W = mg._weights(dev)
        for i, C, S in ((2, 64, 128 * T), (3, 32, 256 * T)):
            xs = (torch.randn(B, S, C, device=dev) * 0.7).to(torch.bfloat16)
            y = torch.empty_like(xs)
            st = W[f"stage{i}"]
            med, lo, hi = timed(lambda: ops.melgan_stage_fwd(xs, st[0], st[1], y, melgan.DILATIONS, slope=0.2, out_slope=0.2),
                                args.warmup, args.windows, args.iters)
            res[f"stage_C{C}_fused_ms"] = round(med, 4)
            G = melgan.GUARD
            cat = [torch.empty(B, S + 2 * G, 2 * C, device=dev, dtype=torch.bfloat16) for _ in range(2)]
            out = torch.empty(B, S + 2 * G, C, device=dev, dtype=torch.bfloat16)

            def chain():
                ops.melgan_guard_rows(xs, cat[0][:, :, :C], G, reflect=True, interior=True)
                for j, d in enumerate(melgan.DILATIONS):
                    cur = cat[j % 2]
                    cur2 = cur.view(-1, 2 * C)
                    if j > 0:
                        ops.melgan_guard_rows(cur[:, G:G + S, :C], cur[:, :, :C], G, reflect=True, interior=False)
                    w3, b3 = W[f"rb{i}.{j}.3"]
                    w11, b11 = W[f"rb{i}.{j}.11"]
                    ops.conv_gemm(cur2, w3, b3, S + 2 * G, taps=3, dil=d, pad=d, act=ops.ACT_LRELU, slope=0.2, in_act=ops.ACT_LRELU,
                                  in_slope=0.2, Cin=C, out=cur2[:, C:])
                    last = j == 2
                    dst = out.view(-1, C) if last else cat[(j + 1) % 2].view(-1, 2 * C)[:, :C]
                    ops.conv_gemm(cur2, w11, b11, S + 2 * G, taps=1, act=ops.ACT_LRELU if last else ops.ACT_NONE, slope=0.2 if last else 0.0,
                                  out=dst)

            med, lo, hi = timed(chain, args.warmup, args.windows, args.iters)
            res[f"stage_C{C}_chain_ms"] = round(med, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
