"""What the modulation-spectrum postfilter (fastspeech2_amd/postfilter.py) costs.  Two numbers, one JSON line:

  apply_ms      `postfilter.apply` on a resident synthetic float32 batch of 8 rows of about 800 frames x 80 bins, device time between
                two events, best of 5 after one warm-up call
  pipeline_ms   one val.txt-shaped batch of 8 through utils.SynthPipeline (bf16 acoustic model and HiFi-GAN, as tools/prof_synth.py
                builds them), wall time per batch over 12 batches, best of 5, without the filter and with it at k = 0.85

    python tools/bench_postfilter.py

The statistics are synthetic (random tables): the filter's cost does not depend on their values."""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tables(K=80, seed=3):
    from fastspeech2_amd import postfilter as PF
    rng = np.random.default_rng(seed)
    mu_g, sd_g = rng.standard_normal((K, PF.BINS)), rng.uniform(0.5, 2.0, (K, PF.BINS))
    return PF.Tables(mu_g + rng.uniform(0.0, 2.0, (K, PF.BINS)), sd_g * rng.uniform(0.8, 1.25, (K, PF.BINS)), mu_g, sd_g, 4, 4, 0, 0, K, 22050, 256)


def time_apply(dev, t, reps=5):
    from fastspeech2_amd import postfilter as PF
    lens = [800, 760, 812, 790, 700, 845, 777, 801]
    g = torch.Generator(device="cpu").manual_seed(7)
    mel = (torch.randn(len(lens), max(lens), 80, generator=g) * 2.0 - 5.0).to(dev)
    out = torch.empty_like(mel)
    PF.apply(mel, lens, t, 0.85, out=out)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        PF.apply(mel, lens, t, 0.85, out=out)
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best, lens


def time_pipeline(dev, t, reps=5, n=12):
    from fastspeech2_amd import hifigan, utils
    from fastspeech2_amd import synthetic as configs
    from fastspeech2_amd.model import FastSpeech2
    from fastspeech2_amd.synthetic import synthetic_batch, val_phoneme_counts
    pcfg, mcfg = configs.make_configs(dec_layers=4, enc_layers=4)
    torch.manual_seed(1234)
    model = FastSpeech2(pcfg, mcfg, compute_dtype="bf16")
    with torch.no_grad():
        model.variance_adaptor.duration_predictor.linear_layer.bias.fill_(math.log(8.0))
    model.to(dev).eval()
    voc = hifigan.Generator(hifigan.AttrDict(utils.HIFIGAN_V1), compute_dtype="bf16")
    voc.eval()
    voc.remove_weight_norm()
    voc.to(dev)
    counts = val_phoneme_counts()
    batches = []
    for gi in range(6):
        b = synthetic_batch(4321 + gi, 0, 0, src_lens=counts[8 * gi:8 * gi + 8], sort=False)
        batches.append(([f"u{i}" for i in range(8)], None, b["speakers"].to(dev), b["texts"].to(dev), b["src_lens"].to(dev), b["max_src_len"]))
    result = {}
    for name, pf in (("pipeline_ms", None), ("pipeline_postfilter_ms", (t, 0.85))):
        pipe = utils.SynthPipeline(model, voc, (pcfg, mcfg), device=dev, voc_streams=3, postfilter=pf)
        frames = []
        for _b, out, _w in pipe(batches[i % len(batches)] for i in range(6)):          # warm-up
            frames.append(int(out[9]._fs2_host.max()))
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            for _item in pipe(batches[i % len(batches)] for i in range(n)):
                pass
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3 / n)
        result[name] = round(best, 3)
        result["pipeline_max_frames"] = max(frames)
    return result


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    t = tables()
    apply_ms, lens = time_apply(dev, t)
    result = {"apply_ms": round(apply_ms, 3), "apply_rows": len(lens), "apply_frames": lens, "apply_bins": 80}
    result.update(time_pipeline(dev, t))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
