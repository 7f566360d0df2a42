"""Throughput of Griffin-Lim mel inversion on the GPU (audio.mels_to_wavs_griffin_lim, 60 iterations by default) over val.txt-shaped
batches of 8 log-mels: mel lengths from a seeded draw (phoneme counts of the reference's LJSpeech val.txt in file order, durations
uniform in [4, 10] frames per phoneme - the bench's synthesis workload), batches in file order as synthesize.py forms them.
Warm-up, then device-event timing of whole batches; a second pass with per-GEMM events gives the GEMMs' share.  Beside it, for
scale: a torch-CPU restatement (F.conv1d / conv_transpose1d, fp32) of the same iterations on one utterance - a restatement, not
the reference.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_TF = 157.3


def workload(n_batches, B=8, seed=0):
    from fastspeech2_amd.synthetic import val_phoneme_counts
    counts = val_phoneme_counts()[:n_batches * B]
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(4, 11, c).sum()) for c in counts]
    return [lens[i:i + B] for i in range(0, len(lens), B)]


def cpu_restatement(mel_len, n_iters, threads):
    """stft.py transform / inverse + audio_processing.py griffin_lim restated with torch CPU ops (fp32), one utterance"""
    import torch.nn.functional as F
    from fastspeech2_amd.audio import dft_basis, inverse_basis, window_sumsquare
    torch.set_num_threads(threads)
    fwd, inv = dft_basis(1024, 1024)[:, None, :], inverse_basis(1024, 256, 1024)[:, None, :]
    Fr = mel_len - 1
    mag = torch.rand(1, 513, Fr)
    env = torch.from_numpy(window_sumsquare("hann", Fr, 256, 1024, 1024))
    nz = env > np.finfo(np.float32).tiny

    def inverse(ph):
        y = F.conv_transpose1d(torch.cat([mag * torch.cos(ph), mag * torch.sin(ph)], 1), inv, stride=256)
        y[:, :, nz] /= env[nz]
        return (y * 4.0)[:, :, 512:-512]

    t0 = time.perf_counter()
    y = inverse(torch.rand(1, 513, Fr) * 6.28)
    for _ in range(n_iters):
        ft = F.conv1d(F.pad(y.unsqueeze(1), (512, 512, 0, 0), mode="reflect").squeeze(1), fwd, stride=256)
        y = inverse(torch.atan2(ft[:, 513:], ft[:, :513]))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="val.txt-shaped batches of 8 (64 = the whole val.txt)")
    ap.add_argument("--iters", type=int, default=60, help="Griffin-Lim iterations (inv_mel_spec: 60)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from fastspeech2_amd import ops
    from fastspeech2_amd.audio import TacotronSTFT, mels_to_wavs_griffin_lim
    dev = torch.device("cuda", 0)
    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(dev)
    batches = workload(args.batches)
    g = torch.Generator().manual_seed(0)
    mels = [torch.normal(-5.0, 2.0, (len(lens), 80, max(lens)), generator=g).to(dev) for lens in batches]
    angles = [[np.random.default_rng(b).uniform(-np.pi, np.pi, (513, n - 1)).astype(np.float32) for n in lens]
              for b, lens in enumerate(batches)]

    def run(i):
        return mels_to_wavs_griffin_lim(mels[i], batches[i], stft, n_iters=args.iters, angles=angles[i])

    for _ in range(args.warmup):
        for i in range(len(batches)):
            run(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_batch = []
    for _ in range(args.repeats):
        e0.record()
        for i in range(len(batches)):
            run(i)                   # ends in a device-to-host copy of the signals: batch i finishes before batch i+1 starts
        e1.record()
        torch.cuda.synchronize()
        per_batch.append(e0.elapsed_time(e1) / len(batches))
    ms = float(np.median(per_batch))
    # the GEMMs alone: per-launch HIP events (ops.PROFILE) over one more pass
    ops.PROFILE = {}
    e0.record()
    for i in range(len(batches)):
        run(i)
    e1.record()
    torch.cuda.synchronize()
    prof, ops.PROFILE = ops.PROFILE, None
    rec = prof.get("conv_gemm", [])
    gemm_ms = sum(r[1].elapsed_time(r[2]) for r in rec) / len(batches)
    gemm_flop = sum(r[0] for r in rec) / len(batches)                 # 2 M N K of the launches as issued (padded frame rows)
    prof_ms = e0.elapsed_time(e1) / len(batches)
    frames = [n - 1 for lens in batches for n in lens]
    valid_flop = args.iters * 2.0 * sum(frames) * (1026 + 1028) * 1024 / len(batches)   # forward + inverse on valid frames only
    audio_s = sum(256 * (f - 1) for f in frames) / 22050 / len(batches)
    out = {
        "workload": f"{len(batches)} val.txt-shaped batches of 8 ({sum(frames)} frames, {audio_s * len(batches):.1f} s of 22.05 kHz audio), "
                    f"{args.iters} Griffin-Lim iterations, fp32",
        "ms_per_batch": round(ms, 3), "ms_per_batch_repeats": [round(x, 3) for x in per_batch],
        "audio_s_per_batch": round(audio_s, 3), "rtf": float(f"{ms * 1e-3 / audio_s:.3e}"),
        "gemm_ms_per_batch": round(gemm_ms, 3), "gemm_tflops": round(gemm_flop / (gemm_ms * 1e-3) / 1e12, 1),
        "gemm_share_of_f32_mfma_peak": round(gemm_flop / (gemm_ms * 1e-3) / 1e12 / PEAK_F32_TF, 3),
        "valid_frame_tflops_end_to_end": round(valid_flop / (ms * 1e-3) / 1e12, 1),
        "non_gemm_share": round(max(prof_ms - gemm_ms, 0.0) / prof_ms, 3), "profiled_pass_ms_per_batch": round(prof_ms, 3),
        "f32_mfma_peak_tf": PEAK_F32_TF,
        "rtf_floor_at_peak": float(f"{valid_flop / (PEAK_F32_TF * 1e12) / audio_s:.3e}"),
    }
    if not args.no_cpu:
        med = int(np.median([n for lens in batches for n in lens]))
        t = cpu_restatement(med, args.iters, args.cpu_threads)
        out["cpu_torch_restatement"] = {"what": "torch-CPU restatement of the same iterations (not the reference), one utterance",
                                        "mel_frames": med, "threads": args.cpu_threads, "s": round(t, 3),
                                        "rtf": float(f"{t / (256 * (med - 2) / 22050):.3e}")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
