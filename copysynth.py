#!/usr/bin/env python
"""copysynth.py — copy synthesis: the RECORDED mel of every utterance through the vocoder, without the acoustic model:

    python copysynth.py -p preprocess.yaml -m model.yaml -t train.yaml --source val.txt [--out_dir DIR] [--batch_size 8]
                        [--vocoder_dtype fp32|bf16] [--hifigan_dir ..] [--melgan_dir ..] [--griffin_iters N] [--random_vocoder]

For every `basename|speaker|...` line of `--source` the file `{preprocessed_path}/mel/{speaker}-mel-{basename}.npy`, which
preprocess.py writes and training reads, goes through the configured vocoder (HiFi-GAN or MelGAN, ragged batches), or through N
Griffin-Lim iterations with `--griffin_iters N` (no vocoder checkpoint needed), and `{out_dir}/{basename}.wav` is written (default
out_dir: `{result_path}/copy`).  This is the "ground-truth mel + vocoder" row of a TTS paper's table: what the vocoder alone costs.
No acoustic model is built and no checkpoint of one is read.  A wav of a mel of T frames has T hop_length samples and shares the
time axis of the recording's TextGrid window, so `score.py --aligned --syn_dir {out_dir}` can score it sample against sample (STOI,
ESTOI).  Griffin-Lim synthesizes (T - 2) hop_length samples, as the reference's inv_mel_spec does; the last two hops are written as
zeros so that the file has the same length.  Missing mel files are listed and the rest is synthesized."""
import argparse
import os

import numpy as np
import yaml


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-p", "--preprocess_config", type=str, required=True, help="path to preprocess.yaml")
    parser.add_argument("-m", "--model_config", type=str, required=True, help="path to model.yaml (vocoder.model, vocoder.speaker)")
    parser.add_argument("-t", "--train_config", type=str, required=True, help="path to train.yaml (path.result_path)")
    parser.add_argument("--source", type=str, required=True, help="metadata file of `basename|speaker|...` lines (val.txt)")
    parser.add_argument("--out_dir", type=str, default=None, help="folder of the wavs (default: {result_path}/copy)")
    parser.add_argument("--batch_size", type=int, default=8, help="utterances per batch")
    parser.add_argument("--vocoder_dtype", default="fp32", choices=["fp32", "bf16"])
    parser.add_argument("--hifigan_dir", default="hifigan", help="directory with config.json + generator_*.pth.tar")
    parser.add_argument("--melgan_dir", default="melgan", help="vocoder.model MelGAN: directory with linda_johnson.pt / multi_speaker.pt")
    parser.add_argument("--griffin_iters", type=int, default=0,
                        help="N > 0: N Griffin-Lim iterations on the recorded mel (float32 wavs, no vocoder loaded); 0 = the vocoder")
    parser.add_argument("--random_vocoder", action="store_true", help="allow a random-init vocoder when no checkpoint exists (smoke runs)")
    parser.add_argument("--device", type=str, default="cuda")
    args = parser.parse_args(argv)
    if args.batch_size < 1:
        parser.error("--batch_size must be at least 1")
    if args.griffin_iters < 0:
        parser.error("--griffin_iters must not be negative")
    return args


def read_source(source, preprocessed_path):
    """-> (found [(basename, mel path)], missing [(basename, reason)]) for the lines of `source`, in their order"""
    found, missing = [], []
    with open(source, encoding="utf-8") as f:
        lines = [ln.strip("\n") for ln in f if ln.strip()]
    for ln in lines:
        parts = ln.split("|")
        if len(parts) < 2:
            missing.append((parts[0], "no speaker field"))
            continue
        path = os.path.join(preprocessed_path, "mel", "{}-mel-{}.npy".format(parts[1], parts[0]))
        if os.path.exists(path):
            found.append((parts[0], path))
        else:
            missing.append((parts[0], "missing " + path))
    return found, missing


def copy_synthesize(configs, source, out_dir=None, vocoder=None, batch_size=8, griffin_iters=0, device="cuda"):
    """The recorded mels of `source` through `vocoder` (or Griffin-Lim with `griffin_iters` > 0, `vocoder` is then not used) in
    batches of `batch_size`, longest first -> (written [(basename, samples)], missing [(basename, reason)])."""
    import torch
    from fastspeech2_amd.utils import _write_wavs, vocoder_infer
    preprocess_config, model_config, train_config = configs
    out_dir = out_dir or os.path.join(train_config["path"]["result_path"], "copy")
    found, missing = read_source(source, preprocess_config["path"]["preprocessed_path"])
    st, mc = preprocess_config["preprocessing"]["stft"], preprocess_config["preprocessing"]["mel"]
    hop, n_mel = st["hop_length"], mc["n_mel_channels"]
    stft = None
    if griffin_iters > 0:
        from fastspeech2_amd.audio import TacotronSTFT, mels_to_wavs_griffin_lim
        stft = TacotronSTFT(st["filter_length"], hop, st["win_length"], n_mel, preprocess_config["preprocessing"]["audio"]["sampling_rate"],
                            mc["mel_fmin"], mc["mel_fmax"]).to(device)
    elif vocoder is None:
        raise ValueError("copy_synthesize needs a vocoder, or griffin_iters > 0")
    mels = []
    for basename, path in found:
        mel = np.load(path)
        if mel.ndim != 2 or mel.shape[1] != n_mel or mel.shape[0] < 1:
            raise ValueError(f"{path}: expected a (frames, {n_mel}) mel, got {mel.shape}")
        mels.append(mel.astype(np.float32))
    order = sorted(range(len(found)), key=lambda i: (-len(mels[i]), i))
    written = [None] * len(found)
    for s in range(0, len(order), batch_size):
        batch = order[s:s + batch_size]
        frames = [len(mels[i]) for i in batch]
        host = np.zeros((len(batch), n_mel, max(frames)), dtype=np.float32)
        for b, i in enumerate(batch):
            host[b, :, :frames[b]] = mels[i].T
        dev_mels = torch.from_numpy(host).to(device)
        if griffin_iters > 0:
            wavs = mels_to_wavs_griffin_lim(dev_mels, frames, stft, griffin_iters)
            wavs = [np.concatenate([w, np.zeros(T * hop - len(w), dtype=w.dtype)]) for w, T in zip(wavs, frames)]
        else:
            wavs = vocoder_infer(dev_mels, vocoder, model_config, preprocess_config, lengths=[T * hop for T in frames])
        _write_wavs(out_dir, [found[i][0] for i in batch], wavs, preprocess_config)
        for i, w in zip(batch, wavs):
            written[i] = (found[i][0], len(w))
    return written, missing


def main(argv=None, vocoder=None):
    args = parse_args(argv)
    configs = tuple(yaml.load(open(p, "r"), Loader=yaml.FullLoader)
                    for p in (args.preprocess_config, args.model_config, args.train_config))
    if vocoder is None and args.griffin_iters == 0:
        import torch
        from fastspeech2_amd.utils import get_vocoder
        vocoder = get_vocoder(configs[1], torch.device(args.device), hifigan_dir=args.hifigan_dir, melgan_dir=args.melgan_dir,
                              compute_dtype=args.vocoder_dtype, allow_random_init=args.random_vocoder)
    written, missing = copy_synthesize(configs, args.source, out_dir=args.out_dir, vocoder=vocoder, batch_size=args.batch_size,
                                       griffin_iters=args.griffin_iters, device=args.device)
    for name, reason in missing:
        print("skipped {}: {}".format(name, reason))
    out_dir = args.out_dir or os.path.join(configs[2]["path"]["result_path"], "copy")
    print("copy-synthesized {} utterances -> {} ({} skipped)".format(len(written), out_dir, len(missing)))
    return written, missing


if __name__ == "__main__":
    main()
