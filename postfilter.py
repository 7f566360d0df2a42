#!/usr/bin/env python
"""postfilter.py — trains the statistics of the modulation-spectrum postfilter (fastspeech2_amd/postfilter.py, whose docstring is the
specification):

    python postfilter.py train -p preprocess.yaml -m model.yaml -t train.yaml --restore_step N [--source train.txt]
                               [--batch_size 8] [--max_utts M] OUT.npz

The natural statistics come from the recorded mels `{preprocessed_path}/mel/{speaker}-mel-{basename}.npy` of the source list, read
the way copysynth.py reads them; the generated statistics from the acoustic model of checkpoint N run free (its own durations, pitch
and energy) over the phoneme strings of the same list, in the batches `synthesize.py --mode batch` builds.  No vocoder is loaded.  The
statistics are pooled over all speakers of the list.  `python synthesize.py --postfilter OUT.npz` then filters what it synthesizes.
Utterances with fewer than 32 or more than 2048 frames are left out of the side they are too short or long on, and counted."""
import argparse
import os

import numpy as np
import yaml


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest="command", required=True)
    t = sub.add_parser("train", help="natural and generated modulation-spectrum statistics over a source list, pooled over its speakers")
    t.add_argument("-p", "--preprocess_config", type=str, required=True, help="path to preprocess.yaml")
    t.add_argument("-m", "--model_config", type=str, required=True, help="path to model.yaml")
    t.add_argument("-t", "--train_config", type=str, required=True, help="path to train.yaml (path.ckpt_path)")
    t.add_argument("--restore_step", type=int, required=True, help="the acoustic model's checkpoint")
    t.add_argument("--source", type=str, default=None, help="metadata file like train.txt (default: {preprocessed_path}/train.txt)")
    t.add_argument("--batch_size", type=int, default=8, help="utterances per batch")
    t.add_argument("--max_utts", type=int, default=0, help="M > 0: only the first M lines of the source list")
    t.add_argument("--dtype", default=None, choices=[None, "fp32", "bf16"], help="the acoustic model's compute dtype")
    t.add_argument("out", metavar="OUT.npz", help="the statistics file: pooled over speakers, one table per side")
    args = parser.parse_args(argv)
    if args.batch_size < 1 or args.max_utts < 0:
        parser.error("--batch_size must be at least 1 and --max_utts not negative")
    return args


def natural_batches(source, preprocess_config, batch_size, max_utts=0):
    """-> (batches [(mels (B, Tmax, n_mel) float32 numpy, zero-padded; frames)], missing [(basename, reason)])"""
    from copysynth import read_source
    n_mel = preprocess_config["preprocessing"]["mel"]["n_mel_channels"]
    found, missing = read_source(source, preprocess_config["path"]["preprocessed_path"])
    if max_utts:
        found = found[:max_utts]
    batches = []
    for s in range(0, len(found), batch_size):
        mels = []
        for _basename, path in found[s:s + batch_size]:
            mel = np.load(path)
            if mel.ndim != 2 or mel.shape[1] != n_mel or mel.shape[0] < 1:
                raise ValueError(f"{path}: expected a (frames, {n_mel}) mel, got {mel.shape}")
            mels.append(mel.astype(np.float32))
        frames = [len(m) for m in mels]
        host = np.zeros((len(mels), max(frames), n_mel), dtype=np.float32)
        for b, m in enumerate(mels):
            host[b, :frames[b]] = m
        batches.append((host, frames))
    return batches, missing


def train(args, configs, model=None, device=None):
    """-> the Tables, also written to args.out.  `model`: an acoustic model already built (tests); else checkpoint args.restore_step"""
    import torch
    from fastspeech2_amd import postfilter as Postfilter
    from fastspeech2_amd.data import DevicePrefetcher, TextDataset
    from fastspeech2_amd.utils import get_model
    preprocess_config, model_config, train_config = configs
    device = device or torch.device("cuda", torch.cuda.current_device())
    pp = preprocess_config["preprocessing"]
    source = args.source or os.path.join(preprocess_config["path"]["preprocessed_path"], "train.txt")
    stats = Postfilter.Stats(pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"], pp["stft"]["hop_length"], args.restore_step)
    batches, missing = natural_batches(source, preprocess_config, args.batch_size, args.max_utts)
    for name, reason in missing:
        print("skipped {}: {}".format(name, reason))
    for host, frames in batches:
        stats.add_natural(torch.from_numpy(host).to(device), frames)
    if model is None:
        model = get_model(args, configs, device, train=False, compute_dtype=args.dtype)
    dataset = TextDataset(source, preprocess_config)
    n = len(dataset) if not args.max_utts else min(len(dataset), args.max_utts)
    batchs = (dataset.collate_fn([dataset[i] for i in range(s, min(s + args.batch_size, n))]) for s in range(0, n, args.batch_size))
    for batch in DevicePrefetcher(batchs, device):
        with torch.no_grad():
            out = model(*(batch[2:]))
        host = getattr(out[9], "_fs2_host", None)
        stats.add_generated(out[1].float(), [max(int(v), 1) for v in (host if host is not None else out[9].tolist())])
    tables = stats.finalize()
    tables.save(args.out)
    print("natural: {} utterances ({} left out), generated: {} utterances ({} left out), pooled over speakers -> {}".format(
        tables.n_natural, tables.left_out_natural, tables.n_generated, tables.left_out_generated, args.out))
    return tables


def main(argv=None, model=None):
    args = parse_args(argv)
    configs = tuple(yaml.load(open(p, "r"), Loader=yaml.FullLoader) for p in (args.preprocess_config, args.model_config, args.train_config))
    return train(args, configs, model=model)


if __name__ == "__main__":
    main()
