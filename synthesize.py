#!/usr/bin/env python
"""synthesize.py — batch / single-utterance synthesis with the reference's CLI (reference synthesize.py:86-214):

    python synthesize.py --restore_step N --mode batch --source val.txt -p ... -m ... -t ...
    python synthesize.py --restore_step N --mode single --text "{HH AH0 L OW1}" -p ... -m ... -t ...

The acoustic model and the HiFi-GAN generator run as HIP kernels; wavs land in train_config.path.result_path.
With --griffin_iters N the wavs come from N Griffin-Lim iterations on the post-net mel instead (no vocoder checkpoint needed).
With --postfilter STATS.npz (written by `python postfilter.py train`) the post-net mel goes through the modulation-spectrum
postfilter (fastspeech2_amd/postfilter.py) before the vocoder or Griffin-Lim reads it; --postfilter_k is its emphasis coefficient.
Batch mode reads phoneme strings (the `{...}` field of train.txt / val.txt), exactly what the reference's TextDataset
does.  Single mode takes the phoneme string directly: the grapheme-to-phoneme step of the reference (g2p_en / pypinyin +
lexicon, synthesize.py:20-84) is host-side string processing outside the hot path and its packages are not in this
image, so raw text without braces is rejected with a clear message instead of being silently mis-read, unless --g2p_model names
a model trained by `python g2p.py train` (fastspeech2_amd/g2p.py): then English free text is pronounced with the lexicon and that model.
With WORLD_SIZE > 1 (torch.distributed.run) the source list is sharded across GPUs: replicas only, no collective.
"""
import argparse
import os
import re

import numpy as np
import torch
import yaml

import fastspeech2_amd
from fastspeech2_amd.data import DevicePrefetcher, TextDataset
from fastspeech2_amd.text import text_to_sequence
from fastspeech2_amd.utils import SynthPipeline, get_model, get_vocoder


def synthesize(model, step, configs, vocoder, batchs, control_values, device=None, postfilter=None):
    preprocess_config, model_config, train_config = configs
    pitch_control, energy_control, duration_control = control_values
    device = device or torch.device("cuda", torch.cuda.current_device())
    n = 0
    # the reference's loop (synthesize.py:87-103) as a stream pipeline: the next batch's acoustic model under the previous batches' vocoders
    pipeline = SynthPipeline(model, vocoder, configs, control_values, device=device, path=train_config["path"]["result_path"],
                             write=True, postfilter=postfilter)
    for batch, _output, _wavs in pipeline(DevicePrefetcher(batchs, device)):
        n += len(batch[0])
    if postfilter is not None and pipeline.passed_through:
        print(f"postfilter: {pipeline.passed_through} utterances too short or too long for it went through unchanged")
    return n


def synthesize_griffin_lim(model, configs, batchs, control_values, n_iters, device=None, postfilter=None):
    """--griffin_iters N: the post-net mel of each utterance (cut at its mel_len) -> Griffin-Lim (N iterations, audio/tools.py:18-34
    inv_mel_spec on the GPU, one ragged launch sequence per batch) -> float32 wavs; no vocoder is loaded."""
    from fastspeech2_amd.audio import TacotronSTFT, mels_to_wavs_griffin_lim
    from fastspeech2_amd.utils import _write_wavs
    preprocess_config, model_config, train_config = configs
    pitch_control, energy_control, duration_control = control_values
    device = device or torch.device("cuda", torch.cuda.current_device())
    st, mel = preprocess_config["preprocessing"]["stft"], preprocess_config["preprocessing"]["mel"]
    stft = TacotronSTFT(st["filter_length"], st["hop_length"], st["win_length"], mel["n_mel_channels"],
                        preprocess_config["preprocessing"]["audio"]["sampling_rate"], mel["mel_fmin"], mel["mel_fmax"]).to(device)
    n = 0
    for batch in DevicePrefetcher(batchs, device):
        with torch.no_grad():
            out = model(*(batch[2:]), p_control=pitch_control, e_control=energy_control, d_control=duration_control)
            mel = out[1]
            if postfilter is not None:
                from fastspeech2_amd import postfilter as Postfilter
                host = getattr(out[9], "_fs2_host", None)
                mel = Postfilter.apply(mel, host if host is not None else out[9].tolist(), postfilter[0], postfilter[1])
            wavs = mels_to_wavs_griffin_lim(mel.transpose(1, 2), out[9], stft, n_iters)
        _write_wavs(train_config["path"]["result_path"], batch[0], wavs, preprocess_config)
        n += len(batch[0])
    return n


def free_text(args, preprocess_config):
    """--g2p_model: English free text -> the braced phoneme string.  Lexicon words keep their lexicon phones, any other word gets the
    trained graphone model's (fastspeech2_amd/g2p.py), punctuation becomes `sp`; what the model cannot pronounce is left out."""
    from fastspeech2_amd.align import read_lexicon
    from fastspeech2_amd.g2p import G2P, text_to_phones
    if preprocess_config["preprocessing"]["text"]["language"] != "en":
        raise SystemExit("--g2p_model pronounces English text only (preprocessing.text.language is not en)")
    model = G2P.load(args.g2p_model, torch.device("cuda", torch.cuda.current_device()))
    phones, dropped = text_to_phones(args.text, read_lexicon(preprocess_config["path"]["lexicon_path"]), model)
    if dropped:
        print("warning: no pronunciation for {} (left out; numbers and abbreviations are not expanded)".format(", ".join(dropped)))
    print("Raw Text Sequence: {}".format(args.text))
    print("Phoneme Sequence: {}".format(phones))
    return phones


def single_batch(args, preprocess_config):
    if args.g2p_model is not None and not re.search(r"\{.+?\}", args.text):
        raw = args.text
        args.text = free_text(args, preprocess_config)
        texts = np.array([np.array(text_to_sequence(args.text, preprocess_config["preprocessing"]["text"]["text_cleaners"]))])
        ids = raw_texts = [raw[:100].replace(" ", "_")]
        return [(ids, raw_texts, np.array([args.speaker_id]), texts, np.array([len(texts[0])]), len(texts[0]))]
    if not re.search(r"\{.+?\}", args.text):
        raise SystemExit("--mode single expects a phoneme string in braces, e.g. --text \"{HH AH0 L OW1 sp W ER1 L D}\" "
                         "(grapheme-to-phoneme conversion needs g2p_en/pypinyin, which this build does not ship)")
    texts = np.array([np.array(text_to_sequence(args.text, preprocess_config["preprocessing"]["text"]["text_cleaners"]))])
    text_lens = np.array([len(texts[0])])
    ids = raw_texts = [args.text[:100].replace("{", "").replace("}", "").replace(" ", "_")]
    return [(ids, raw_texts, np.array([args.speaker_id]), texts, text_lens, max(text_lens))]


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--restore_step", type=int, required=True)
    parser.add_argument("--mode", type=str, choices=["batch", "single"], required=True,
                        help="Synthesize a whole dataset or a single sentence")
    parser.add_argument("--source", type=str, default=None,
                        help="path to a source file with format like train.txt and val.txt, for batch mode only")
    parser.add_argument("--text", type=str, default=None, help="phoneme string in braces, for single-sentence mode only")
    parser.add_argument("--speaker_id", type=int, default=0, help="speaker ID for multi-speaker synthesis, single mode only")
    parser.add_argument("-p", "--preprocess_config", type=str, required=True, help="path to preprocess.yaml")
    parser.add_argument("-m", "--model_config", type=str, required=True, help="path to model.yaml")
    parser.add_argument("-t", "--train_config", type=str, required=True, help="path to train.yaml")
    parser.add_argument("--pitch_control", type=float, default=1.0)
    parser.add_argument("--energy_control", type=float, default=1.0)
    parser.add_argument("--duration_control", type=float, default=1.0)
    parser.add_argument("--batch_size", type=int, default=8, help="utterances per batch (reference: 8)")
    parser.add_argument("--dtype", default=None, choices=[None, "fp32", "bf16"])
    parser.add_argument("--vocoder_dtype", default="fp32", choices=["fp32", "bf16"])
    parser.add_argument("--hifigan_dir", default="hifigan", help="directory with config.json + generator_*.pth.tar")
    parser.add_argument("--hw_queues", type=int, default=fastspeech2_amd.HW_QUEUES_DEFAULT,
                        help="HIP hardware queues of this process (GPU_MAX_HW_QUEUES; the runtime default 4 makes streams share queues: "
                             "utils.SynthPipeline / the engine's side streams); the same for every world size; an exported value wins; 0 = leave the runtime default")
    parser.add_argument("--melgan_dir", default="melgan",
                        help="vocoder.model MelGAN: directory with linda_johnson.pt / multi_speaker.pt (after a torch.hub run of the "
                             "reference they lie in ~/.cache/torch/hub/descriptinc_melgan-neurips_master/models/)")
    parser.add_argument("--random_vocoder", action="store_true", help="allow a random-init vocoder when no checkpoint exists (smoke runs)")
    parser.add_argument("--g2p_model", default=None,
                        help="a model trained by `python g2p.py train`: --mode single takes free English text (without it, a phoneme string in braces)")
    parser.add_argument("--griffin_iters", type=int, default=0,
                        help="N > 0: waveforms by N Griffin-Lim iterations on the post-net mel (float32 wavs, no vocoder loaded); 0 = HiFi-GAN")
    parser.add_argument("--postfilter", default=None, metavar="STATS.npz",
                        help="statistics written by `python postfilter.py train`: the post-net mel goes through the modulation-spectrum "
                             "postfilter before the vocoder (or Griffin-Lim) reads it")
    parser.add_argument("--postfilter_k", type=float, default=0.85, help="the postfilter's emphasis coefficient in [0, 1]; 0 = no filter")
    args = parser.parse_args(argv)
    if not 0.0 <= args.postfilter_k <= 1.0:
        parser.error("--postfilter_k must lie in [0, 1]")
    return args


def main(args):
    if args.mode == "batch":
        assert args.source is not None and args.text is None
    if args.mode == "single":
        assert args.source is None and args.text is not None
    configs = tuple(yaml.load(open(p, "r"), Loader=yaml.FullLoader)
                    for p in (args.preprocess_config, args.model_config, args.train_config))
    preprocess_config, model_config, train_config = configs
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    device = torch.device("cuda", torch.cuda.current_device())
    model = get_model(args, configs, device, train=False, compute_dtype=args.dtype)
    vocoder = None if args.griffin_iters > 0 else get_vocoder(model_config, device, hifigan_dir=args.hifigan_dir, melgan_dir=args.melgan_dir,
                                                              compute_dtype=args.vocoder_dtype, allow_random_init=args.random_vocoder)
    if args.mode == "batch":
        dataset = TextDataset(args.source, preprocess_config)
        mine = list(range(rank, len(dataset), world))          # replicas only: each GPU takes every world-th utterance
        batchs = (dataset.collate_fn([dataset[i] for i in mine[s:s + args.batch_size]])
                  for s in range(0, len(mine), args.batch_size))
    else:
        batchs = single_batch(args, preprocess_config)
    controls = (args.pitch_control, args.energy_control, args.duration_control)
    postfilter = None
    if args.postfilter is not None:
        from fastspeech2_amd import postfilter as Postfilter
        postfilter = (Postfilter.load(args.postfilter, preprocess_config), args.postfilter_k)
    if args.griffin_iters > 0:
        n = synthesize_griffin_lim(model, configs, batchs, controls, args.griffin_iters, device=device, postfilter=postfilter)
    else:
        n = synthesize(model, args.restore_step, configs, vocoder, batchs, controls, device=device, postfilter=postfilter)
    print(f"[rank {rank}] synthesized {n} utterances -> {train_config['path']['result_path']}")


if __name__ == "__main__":
    _args = parse_args()
    fastspeech2_amd.configure_hw_queues(_args.hw_queues)      # before the first HIP call; the pipeline keeps 4+ streams busy
    main(_args)
