#!/usr/bin/env python
"""recognize.py — phone error rate of a folder of wavs under the forced aligner's acoustic model (fastspeech2_amd/recognize.py):

    python recognize.py MODEL.npz -p preprocess.yaml --source val.txt --wav_dir DIR [--lm none] [--lm_scale 8] [--penalty 0]
                        [--out per.jsonl]

MODEL.npz is what `python align.py preprocess.yaml --save_model MODEL.npz` wrote.  For every `basename|speaker|{phones}|...` line of
`--source`, `{wav_dir}/{basename}.wav` is decoded by a Viterbi pass over a free loop of all phones and the phones it hears are
scored against the line's `{...}` field by edit distance, `sil`, `sp` and `spn` dropped from both sides.  One JSON object per
utterance goes to `--out` (basename, n_ref, hits, sub, del, ins, per, score_per_frame, hyp = [[phone, start_s, end_s], ...]), one
summary line to stdout: the corpus PER (the sum of the errors over the sum of n_ref), the counts, the 10 most frequent
substitutions and the most deleted and inserted phones.  Run it on the folder `synthesize.py --mode batch` wrote and on the
recorded wavs: the second number is the recogniser's own floor, and only the difference of the two means anything.  `--lm_scale 8`
and `--penalty 0` are choices, not measurements; no PER has been measured on real speech."""
import argparse
import json
import sys

import yaml

from fastspeech2_amd import recognize


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("model", type=str, help="model file written by `align.py --save_model`")
    parser.add_argument("-p", "--preprocess_config", type=str, required=True, help="path to preprocess.yaml")
    parser.add_argument("--source", type=str, required=True, help="metadata file of `basename|speaker|{phones}|...` lines (val.txt)")
    parser.add_argument("--wav_dir", type=str, required=True, help="folder of the wavs to decode, `{basename}.wav`")
    parser.add_argument("--lm", choices=("bigram", "none"), default="bigram", help="the model file's phone bigram, or no language model")
    parser.add_argument("--lm_scale", type=float, default=8.0, help="weight of the bigram's log-probabilities (a choice)")
    parser.add_argument("--penalty", type=float, default=0.0, help="added to every phone-to-phone arc; negative: fewer insertions")
    parser.add_argument("--out", type=str, default="per.jsonl")
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--batch_gib", type=float, default=2.0, help="device buffers per ragged batch")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    config = yaml.load(open(args.preprocess_config, "r"), Loader=yaml.FullLoader)
    try:
        rows, missing, summary = recognize.run(args.model, config, args.source, args.wav_dir, lm=args.lm, lm_scale=args.lm_scale,
                                               penalty=args.penalty, out_path=args.out, device=args.device,
                                               batch_bytes=int(args.batch_gib * (1 << 30)))
    except ValueError as e:
        sys.exit(str(e))
    for name, reason in missing:
        print("skipped {}: {}".format(name, reason))
    print(json.dumps(summary))
    return rows, missing, summary


if __name__ == "__main__":
    main()
