#!/usr/bin/env python
"""speaker.py — speaker similarity of a folder of wavs under a GMM-UBM verifier (fastspeech2_amd/speaker.py):

    python speaker.py train preprocess.yaml MODEL.npz [--source train.txt] [--components 256] [--iters 4] [--relevance 16]
                            [--n_cep 19] [--max_frames_per_speaker 20000]
    python speaker.py score MODEL.npz -p preprocess.yaml --source val.txt --wav_dir DIR [--out rows.jsonl]

`train` reads `{raw_path}/{speaker}/{basename}.wav` for every `basename|speaker|...` line of `--source` (default:
`{preprocessed_path}/train.txt`), trains the universal background model on the pooled frames, MAP-adapts one model per speaker and
writes MODEL.npz.  A list of fewer than two speakers is refused: a single-speaker UBM is the speaker.  `score` scores
`{wav_dir}/{basename}.wav` against the speaker column of the list: one JSON object per utterance goes to `--out` (basename,
speaker, llr, rank, rival, margin, n_kept), one summary line to stdout (mean target llr, top-1 accuracy, equal error rate, a
per-speaker table).  Run it on the folder `synthesize.py --mode batch` wrote and on the recorded wavs: the second run is the floor,
and only the difference of the two means anything.  No number has been measured on real speech."""
import argparse
import json
import os
import sys

import yaml

from fastspeech2_amd import speaker


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train")
    tr.add_argument("preprocess_config", type=str, help="path to preprocess.yaml")
    tr.add_argument("model", type=str, help="model file to write")
    tr.add_argument("--source", type=str, default=None, help="`basename|speaker|...` lines (default: train.txt of the config)")
    tr.add_argument("--components", type=int, default=256, help="mixture components, a power of two")
    tr.add_argument("--iters", type=int, default=4, help="EM passes after each doubling")
    tr.add_argument("--relevance", type=float, default=16.0, help="MAP relevance factor r")
    tr.add_argument("--n_cep", type=int, default=19, help="cepstra beside c0; the features have twice as many dimensions")
    tr.add_argument("--max_frames_per_speaker", type=int, default=20000)
    tr.add_argument("--var_floor", type=float, default=0.01, help="variance floor, times the global variance")
    tr.add_argument("--min_occ", type=float, default=3.0, help="a component under this occupancy is re-seeded")
    tr.add_argument("--energy_floor", type=float, default=None, help="keep frames whose c0 is within this of the utterance's maximum")
    sc = sub.add_parser("score")
    sc.add_argument("model", type=str, help="model file written by `speaker.py train`")
    sc.add_argument("-p", "--preprocess_config", type=str, required=True, help="path to preprocess.yaml")
    sc.add_argument("--source", type=str, required=True, help="`basename|speaker|...` lines (val.txt)")
    sc.add_argument("--wav_dir", type=str, required=True, help="folder of the wavs to score, `{basename}.wav`")
    sc.add_argument("--out", type=str, default="speaker.jsonl")
    for p in (tr, sc):
        p.add_argument("--device", type=str, default="cuda")
        p.add_argument("--batch_gib", type=float, default=1.0, help="device buffers per ragged batch")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    config = yaml.load(open(args.preprocess_config, "r"), Loader=yaml.FullLoader)
    budget = int(args.batch_gib * (1 << 30))
    try:
        if args.command == "train":
            source = args.source or os.path.join(config["path"]["preprocessed_path"], "train.txt")
            model, skipped = speaker.train(config, args.model, source, args.components, args.iters, args.relevance, args.n_cep,
                                           args.max_frames_per_speaker, args.var_floor, args.min_occ, args.energy_floor, args.device,
                                           budget)
            for name, reason in skipped:
                print("skipped {}: {}".format(name, reason))
            print("log-likelihood per frame: " + " ".join("{:.6f}".format(v) for stage in model.history for v in stage))
            print("{} speakers enrolled, {} components of {} dimensions".format(len(model.names), model.components, model.D))
            return model
        rows, missing, summary = speaker.score(args.model, config, args.source, args.wav_dir, args.out, args.device, budget)
    except ValueError as e:
        sys.exit(str(e))
    for name, reason in missing:
        print("skipped {}: {}".format(name, reason))
    print(json.dumps(summary))
    return rows, missing, summary


if __name__ == "__main__":
    main()
