#!/usr/bin/env python
"""g2p.py — train a grapheme-to-phoneme model from a pronunciation lexicon and apply it (fastspeech2_amd/g2p.py):

    python g2p.py train LEXICON MODEL.npz [--order 4 --iters 8 --beam 64 --holdout 0.05 --seed 0]
    python g2p.py apply MODEL.npz WORDS.txt [--output OUT.txt]

`train` runs the many-to-many EM alignment and the n-gram estimate on the lexicon's first pronunciations; with --holdout it prints the
word and phone error rates on the held-out entries (an instrument: no threshold is claimed).  `apply` reads one word per line and
writes lexicon-format lines (WORD<tab>PHONES); a word without a pronunciation is reported and left out.
"""
import argparse
import sys

from fastspeech2_amd.g2p import G2P


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers(dest="command", required=True)
    t = sub.add_parser("train")
    t.add_argument("lexicon")
    t.add_argument("model")
    t.add_argument("--order", type=int, default=4)
    t.add_argument("--iters", type=int, default=8)
    t.add_argument("--beam", type=int, default=64)
    t.add_argument("--holdout", type=float, default=0.0)
    t.add_argument("--seed", type=int, default=0)
    a = sub.add_parser("apply")
    a.add_argument("model")
    a.add_argument("words")
    a.add_argument("--output", default=None)
    for p in (t, a):
        p.add_argument("--device", default="cuda")
    return parser.parse_args(argv)


def main(args):
    if args.command == "train":
        model = G2P.train(args.lexicon, order=args.order, iters=args.iters, beam=args.beam, device=args.device, holdout=args.holdout,
                          seed=args.seed)
        model.save(args.model)
        s = model.summary
        print(f"trained on {s['entries_used']} entries (skipped {s['skipped']}), {s['graphone_types']} graphone types, n-grams {s['ngrams']}")
        print("log-likelihood per E-step: " + " ".join(f"{v:.3f}" for v in s["loglik"]))
        if "holdout_wer" in s:
            print(f"held out {s['entries_held_out']} entries: word error rate {s['holdout_wer']:.4f}, phone error rate {s['holdout_per']:.4f}")
        return
    model = G2P.load(args.model, args.device)
    with open(args.words, encoding="utf-8") as f:
        words = [line.split()[0] for line in f if line.split()]
    out = open(args.output, "w", encoding="utf-8") if args.output else sys.stdout
    missing = []
    for word, phones in zip(words, model.pronounce(words)):
        if phones is None:
            missing.append(word)
        else:
            out.write(word + "\t" + " ".join(phones) + "\n")
    if args.output:
        out.close()
    if missing:
        print(f"no pronunciation for {len(missing)} words: " + " ".join(missing[:20]), file=sys.stderr)


if __name__ == "__main__":
    main(parse_args())
