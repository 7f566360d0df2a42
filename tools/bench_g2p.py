#!/usr/bin/env python
"""Times the grapheme-to-phoneme model (fastspeech2_amd/g2p.py) on a synthetic lexicon (tests/g2p_corpus.py's rules, 200 000 entries):

    python tools/bench_g2p.py [--entries 200000] [--decode 20000] [--slice 2000] [--ref_decode 200]

Prints one JSON line: entries/s of every EM iteration (E-step, count reduction, M-step) and words/s of decoding at K = 64, N = 4 on
the GPU, and the same two figures for the numpy reference (tests/g2p_ref.py) on a slice of the lexicon: one E-step over `--slice`
entries and the beam search over the first `--ref_decode` of them.  An instrument: no bar is set.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastspeech2_amd import g2p  # noqa: E402
from tests import g2p_corpus, g2p_ref  # noqa: E402


def lexicon(n, seed=0):
    """n distinct words of 3 to 9 letters with their regular pronunciation, about 5 % exceptions"""
    rng = np.random.RandomState(seed)
    lex = {}
    while len(lex) < n:
        for row, length in zip(rng.randint(0, len(g2p_corpus.LETTERS), (n, 9)), rng.randint(3, 10, n)):
            word = "".join(g2p_corpus.LETTERS[k] for k in row[:length])
            pron = g2p_corpus.regular(word)
            if word in lex or not pron:
                continue
            if rng.rand() < 0.05:
                pron[rng.randint(0, len(pron))] = g2p_corpus.PHONES[rng.randint(0, len(g2p_corpus.PHONES))]
            lex[word] = pron
            if len(lex) == n:
                break
    return lex


def main(args):
    lex = lexicon(args.entries)
    t0 = time.perf_counter()
    model = g2p.G2P.train(lex, order=4, iters=args.iters, beam=64, device="cuda", tol=-1.0)
    train_s = time.perf_counter() - t0
    n = model.summary["entries_used"]
    words = list(lex)[:args.decode]
    model.pronounce(words[:64])                                            # tables to the device, first launch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    said = model.pronounce(words)
    decode_s = time.perf_counter() - t0
    right = sum(1 for w, p in zip(words, said) if p == lex[w])

    entries, letters, phones = g2p_corpus.ids({w: lex[w] for w in list(lex)[:args.slice]})
    A, P = len(letters), len(phones)
    t0 = time.perf_counter()
    g2p_ref.counts_of(entries, np.zeros(g2p_ref.table_size(A, P)), A, P)                   # the flat-start E-step
    ref_em_s = time.perf_counter() - t0
    md = g2p_ref.model_from_arrays(model.lm, 4)
    sp = g2p_ref.spelling(model.type_letters.tolist(), len(model.letters))
    lid = {c: k for k, c in enumerate(model.letters)}
    t0 = time.perf_counter()
    for w in words[:args.ref_decode]:
        g2p_ref.beam_search([lid[c] for c in w], sp, md, 4, 64, len(model.type_phones), model.type_phones.tolist())
    ref_decode_s = time.perf_counter() - t0
    print(json.dumps({"entries": n, "em_entries_per_s": [round(n / s, 1) for s in model.summary["em_seconds"]],
                      "train_seconds_total": round(train_s, 2), "em_types": model.summary["em_types"],
                      "graphone_types": model.summary["graphone_types"], "ngrams": model.summary["ngrams"],
                      "decode_words": len(words), "decode_words_per_s": round(len(words) / decode_s, 1),
                      "decode_words_right": right, "beam": 64, "order": 4,
                      "reference_em_entries": len(entries), "reference_em_entries_per_s": round(len(entries) / ref_em_s, 1),
                      "reference_decode_words": min(args.ref_decode, len(words)),
                      "reference_decode_words_per_s": round(min(args.ref_decode, len(words)) / ref_decode_s, 1)}))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--entries", type=int, default=200000)
    parser.add_argument("--iters", type=int, default=8)
    parser.add_argument("--decode", type=int, default=20000)
    parser.add_argument("--slice", type=int, default=2000)
    parser.add_argument("--ref_decode", type=int, default=200)
    main(parser.parse_args())
