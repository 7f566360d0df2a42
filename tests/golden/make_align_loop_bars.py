"""Writes tests/golden/align_loop_bars.json: the phone error rate of the pure-numpy pipeline (tests/align_ref.py training, then the
phone-loop oracle tests/align_loop_ref.py) on the synthetic corpus of tests/align_corpus.py, per language-model setting and seed.
The GPU test (tests/test_align_loop_gpu.py) holds the product's PER on the first seed against `bar` = the worst recorded oracle
PER + MARGIN; the margin allows for tables trained by the two implementations differing in final rounding.

    python -m tests.golden.make_align_loop_bars

Per seed: `corpus(seed, 50)`, training on the first 40 utterances (2 states, 8 passes), the bigram from the oracle's own
alignments of those 40 (the blocks with frames, `sil` / `sp` included), decoding of the last 10 without a language model and with
the bigram (scale 8, penalty 0); the reference is the utterance's true segments, silences dropped on both sides."""
import json
import os

import numpy as np

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_loop_ref as LR
from tests import align_ref as R

SEEDS, N_UTT, N_TRAIN, ITERS, LM_SCALE, PENALTY, SMOOTHING, MARGIN = (4321, 17, 99), 50, 40, 8, 8.0, 0.0, 0.5, 0.02
SILENT = ("sil", "sp", "spn")
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_loop_bars.json")


def setup(seed):
    """-> (phone ids, graphs, features, utterances) of the seed's corpus"""
    lex, utts = C.corpus(seed, N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    return ids, graphs, [R.features(u["mel"]) for u in utts], utts


def heard(graph, frames, ids):
    """the phone ids of the blocks with frames"""
    return [ids[b[0]] for b, n in zip(graph["blocks"], frames) if n > 0]


def loop_costs(P, S, logp):
    """(self_, next_, link, init, final_) of a model without transitions; logp None: no language model"""
    C_ = P * S
    if logp is None:
        return np.zeros(C_), np.zeros(C_), np.zeros((P, P)), np.zeros(P), np.zeros(P)
    return np.zeros(C_), np.zeros(C_), LM_SCALE * logp[:P, :P] + PENALTY, LM_SCALE * logp[P, :P], LM_SCALE * logp[:P, P]


def score(hyps, utts):
    """-> (corpus PER, per-utterance (counts, ops, ref, hyp)); hyps: phone names per utterance, silences still in"""
    rows, err, n = [], 0, 0
    for hyp, u in zip(hyps, utts):
        ref = [p for p, _ in u["segments"] if p not in SILENT]
        hyp = [p for p in hyp if p not in SILENT]
        counts, ops = LR.edit_counts(ref, hyp)
        rows.append((counts, ops, ref, hyp))
        err, n = err + sum(counts[1:]), n + len(ref)
    return err / n, rows


def oracle_pers(seed):
    ids, graphs, xs, utts = setup(seed)
    names = sorted(ids, key=ids.get)
    P, S = len(ids), C.STATES
    mu, var, _ = R.fit(xs[:N_TRAIN], graphs[:N_TRAIN], P * S, ITERS)
    seqs = [heard(g, R.align(x, g, mu, var), ids) for x, g in zip(xs[:N_TRAIN], graphs[:N_TRAIN])]
    _, logp = LR.phone_bigram(seqs, P, SMOOTHING)
    out = {}
    for lm, table in (("none", None), ("bigram", logp)):
        costs = loop_costs(P, S, table)
        hyps = [[names[p] for p, _, _ in LR.decode(R.emissions(x, np.arange(P * S), mu, var), *costs, P, S)[0]] for x in xs[N_TRAIN:]]
        out[lm] = score(hyps, utts[N_TRAIN:])[0]
    return out


if __name__ == "__main__":
    per = {str(seed): oracle_pers(seed) for seed in SEEDS}
    doc = {"corpus": f"tests.align_corpus.corpus(seed, {N_UTT}), training on the first {N_TRAIN}, {ITERS} passes, {C.STATES} states",
           "lm_scale": LM_SCALE, "penalty": PENALTY, "smoothing": SMOOTHING, "margin": MARGIN, "seeds": list(SEEDS), "per": per,
           "bar": {lm: max(v[lm] for v in per.values()) + MARGIN for lm in ("none", "bigram")}}
    with open(PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))
