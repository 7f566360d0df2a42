"""Writes tests/golden/g2p_bars.json: the float64 reference (tests/g2p_ref.py) trained on the synthetic lexicon of tests/g2p_corpus.py
with 10 % held out, run on the CPU.  Recorded: the log-likelihood of every E-step, the reference's pronunciation of every held-out
word with the smallest score gap that decided it (relative to |score|), the share of held-out words whose gap is above 0 and below
1e-9 (an exact tie is decided by the stated rule, the lower index, on both sides, and is no near tie; the near-tie rule of tests/test_g2p_gpu.py allows at most 2 %) and the held-out word accuracy, the bar the GPU model must reach minus one
word.  The corpus seed is the first of 0, 1, 2, ... for which the near-tie share stays within 2 %.

    python tests/golden/make_g2p_bars.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import g2p_corpus, g2p_ref  # noqa: E402

HOLDOUT, SPLIT_SEED, ORDER, BEAM, NEAR = 0.1, 0, 4, 64, 1e-9


def run(seed):
    lex = g2p_corpus.lexicon(seed)
    entries, letters, phones = g2p_corpus.ids(lex)
    train, held = g2p_ref.split(len(entries), HOLDOUT, SPLIT_SEED)
    m = g2p_ref.train_model([entries[k] for k in train], len(letters), len(phones), ORDER)
    words, rows = list(lex), []
    for k in held:
        ph, score, _, gap = g2p_ref.pronounce(m, entries[k][0], BEAM)
        rows.append({"word": words[k], "phones": None if ph is None else [phones[p] for p in ph],
                     "gap": None if ph is None else min(gap / abs(score), 1.0), "correct": ph == entries[k][1]})
    near = sum(1 for r in rows if r["gap"] is not None and 0.0 < r["gap"] < NEAR)
    return {"corpus_seed": seed, "holdout": HOLDOUT, "split_seed": SPLIT_SEED, "order": ORDER, "beam": BEAM,
            "loglik": [float(v) for v in m["history"]], "graphone_types": len(m["tokens"]),
            "align_near_ties": sum(1 for g in m["align_gaps"] if 0.0 < g < NEAR) / len(train), "held_out": rows,
            "near_tie_share": near / len(rows), "word_accuracy": sum(r["correct"] for r in rows) / len(rows)}


if __name__ == "__main__":
    for seed in range(20):
        bars = run(seed)
        print(seed, bars["near_tie_share"], bars["align_near_ties"], bars["word_accuracy"])
        if bars["near_tie_share"] <= 0.02 and bars["align_near_ties"] <= 0.02:
            break
    with open(os.path.join(ROOT, "tests", "golden", "g2p_bars.json"), "w") as f:
        json.dump(bars, f, indent=1)
