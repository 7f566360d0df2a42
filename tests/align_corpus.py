"""Seeded synthetic corpora whose phone boundaries are known, for the forced aligner's tests.

`corpus(seed, n)`: 12 phones plus `sil` / `sp`, a 30-word lexicon of 2-4 phones per word.  Every (phone, state) class (2 states per
phone) draws a mean in R^80, N(0, SEP^2) per dimension; utterances have 3-8 words, phones of 2-12 frames (the first state takes the
first half, rounded up), a pause of 2-12 frames between two words with probability 0.3 and 0-10 frames of leading and of trailing
silence; frame t is N(mean of its class, SIGMA^2).  The 80-channel matrix stands where the log-mel spectrogram stands in the
product, so the aligner's own feature step (mean removal, differences) applies to it.

`wav_corpus(root, seed, n)`: the same idea as audio for the command-line test: every phone is a fixed mixture of three sinusoids (one
between 100 and 300 Hz, so that the F0 extractor finds the utterance voiced),
silence is faint noise, 16-bit PCM at 22050 Hz, boundaries on multiples of the 256-sample hop; writes `{raw}/{speaker}/{name}.wav`,
`.lab` and a lexicon file."""
import os

import numpy as np

PHONES = ["AA", "B", "CH", "D", "EH", "F", "G", "IY", "K", "L", "M", "S"]
N_MEL, STATES, SIGMA, SEP = 80, 2, 1.0, 0.5
SR, HOP = 22050, 256


def lexicon(rng):
    lex = {}
    for i in range(30):
        lex[f"w{i:02d}"] = [PHONES[k] for k in rng.randint(0, len(PHONES), rng.randint(2, 5))]
    return lex


def _utterance(rng, lex, dur_lo, dur_hi):
    """-> (words, segments [(phone, frames)] with silences of 0 frames left out)"""
    words = [sorted(lex)[k] for k in rng.randint(0, len(lex), rng.randint(3, 9))]
    segs = [("sil", int(rng.randint(0, 11)))]
    for w, word in enumerate(words):
        if w and rng.rand() < 0.3:
            segs.append(("sp", int(rng.randint(dur_lo, dur_hi + 1))))
        segs += [(p, int(rng.randint(dur_lo, dur_hi + 1))) for p in lex[word]]
    segs.append(("sil", int(rng.randint(0, 11))))
    return words, [s for s in segs if s[1] > 0]


def boundaries(durations):
    """interior boundaries (frames) of a sequence of segment lengths, zero-length segments ignored"""
    d = [int(n) for n in durations if n > 0]
    return np.cumsum(d)[:-1]


def accuracy(true_durs, got_durs, tol):
    """share of the true interior boundaries, over all utterances, that have a found boundary within +-tol frames"""
    hit = n = 0
    for t, g in zip(true_durs, got_durs):
        tb, gb = boundaries(t), boundaries(g)
        n += len(tb)
        hit += sum(1 for v in tb if len(gb) and np.abs(gb - v).min() <= tol)
    return hit / n


def corpus(seed, n):
    """-> (lexicon, [dict(words, mel (80, T) float32, segments)])"""
    rng = np.random.RandomState(seed)
    lex = lexicon(rng)
    means = {(p, s): SEP * rng.randn(N_MEL) for p in PHONES + ["sil", "sp"] for s in range(STATES)}
    utts = []
    for _ in range(n):
        words, segs = _utterance(rng, lex, 2, 12)
        rows = []
        for p, d in segs:
            first = (d + 1) // 2
            rows += [means[(p, 0)]] * first + [means[(p, 1)]] * (d - first)
        mel = np.stack(rows) + SIGMA * rng.randn(len(rows), N_MEL)
        utts.append({"words": words, "mel": mel.T.astype(np.float32), "segments": segs})
    return lex, utts


def wav_corpus(root, seed, n, dur_lo=6, dur_hi=14, speaker="spk"):
    """Writes {root}/raw/{speaker}/{name}.wav|.lab and {root}/lexicon.txt; -> (lexicon path, {name: segments})."""
    from scipy.io import wavfile
    rng = np.random.RandomState(seed)
    lex = lexicon(rng)
    tones = {p: (np.concatenate([rng.uniform(100, 300, 1), rng.uniform(400, 4000, 2)]), rng.uniform(0.5, 1.0, 3)) for p in PHONES}
    os.makedirs(os.path.join(root, "raw", speaker), exist_ok=True)
    with open(os.path.join(root, "lexicon.txt"), "w") as f:
        for w in sorted(lex):
            f.write(w.upper() + "\t" + " ".join(lex[w]) + "\n")
    truth = {}
    for u in range(n):
        words, segs = _utterance(rng, lex, dur_lo, dur_hi)
        parts = []
        for p, d in segs:
            k = np.arange(d * HOP)
            if p in tones:
                fr, am = tones[p]
                parts.append(0.25 * sum(a * np.sin(2 * np.pi * f * k / SR) for f, a in zip(fr, am)) / am.sum())
            else:
                parts.append(1e-3 * rng.randn(d * HOP))
        pcm = np.round(np.concatenate(parts) * 32767).astype(np.int16)
        name = f"utt{u:03d}"
        wavfile.write(os.path.join(root, "raw", speaker, name + ".wav"), SR, pcm)
        with open(os.path.join(root, "raw", speaker, name + ".lab"), "w") as f:
            f.write(" ".join(words))
        truth[name] = segs
    return os.path.join(root, "lexicon.txt"), truth
