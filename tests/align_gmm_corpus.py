"""A seeded bimodal variant of tests/align_corpus.py for the aligner's Gaussian-mixture emissions: the same lexicon, utterances and
durations, but every (phone, state) class has two variant means, the class mean of that corpus (N(0, SEP^2) per dimension) plus and
minus an offset of VSEP per dimension with a random sign per (class, dimension), and every segment (one phone of one utterance,
both of its states) draws one of the two variants with equal probability; frame t is N(mean of its class and variant, SIGMA^2).
The true boundaries are known.  A single Gaussian per class has to cover both variants with a variance of SIGMA^2 + VSEP^2 in
every dimension of every class (an offset whose size differed between classes would itself tell them apart), which leaves it
2 SEP^2 / (SIGMA^2 + VSEP^2) per dimension to separate two classes by; two components can take a variant each and keep
2 SEP^2 / SIGMA^2.  Measured with the two numpy oracles: see tests/test_align_gmm_gpu.py and DESIGN.md."""
import numpy as np

from tests.align_corpus import N_MEL, PHONES, STATES, _utterance, lexicon

SIGMA, SEP, VSEP = 1.0, 0.5, 3.0


def corpus(seed, n, sep=None, vsep=None, sigma=None):
    """-> (lexicon, [dict(words, mel (80, T) float32, segments, variants)])"""
    sep, vsep, sigma = SEP if sep is None else sep, VSEP if vsep is None else vsep, SIGMA if sigma is None else sigma
    rng = np.random.RandomState(seed)
    lex = lexicon(rng)
    means = {}
    for p in PHONES + ["sil", "sp"]:
        for s in range(STATES):
            centre, off = sep * rng.randn(N_MEL), vsep * np.where(rng.rand(N_MEL) < 0.5, -1.0, 1.0)
            means[(p, s, 0)], means[(p, s, 1)] = centre + off, centre - off
    utts = []
    for _ in range(n):
        words, segs = _utterance(rng, lex, 2, 12)
        rows, variants = [], []
        for p, d in segs:
            v = int(rng.randint(0, 2))
            variants.append(v)
            first = (d + 1) // 2
            rows += [means[(p, 0, v)]] * first + [means[(p, 1, v)]] * (d - first)
        mel = np.stack(rows) + sigma * rng.randn(len(rows), N_MEL)
        utts.append({"words": words, "mel": mel.T.astype(np.float32), "segments": segs, "variants": variants})
    return lex, utts
