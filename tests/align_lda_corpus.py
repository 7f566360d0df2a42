"""A seeded variant of tests/align_corpus.py with correlated channels, for the aligner's LDA stage: the same lexicon, utterances,
durations and class means (N(0, SEP^2) per dimension), but every frame carries the noise A w, w ~ N(0, I), with one dense mixing
matrix A = SIGMA (I + (GAIN - 1) Q Q^T) shared by all classes: Q holds RANK orthonormal dense directions (a fixed seed, the same
for every corpus seed), so A has RANK singular values GAIN SIGMA and N_MEL - RANK equal to SIGMA.  The loud directions carry next
to no class information (the class means have SEP in them, like anywhere else, under GAIN SIGMA of noise), but being dense they
raise the variance of every channel to SIGMA^2 (1 + RANK (GAIN^2 - 1) / N_MEL) and make the channels' errors move together.  A
diagonal Gaussian charges that shared noise once per channel and the directions that do tell two phones apart drown in it; a
transform that whitens the within-class covariance leaves the loud directions one unit of variance each and keeps
SEP^2 / SIGMA^2 per quiet direction.  SEP and the spectrum of A were chosen on the host with the numpy oracles (tests/align_ref.py,
tests/align_lda_ref.py): the measured accuracies are in tests/test_align_lda_cpu.py and DESIGN.md."""
import numpy as np

from tests.align_corpus import N_MEL, PHONES, STATES, _utterance, lexicon

SIGMA, SEP, RANK, GAIN = 1.0, 0.5, 4, 8.0


def mixing(rank=RANK, gain=GAIN, sigma=SIGMA):
    """A (N_MEL, N_MEL): the same for every corpus seed"""
    Q = np.linalg.qr(np.random.RandomState(20240).randn(N_MEL, rank))[0]
    return sigma * (np.eye(N_MEL) + (gain - 1.0) * Q @ Q.T)


def corpus(seed, n, sep=None, rank=None, gain=None, sigma=None):
    """-> (lexicon, [dict(words, mel (80, T) float32, segments)])"""
    sep, rank = SEP if sep is None else sep, RANK if rank is None else rank
    A = mixing(rank, GAIN if gain is None else gain, SIGMA if sigma is None else sigma)
    rng = np.random.RandomState(seed)
    lex = lexicon(rng)
    means = {(p, s): sep * rng.randn(N_MEL) for p in PHONES + ["sil", "sp"] for s in range(STATES)}
    utts = []
    for _ in range(n):
        words, segs = _utterance(rng, lex, 2, 12)
        rows = []
        for p, d in segs:
            first = (d + 1) // 2
            rows += [means[(p, 0)]] * first + [means[(p, 1)]] * (d - first)
        mel = np.stack(rows) + rng.randn(len(rows), N_MEL) @ A.T
        utts.append({"words": words, "mel": mel.T.astype(np.float32), "segments": segs})
    return lex, utts
