"""A seeded multi-speaker variant of tests/align_lda_corpus.py, for the aligner's fMLLR stage: the same lexicon, utterances,
durations, class means and correlated noise, but utterance u belongs to speaker u mod N_SPEAKERS and every frame of speaker s passes
through that speaker's own fixed dense matrix M_s = I + EPSILON R_s (R_s has N(0, 1 / N_MEL) entries, a fixed seed, the same for
every corpus seed): a speaker-specific linear distortion of the channels.  A constant shift per speaker would not do: the
per-utterance mean removal of the feature step cancels it.  One extra speaker (index N_SPEAKERS) has a single utterance of three
words, under 200 frames, so that it stays below `fmllr_min_frames` and keeps the identity.  A speaker-independent Gaussian has to
cover all the images M_s mean of a class at once; one affine transform per speaker can bring them back together.  EPSILON and the
utterance count were chosen on the host with the numpy oracles (tests/align_lda_ref.py, tests/align_fmllr_ref.py): the measured
accuracies are in tests/test_align_fmllr_cpu.py and DESIGN.md."""
import numpy as np

from tests.align_corpus import N_MEL, PHONES, STATES, _utterance, lexicon
from tests.align_lda_corpus import SEP, mixing

N_SPEAKERS, EPSILON = 4, 1.0


def distortions(epsilon=EPSILON):
    """M (N_SPEAKERS + 1, N_MEL, N_MEL): the same for every corpus seed"""
    rng = np.random.RandomState(4242)
    return np.eye(N_MEL)[None] + epsilon * rng.randn(N_SPEAKERS + 1, N_MEL, N_MEL) / np.sqrt(N_MEL)


def corpus(seed, n, epsilon=None):
    """-> (lexicon, [dict(words, mel (80, T) float32, segments, speaker)]): n utterances of the N_SPEAKERS speakers in turn, then the
    one short utterance of the extra speaker"""
    A, M = mixing(), distortions(EPSILON if epsilon is None else epsilon)
    rng = np.random.RandomState(seed)
    lex = lexicon(rng)
    means = {(p, s): SEP * rng.randn(N_MEL) for p in PHONES + ["sil", "sp"] for s in range(STATES)}
    utts = []
    for u in range(n + 1):
        words, segs = _utterance(rng, lex, 2, 12)
        while u == n and len(words) != 3:                                  # the extra speaker's utterance is short
            words, segs = _utterance(rng, lex, 2, 12)
        speaker = u % N_SPEAKERS if u < n else N_SPEAKERS
        rows = []
        for p, d in segs:
            first = (d + 1) // 2
            rows += [means[(p, 0)]] * first + [means[(p, 1)]] * (d - first)
        mel = (np.stack(rows) + rng.randn(len(rows), N_MEL) @ A.T) @ M[speaker].T
        utts.append({"words": words, "mel": mel.T.astype(np.float32), "segments": segs, "speaker": speaker})
    return lex, utts
