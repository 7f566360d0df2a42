"""Seeded inputs that tests/test_align_score_cpu.py pins and tests/test_align_score_gpu.py runs on the GPU: the ragged batches of
the frame-score comparison and the substituted-transcript cases."""
import functools

import numpy as np

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_ref as R
from tests import align_score_ref as SR

FRAME_TILE, CLASS_TILE = 64, 64                                            # SC_FT, SC_CT of csrc/fs2_align_score.hip
LENS = (1, 31, 32, 33, 70, FRAME_TILE - 1, FRAME_TILE, FRAME_TILE + 1, 2 * FRAME_TILE + 3)
# (classes, dimensions, components): every value the kernel's tiles and the feature chunk of 16 make special, and three class tiles
SHAPES = ((1, 1, 1), (33, 33, 3), (67, 40, 8), (CLASS_TILE - 1, 160, 1), (CLASS_TILE, 40, 3), (CLASS_TILE + 1, 33, 8), (67, 160, 3),
          (33, 1, 8), (2 * CLASS_TILE + 7, 16, 1), (CLASS_TILE, 17, 1))
MARGIN = 1e-6                                                              # arg is compared where best - runner-up > MARGIN |best|


def tables(rng, n_classes, D, M):
    """mixture tables with ragged component counts: inactive components are w = 0, mu = 0, var = 1"""
    ncomp = rng.randint(1, M + 1, n_classes)
    active = np.arange(M)[None, :] < ncomp[:, None]
    w = np.where(active, rng.uniform(0.2, 1.0, (n_classes, M)), 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    mu = np.where(active[:, :, None], rng.randn(n_classes, M, D), 0.0)
    var = np.where(active[:, :, None], rng.uniform(0.5, 2.0, (n_classes, M, D)), 1.0)
    return w, mu, var, ncomp


@functools.lru_cache(maxsize=None)
def frame_case(i):
    """-> (fs [(T, D)], cls [(T,)], w, mu, var, oracle [(own, best, arg, margin)]) of SHAPES[i]: every frame is drawn around a
    component of some class; cls is another draw, so own is the best in about half the frames"""
    n_classes, D, M = SHAPES[i]
    rng = np.random.RandomState(100 + i)
    w, mu, var, ncomp = tables(rng, n_classes, D, M)
    fs, cs, want = [], [], []
    for T in LENS:
        c = rng.randint(0, n_classes, T)
        m = (rng.rand(T) * ncomp[c]).astype(np.int64)
        f = mu[c, m] + np.sqrt(var[c, m]) * rng.randn(T, D)
        cls = np.where(rng.rand(T) < 0.5, c, rng.randint(0, n_classes, T)).astype(np.int32)
        fs.append(f), cs.append(cls)
        want.append(SR.frame_scores(SR.class_scores(f, w, mu, var), cls))
    return fs, cs, w, mu, var, want


# ------------------------------------------------------------------ substituted transcripts
SEED, N_UTT, ITERS, K = 1234, 24, 4, 8


def substitute(rng, words, lex):
    """one inner word replaced by a lexicon word that shares no phone with it -> (words, index of the word)"""
    i = int(rng.randint(1, len(words) - 1))
    others = [v for v in sorted(lex) if not set(lex[v]) & set(lex[words[i]])]
    return words[:i] + [others[int(rng.randint(0, len(others)))]] + words[i + 1:], i


@functools.lru_cache(maxsize=None)
def substitution():
    """-> (mu, var (C, D), n_classes, [(x, true graph, substituted graph, blocks of the substituted word, blocks of the other
    words)]): a table trained on the true transcripts, K utterances with one inner word replaced"""
    lex, utts = C.corpus(SEED, N_UTT)
    ids = A.phone_table(lex)
    n_classes = len(ids) * C.STATES
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    mu, var, _ = R.fit(xs, graphs, n_classes, ITERS)
    rng = np.random.RandomState(SEED + 1)
    cases = []
    for u, x, g in zip(utts[:K], xs, graphs):
        words, i = substitute(rng, u["words"], lex)
        gs = A.utterance_graph(words, lex, ids, C.STATES)
        sub = [k for k, b in enumerate(gs["blocks"]) if b[1] == i]
        rest = [k for k, b in enumerate(gs["blocks"]) if b[1] >= 0 and b[1] != i]
        cases.append((x, g, gs, sub, rest))
    return mu, var, n_classes, cases
