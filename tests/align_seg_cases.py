"""Seeded inputs with hand-made segments (independent of any Viterbi pass) that tests/test_align_seg_cpu.py pins and
tests/test_align_seg_gpu.py runs on the GPU, with the oracle's V computed once."""
import functools

import numpy as np

from tests import align_score_cases as K
from tests import align_score_ref as SR
from tests import align_seg_ref as GR

MARGIN = K.MARGIN                                                          # rival is compared where its lead exceeds MARGIN |V|
FRAME_TILE, COLUMN_TILE = 16, 64                                           # SG_FT, SG_CT of csrc/fs2_align_seg.hip
# (S, P, D, M, trained arcs, block-dependent candidates): P S = 1, 63, 64, 66, 3 * 64 + 3 and one state per phone over a full tile
CASES = ((1, 1, 1, 1, False, False), (3, 21, 17, 1, True, False), (2, 32, 40, 3, True, True), (3, 22, 17, 3, False, True),
         (3, 65, 40, 1, True, True), (1, 64, 1, 3, False, False), (2, 33, 1, 1, True, False))
IDS = [f"S{s}-P{p}-D{d}-M{m}-arc{int(a)}-tri{int(t)}" for s, p, d, m, a, t in CASES]


def lengths(S):
    """the segment lengths of the three utterances: S - 1, S, S + 1, the frame tile's edges and several tiles; a 0-frame block
    between two others (with S = 1 that is S - 1 as well)"""
    first = [S + 1, 0, FRAME_TILE - 1, FRAME_TILE, FRAME_TILE + 1] + ([S - 1] if S > 1 else []) + [S, 6]
    return [first, [4 * FRAME_TILE, 4 * FRAME_TILE + 1, 8 * FRAME_TILE + 2], [FRAME_TILE + 1, S, 5]]


def draw(rng, n, classes, ncomp, mu, var):
    """n frames around components of the S classes of one candidate, the states in order"""
    S = len(classes)
    c = np.asarray(classes)[(np.arange(n) * S) // max(n, 1)]
    m = (rng.rand(n) * ncomp[c]).astype(np.int64)
    return mu[c, m] + np.sqrt(var[c, m]) * rng.randn(n, mu.shape[2])


@functools.lru_cache(maxsize=None)
def seg_case(i):
    """-> dict(S, P, fs [(T, D)], seg [(K, 2)], cand [(K, P S)], phone [(K,)] the transcript's phone of every block, w, mu, var, arc,
    want [(V, magnitude)]).  The segments of an utterance partition its frames, so the last one ends at T - 1; the third utterance
    is shorter than the first two, its last block lies outside it (start + frames > T: absent), and one block of the first
    utterance has a -1 among its candidates (absent)."""
    S, P, D, M, arcs, tri = CASES[i]
    rng = np.random.RandomState(500 + i)
    C = P * S + 7
    w, mu, var, ncomp = K.tables(rng, C, D, M)
    loop = rng.uniform(0.1, 0.9, C)
    arc = np.stack([np.log(loop), np.log(1.0 - loop)], 1) if arcs else np.zeros((C, 2))
    fs, segs, cands, phones = [], [], [], []
    for u, ns in enumerate(lengths(S)):
        seg, cand, phone, f, a = [], [], [], [], 0
        for n in ns:
            row = np.arange(P * S, dtype=np.int32)
            if tri:                                                        # the table row of a column depends on the block
                swap = rng.rand(P * S) < 0.3
                row[swap] = rng.randint(0, C, int(swap.sum()))
            true = int(rng.randint(0, P))
            f.append(draw(rng, n, row[true * S:(true + 1) * S], ncomp, mu, var))
            seg.append((a if n else 0, n)), cand.append(row), phone.append(true if rng.rand() < 0.5 else int(rng.randint(0, P)))
            a += n
        if u == 0:
            cand[-1] = cand[-1].copy()                                     # the block of 6 frames
            cand[-1][(P * S) // 2] = -1
        if u == 2:
            seg.append((a - 3, 10)), cand.append(np.arange(P * S, dtype=np.int32)), phone.append(0)
        fs.append(np.concatenate(f)), segs.append(np.array(seg, np.int32)), cands.append(np.array(cand, np.int32))
        phones.append(np.array(phone))
    want = [GR.segment_scores(SR.class_scores(f, w, mu, var), len(f), s, c, arc, S) for f, s, c in zip(fs, segs, cands)]
    return {"S": S, "P": P, "fs": fs, "seg": segs, "cand": cands, "phone": phones, "w": w, "mu": mu, "var": var, "arc": arc, "want": want}


@functools.lru_cache(maxsize=None)
def twin_case(M):
    """65 phones of 3 states (four column tiles, the last one partial); phones 44 and 64 carry the table rows and arcs of phone 2 and
    every segment's frames are drawn around them; the transcript claims another phone -> the case dict of `seg_case` and (lo, twins)"""
    S, P, D, lo, twins = 3, 65, 24, 2, (44, 64)
    rng = np.random.RandomState(900 + M)
    C = P * S
    w, mu, var, ncomp = K.tables(rng, C, D, M)
    loop = rng.uniform(0.1, 0.9, C)
    for q in twins:
        for t in (w, mu, var, ncomp, loop):
            t[q * S:(q + 1) * S] = t[lo * S:(lo + 1) * S]
    arc = np.stack([np.log(loop), np.log(1.0 - loop)], 1)
    ns = [S, FRAME_TILE + 3, 3 * FRAME_TILE]
    row = np.arange(P * S, dtype=np.int32)
    f = np.concatenate([draw(rng, n, row[twins[0] * S:(twins[0] + 1) * S], ncomp, mu, var) for n in ns])
    seg = np.array([(sum(ns[:k]), n) for k, n in enumerate(ns)], np.int32)
    cand = np.tile(row, (len(ns), 1))
    want = [GR.segment_scores(SR.class_scores(f, w, mu, var), len(f), seg, cand, arc, S)]
    return {"S": S, "P": P, "fs": [f], "seg": [seg], "cand": [cand], "phone": [np.array([7, 30, 50])], "w": w, "mu": mu, "var": var,
            "arc": arc, "want": want}, (lo, twins)
