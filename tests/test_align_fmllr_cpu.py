"""CPU: the numpy oracle of the aligner's fMLLR stage (tests/align_fmllr_ref.py) on the multi-speaker corpus of
tests/align_fmllr_corpus.py, the product's host-side update (fastspeech2_amd.align.fmllr_update) against its defining properties
and against the oracle's, and the stability of the oracle's alignment that the GPU end-to-end comparison
(tests/test_align_fmllr_gpu.py) relies on."""
import functools

import numpy as np
import pytest

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_fmllr_corpus as FC
from tests import align_fmllr_ref as FR
from tests import align_lda_ref as LR
from tests import align_ref as R

# the accuracy measurement and the end-to-end comparison on the GPU share one corpus and one schedule: 40 utterances of four
# speakers and one short one of a fifth, 6 passes in x, k = 8 of D_s = 240 (c = 1), 3 passes in z, 2 rounds of fMLLR with 2 passes each
E2E_SEED, E2E_N_UTT, E2E_ITERS, E2E_K, E2E_SPLICE, E2E_LDA_ITERS = 1234, 40, 6, 8, 1, 3
E2E_ROUNDS, E2E_FMLLR_ITERS, E2E_SWEEPS, E2E_MIN_FRAMES = 2, 2, 20, 500
ACC_LDA, ACC_FMLLR = 0.5895, 0.6703


def prepared(lex, utts):
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    return graphs, [R.features(u["mel"]) for u in utts], [u["speaker"] for u in utts], len(ids) * C.STATES


@functools.lru_cache(maxsize=None)
def e2e():
    """(utts, graphs, xs, spk, n_classes, the oracle's model), computed once"""
    lex, utts = FC.corpus(E2E_SEED, E2E_N_UTT)
    graphs, xs, spk, n_classes = prepared(lex, utts)
    model = FR.fit(xs, graphs, spk, n_classes, E2E_ITERS, C.N_MEL, E2E_K, E2E_SPLICE, E2E_LDA_ITERS, E2E_ROUNDS, E2E_FMLLR_ITERS,
                   E2E_SWEEPS, E2E_MIN_FRAMES)
    return utts, graphs, xs, spk, n_classes, model


def random_statistics(rng, D, S=3, N=600, n_cls=5):
    """beta, G, k of S speakers: N frames each, hard posteriors over n_cls diagonal Gaussians, every speaker's frames distorted by
    its own affine map; well conditioned"""
    mu, var = rng.randn(n_cls, D), 0.5 + rng.rand(n_cls, D)
    fs, cs, hs = [], [], []
    for _ in range(S):
        cls = rng.randint(0, n_cls, N)
        fh = mu[cls] + rng.randn(N, D) * np.sqrt(var[cls])
        Am, b = np.eye(D) + 0.3 * rng.randn(D, D) / np.sqrt(D), 0.5 * rng.randn(D)
        fs.append((fh - b) @ np.linalg.inv(Am).T)                          # fh = Am f + b
        cs.append(1.0 / var[cls])
        hs.append(mu[cls] / var[cls])
    return FR.accumulate(fs, cs, hs, list(range(S)), S)


@pytest.mark.parametrize("D", [3, 16, 40])
def test_no_row_step_lowers_the_auxiliary_function(D):
    beta, G, k = random_statistics(np.random.RandomState(D), D)
    S = len(beta)
    W0 = np.tile(np.eye(D, D + 1), (S, 1, 1))
    trace = []
    W, status = A.fmllr_update(beta, G, k, W0, 500.0, 3, trace=trace)
    assert (status == 0).all() and len(trace) == 3 * D and np.array_equal(trace[-1], W)
    prev = np.array([FR.auxiliary(beta[s], G[s], k[s], W0[s]) for s in range(S)])
    first = prev.copy()
    for Wt in trace:
        now = np.array([FR.auxiliary(beta[s], G[s], k[s], Wt[s]) for s in range(S)])
        assert (now >= prev - 1e-12 * np.abs(prev)).all(), (now, prev)
        prev = now
    assert (prev > first).all()


def test_update_recovers_an_exact_affine_image():
    """Frames whose class means and class covariances under the true transform are exactly the model's: the true W is then the
    stationary point of the auxiliary function, and the update finds it from the identity.  The row sweeps converge linearly (on
    these statistics the deviation is 6e-2 after 20 sweeps, 3e-6 after 200, 5e-11 after 400), so this test takes 500."""
    rng = np.random.RandomState(5)
    D, n_cls = 6, 4
    mu, var = rng.randn(n_cls, D), 0.5 + rng.rand(n_cls, D)
    fh, cls = [], []
    for c in range(n_cls):
        for rep in range(1 + c):                                           # unequal occupancies
            for i in range(D):
                for sign in (1.0, -1.0):
                    d = np.zeros(D)
                    d[i] = sign * np.sqrt(D * var[c, i])
                    fh.append(mu[c] + d)
                    cls.append(c)
    fh, cls = np.array(fh), np.array(cls)
    Am, b = np.eye(D) + 0.4 * rng.randn(D, D) / np.sqrt(D), rng.randn(D)
    f = (fh - b) @ np.linalg.inv(Am).T
    beta, G, k = FR.accumulate([f], [1.0 / var[cls]], [mu[cls] / var[cls]], [0], 1)
    W, status = A.fmllr_update(beta, G, k, np.eye(D, D + 1)[None], 1.0, 500)
    err = np.abs(W[0] - np.concatenate([Am, b[:, None]], axis=1)).max()
    print("largest deviation from the true W", err)
    assert status[0] == 0 and err <= 1e-8


def test_speakers_that_keep_their_transform():
    rng = np.random.RandomState(7)
    D = 4
    beta, G, k = random_statistics(rng, D, S=4)
    W0 = np.tile(np.eye(D, D + 1), (4, 1, 1)) + 0.01 * rng.randn(4, D, D + 1)
    beta[1] = 499.0                                                        # under fmllr_min_frames
    G[2, 3] = 0.0                                                          # singular
    G[3, 0] = -G[3, 0]                                                     # not positive definite
    W, status = A.fmllr_update(beta, G, k, W0)
    assert list(status) == [0, 1, 2, 2]
    assert np.array_equal(W[1:], W0[1:]) and not np.array_equal(W[0], W0[0])
    Wr, status_r = FR.update(beta, G, k, W0)
    assert list(status_r) == [0, 1, 2, 2] and np.array_equal(Wr[1:], W0[1:])
    assert A.fmllr_update(beta, G, k, W0, min_frames=1e9)[1].tolist() == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        A.fmllr_update(beta, G[:, :, :-1], k, W0)


@pytest.mark.parametrize("D", [3, 16, 40])
def test_update_agrees_with_the_oracle(D):
    beta, G, k = random_statistics(np.random.RandomState(100 + D), D)
    W0 = np.tile(np.eye(D, D + 1), (len(beta), 1, 1))
    W, status = A.fmllr_update(beta, G, k, W0, 500.0, 20)
    Wr, status_r = FR.update(beta, G, k, W0, 500.0, 20)
    rel = np.abs(W - Wr).max() / np.abs(Wr).max()
    print("D", D, "relative difference", rel)
    assert np.array_equal(status, status_r) and rel <= 1e-10


def test_argument_errors_and_the_batch_budget():
    assert A.max_fmllr_dim() == 64
    frames, states = [900, 100, 500, 500, 40], [300, 40, 200, 180, 20]
    for budget in (1, 2 * 900 * 300 * 17 + 2 * 900 * 160 * 8 + 2 * 300 * 321 * 8, 1 << 30):
        assert list(A.batches_by_bytes(frames, states, 160, budget, fmllr_dim=0)) == list(A.batches_by_bytes(frames, states, 160, budget))
    one = 900 * 300 * 17 + 900 * 160 * 8 + 300 * 321 * 8 + 900 * 3 * 40 * 8
    assert list(A.batches_by_bytes(frames, states, 160, one, fmllr_dim=40))[0] == [0]
    two = 2 * (500 * 200 * 17 + 500 * 160 * 8 + 200 * 321 * 8)               # utterances 2 and 3 together, without c, h and fh
    assert [2, 3] in list(A.batches_by_bytes(frames, states, 160, two)) and [2, 3] not in list(A.batches_by_bytes(frames, states, 160, two, fmllr_dim=40))
    assert [2, 3] in list(A.batches_by_bytes(frames, states, 160, two + 2 * 500 * 3 * 40 * 8, fmllr_dim=40))
    assert "--lda k with k <= 64" in A.fmllr_dim_message(160, 0)


def test_corpus_is_seeded_and_has_the_speakers_the_docstring_says():
    lex, utts = FC.corpus(E2E_SEED, 9)
    lex2, utts2 = FC.corpus(E2E_SEED, 9)
    assert lex == lex2 and all(np.array_equal(a["mel"], b["mel"]) and a["segments"] == b["segments"] for a, b in zip(utts, utts2))
    assert lex == C.corpus(E2E_SEED, 1)[0]                                 # the lexicon of the plain corpus
    assert [u["speaker"] for u in utts] == [0, 1, 2, 3, 0, 1, 2, 3, 0, 4]
    assert len(utts[-1]["words"]) == 3 and utts[-1]["mel"].shape[1] < 200
    M = FC.distortions()
    assert M.shape == (5, C.N_MEL, C.N_MEL) and np.array_equal(M, FC.distortions()) and not np.allclose(M[0], M[1])


def test_schedule_reports_no_drop_after_an_update_and_adapts_the_four_speakers():
    *_, model = e2e()
    hist = model["history"]
    print("log-likelihood per frame", hist)
    assert len(hist) == E2E_ITERS + 1 + E2E_LDA_ITERS + E2E_ROUNDS * (1 + E2E_FMLLR_ITERS) and np.isfinite(hist).all()
    assert model["stat_passes"] == [E2E_ITERS + 1 + E2E_LDA_ITERS + r * (1 + E2E_FMLLR_ITERS) for r in range(E2E_ROUNDS)]
    for p in model["stat_passes"]:
        assert hist[p + 1] >= hist[p], (p, hist[p], hist[p + 1])
    for status in model["status"]:
        assert list(status) == [0, 0, 0, 0, 1]                             # the short speaker stays under fmllr_min_frames
    assert np.array_equal(model["W"][4], np.eye(E2E_K, E2E_K + 1))


def test_fmllr_beats_the_speaker_independent_aligner():
    """Share of the true phone boundaries found within +-1 frame by the oracles on FC.corpus(1234, 40) (EPSILON 1.0), 6 passes in x,
    k = 8, c = 1, 3 passes in z, then 2 rounds of fMLLR with 2 passes each, measured on the host:
        LDA alone 0.5895 (0.6070 with four more passes in z), with fMLLR 0.6703
    fMLLR has to win by half of the measured gap."""
    utts, graphs, xs, spk, n_classes, model = e2e()
    true = [[d for _, d in u["segments"]] for u in utts]
    base = LR.fit(xs, graphs, n_classes, E2E_ITERS, C.N_MEL, E2E_K, E2E_SPLICE, E2E_LDA_ITERS)
    a_lda = C.accuracy(true, [LR.align(x, g, base) for x, g in zip(xs, graphs)], 1)
    a_fmllr = C.accuracy(true, [FR.align(x, g, model, s) for x, g, s in zip(xs, graphs, spk)], 1)
    print("lda", a_lda, "fmllr", a_fmllr)
    assert a_fmllr > a_lda
    assert a_fmllr >= a_lda + 0.5 * (ACC_FMLLR - ACC_LDA), (a_lda, a_fmllr)


def test_oracle_alignment_does_not_move_under_perturbed_transforms():
    """What the exact comparison of frames in tests/test_align_fmllr_gpu.py rests on: for the committed seed, 1e-12 relative noise
    on every entry of every W after every update (far above what separates the kernels' sums from numpy's) moves no boundary of
    the oracle's alignment and moves its reported log-likelihoods by far less than the 1e-9 the GPU test allows."""
    utts, graphs, xs, spk, n_classes, base = e2e()
    rng = np.random.RandomState(1)
    moved = FR.fit(xs, graphs, spk, n_classes, E2E_ITERS, C.N_MEL, E2E_K, E2E_SPLICE, E2E_LDA_ITERS, E2E_ROUNDS, E2E_FMLLR_ITERS,
                   E2E_SWEEPS, E2E_MIN_FRAMES, perturb_W=lambda W: W * (1.0 + 1e-12 * rng.randn(*W.shape)))
    assert not np.array_equal(base["W"], moved["W"])
    rel = np.abs(np.array(moved["history"]) / np.array(base["history"]) - 1.0)
    print("relative change of the log-likelihoods", rel.max())
    assert rel.max() <= 1e-11
    for x, g, s in zip(xs, graphs, spk):
        assert np.array_equal(FR.align(x, g, base, s), FR.align(x, g, moved, s))


def test_oracle_schedule_with_mixtures_and_without_lda():
    lex, utts = FC.corpus(E2E_SEED, 12)
    graphs, xs, spk, n_classes = prepared(lex, utts)
    m = FR.fit(xs, graphs, spk, n_classes, 2, C.N_MEL, 6, 1, 1, 1, 1, 5, 100.0, mixtures=2, mix_iters=1, min_split_occ=20.0)
    assert len(m["history"]) == 2 + 1 + 1 + 1 * (1 + 1) + 1 and np.isfinite(m["history"]).all()
    assert m["gmu"].shape == (n_classes, 2, 6) and m["ncomp"].max() == 2
    assert FR.align(xs[0], graphs[0], m, spk[0]).sum() == len(xs[0])
    xs8 = [np.ascontiguousarray(x[:, :8]) for x in xs]                     # no LDA: the features themselves, here 8 of them
    m = FR.fit(xs8, graphs, spk, n_classes, 2, C.N_MEL, 0, 0, 0, 1, 1, 5, 100.0)
    assert len(m["history"]) == 2 + 1 * (1 + 1) and m["W"].shape == (5, 8, 9)
    assert m["history"][3] >= m["history"][2]
