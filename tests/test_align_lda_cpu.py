"""CPU: the numpy oracle of the aligner's LDA stage (tests/align_lda_ref.py) on the correlated-channel corpus of
tests/align_lda_corpus.py, the product's host-side transform (fastspeech2_amd.align.lda_transform) against its defining properties
and against the oracle's, the splice rule at the edges, the argument checks, and the stability of the oracle's alignment that the
GPU end-to-end comparison (tests/test_align_lda_gpu.py) relies on."""
import numpy as np
import pytest

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_lda_corpus as LC
from tests import align_lda_ref as LR
from tests import align_ref as R

# the accuracy measurement: 30 utterances, 6 passes in x, k = 16 of D_s = 240 (c = 1), 3 passes in z
ACC_SEEDS, ACC_N_UTT, ACC_ITERS, ACC_K, ACC_SPLICE, ACC_LDA_ITERS = (1234, 1235, 1236), 30, 6, 16, 1, 3
ACC_SINGLE = {1234: 0.4707, 1235: 0.4896, 1236: 0.4821}
ACC_LDA = {1234: 0.8608, 1235: 0.8668, 1236: 0.8512}
# the end-to-end comparison on the GPU
E2E_SEED, E2E_N_UTT, E2E_ITERS, E2E_K, E2E_SPLICE, E2E_LDA_ITERS = 1234, 40, 6, 8, 1, 3


def prepared(lex, utts):
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    return graphs, [R.features(u["mel"]) for u in utts], len(ids) * C.STATES


@pytest.mark.parametrize("seed", ACC_SEEDS)
def test_lda_beats_the_single_gaussians_on_correlated_channels(seed):
    """Share of the true phone boundaries found within +-1 frame by the two oracles on LC.corpus(seed, 30) (SEP 0.5, SIGMA 1, four
    dense directions of gain 8), 6 passes in x, then k = 16, c = 1 and 3 passes in z, measured on the host:
        seed 1234: single Gaussians 0.4707, LDA 0.8608
        seed 1235: single Gaussians 0.4896, LDA 0.8668
        seed 1236: single Gaussians 0.4821, LDA 0.8512
    The smallest gap is 0.3691 (seed 1236); LDA has to win by half of it, because the gap varies by seed."""
    gap = min(ACC_LDA[s] - ACC_SINGLE[s] for s in ACC_SEEDS)
    assert abs(gap - 0.3691) < 1e-9
    lex, utts = LC.corpus(seed, ACC_N_UTT)
    graphs, xs, n_classes = prepared(lex, utts)
    true = [[d for _, d in u["segments"]] for u in utts]
    mu, var, _ = R.fit(xs, graphs, n_classes, ACC_ITERS)
    a_single = C.accuracy(true, [R.align(x, g, mu, var) for x, g in zip(xs, graphs)], 1)
    model = LR.fit(xs, graphs, n_classes, ACC_ITERS, C.N_MEL, ACC_K, ACC_SPLICE, ACC_LDA_ITERS)
    a_lda = C.accuracy(true, [LR.align(x, g, model) for x, g in zip(xs, graphs)], 1)
    print("seed", seed, "single", a_single, "lda", a_lda, "eigenvalues", model["eig"])
    assert len(model["history"]) == ACC_ITERS + 1 + ACC_LDA_ITERS and np.isfinite(model["history"]).all()
    assert a_lda >= a_single + 0.5 * gap, (a_single, a_lda)


def random_statistics(rng, C_=7, Ds=12, N=400):
    """class sums and totals of N frames spread over C_ classes, one of them with less than one frame of mass"""
    means = rng.randn(C_, Ds)
    mix = rng.randn(Ds, Ds) * 0.3 + np.eye(Ds)
    gamma = rng.dirichlet(0.3 * np.ones(C_ - 1), N)
    gamma = np.concatenate([gamma * (1 - 1e-3 / N), np.full((N, 1), 1e-3 / N)], axis=1)     # the last class: 1e-3 frames
    y = gamma @ means + rng.randn(N, Ds) @ mix.T + 3.0
    return gamma.sum(axis=0), gamma.T @ y, N, y.sum(axis=0), y.T @ y


def test_transform_properties():
    rng = np.random.RandomState(11)
    n, a, N, s, S = random_statistics(rng)
    Ds, k = len(s), 5
    m, S_T, S_B, S_W = LR.scatter_matrices(n, a, N, s, S)
    P, o, eig = A.lda_transform(n, a, N, s, S, k)
    assert P.shape == (k, Ds) and o.shape == (k,) and eig.shape == (k,)
    assert np.abs(P @ S_W @ P.T - np.eye(k)).max() <= 1e-9                 # the within-class covariance of z is the identity
    B = P @ S_B @ P.T
    assert np.abs(B - np.diag(np.diag(B))).max() <= 1e-9 and np.abs(np.diag(B) - eig).max() <= 1e-9
    assert (np.diff(eig) <= 0.0).all() and eig[-1] > 0.0                   # descending
    full = A.lda_transform(n, a, N, s, S, Ds)[2]
    assert np.abs(full[:k] - eig).max() <= 1e-9 and full[k] <= eig[-1]     # and the k largest
    assert np.abs(o - P @ m).max() <= 1e-9
    for row in P:                                                          # the sign rule
        assert row[np.argmax(np.abs(row))] > 0.0
    order = rng.permutation(len(n))                                        # the order of the classes does not matter
    P2, o2, eig2 = A.lda_transform(n[order], a[order], N, s, S, k)
    assert np.abs(P2 - P).max() <= 1e-9 and np.abs(o2 - o).max() <= 1e-9 and np.abs(eig2 - eig).max() <= 1e-9
    n0, a0 = n.copy(), a.copy()                                            # a class with n < 1 is left out whatever its sums hold
    a0[-1] = 1e6
    assert np.array_equal(A.lda_transform(n0, a0, N, s, S, k)[0], P)
    Pr, orr, eigr = LR.transform(n, a, N, s, S, k)                         # the oracle takes another route to the same transform
    assert np.abs(Pr - P).max() <= 1e-9 and np.abs(orr - o).max() <= 1e-9 and np.abs(eigr - eig).max() <= 1e-9


@pytest.mark.parametrize("T,c", [(1, 1), (1, 4), (2, 1), (2, 3), (3, 3), (4, 4), (9, 2)])
def test_splice_edge_rule(T, c):
    n_mel = 3
    x = np.arange(T * 2 * n_mel, dtype=np.float64).reshape(T, 2 * n_mel) + 1.0
    y = LR.splice(x, n_mel, c)
    assert y.shape == (T, n_mel * (2 * c + 1))
    for t in range(T):
        for p in range(-c, c + 1):
            src = min(max(t + p, 0), T - 1)
            assert np.array_equal(y[t, (p + c) * n_mel:(p + c + 1) * n_mel], x[src, :n_mel])
    if T == 1:
        assert np.array_equal(y, np.tile(x[:, :n_mel], (1, 2 * c + 1)))    # one frame: 2 c + 1 copies of it
    assert np.array_equal(y[:, c * n_mel:(c + 1) * n_mel], x[:, :n_mel])   # the centre is the frame itself, deltas are not spliced


def test_argument_errors():
    assert A.max_splice_dim() == 720
    assert A.splice_dim(80, 3) == 560 and A.splice_dim(80, 4, 720) == 720 and A.splice_dim(80, 0, 1) == 80
    for n_mel, c, k in ((80, 1, 241), (80, 1, 0), (80, 5, 8), (80, -1, 8), (81, 4, 8), (0, 1, None)):   # k > D_s, c = 5, D_s > 720
        with pytest.raises(ValueError):
            A.splice_dim(n_mel, c, k)
    n, a, N, s, S = random_statistics(np.random.RandomState(0))
    for k in (0, len(s) + 1):
        with pytest.raises(ValueError):
            A.lda_transform(n, a, N, s, S, k)
    with pytest.raises(ValueError):
        A.lda_transform(n, a[:, :-1], N, s, S, 2)


def test_batches_by_bytes_budgets_for_the_spliced_frames():
    frames, states = [900, 100, 500, 500, 40], [300, 40, 200, 180, 20]
    for budget in (1, 2 * 900 * 300 * 17 + 2 * 900 * 160 * 8 + 2 * 300 * 321 * 8, 1 << 30):
        assert list(A.batches_by_bytes(frames, states, 160, budget, splice_dim=0)) == list(A.batches_by_bytes(frames, states, 160, budget))
    one = 900 * 300 * 17 + 900 * 160 * 8 + 300 * 321 * 8 + 900 * 560 * 8 + 300 * 1121 * 8
    assert list(A.batches_by_bytes(frames, states, 160, one, splice_dim=560))[0] == [0]
    assert len(list(A.batches_by_bytes(frames, states, 160, one, splice_dim=560))) > len(list(A.batches_by_bytes(frames, states, 160, one)))


def test_corpus_is_seeded_and_its_noise_is_what_the_docstring_says():
    lex, utts = LC.corpus(E2E_SEED, 3)
    lex2, utts2 = LC.corpus(E2E_SEED, 3)
    assert lex == lex2 and all(np.array_equal(a["mel"], b["mel"]) and a["segments"] == b["segments"] for a, b in zip(utts, utts2))
    assert lex == C.corpus(E2E_SEED, 1)[0]                                 # the lexicon of the plain corpus
    sv = np.linalg.svd(LC.mixing(), compute_uv=False)
    assert np.allclose(sv[:LC.RANK], LC.GAIN * LC.SIGMA) and np.allclose(sv[LC.RANK:], LC.SIGMA)
    assert np.array_equal(LC.mixing(), LC.mixing())


def test_oracle_schedule_with_mixtures_runs_on_z():
    graphs, xs, n_classes = prepared(*LC.corpus(E2E_SEED, 12))
    m = LR.fit(xs, graphs, n_classes, 2, C.N_MEL, 6, 1, 1, mixtures=2, mix_iters=1, min_split_occ=20.0)
    assert len(m["history"]) == 2 + 1 + 1 + 1 and np.isfinite(m["history"]).all()
    assert m["gmu"].shape == (n_classes, 2, 6) and m["ncomp"].max() == 2
    assert np.abs(m["w"].sum(axis=1) - 1.0).max() <= 1e-12
    fr = LR.align(xs[0], graphs[0], m)
    assert fr.sum() == len(xs[0])


def test_oracle_alignment_does_not_move_under_a_perturbed_transform():
    """What the exact comparison of frames in tests/test_align_lda_gpu.py rests on: for the committed seed, 1e-12 relative noise on
    every entry of P (far above what separates the kernels' sums from numpy's) moves no boundary of the oracle's alignment and
    moves its log-likelihoods by far less than the 1e-9 the GPU test allows."""
    graphs, xs, n_classes = prepared(*LC.corpus(E2E_SEED, E2E_N_UTT))
    args = (xs, graphs, n_classes, E2E_ITERS, C.N_MEL, E2E_K, E2E_SPLICE, E2E_LDA_ITERS)
    base = LR.fit(*args)
    rng = np.random.RandomState(1)
    moved = LR.fit(*args, perturb_P=lambda P: P * (1.0 + 1e-12 * rng.randn(*P.shape)))
    assert not np.array_equal(base["P"], moved["P"])
    rel = np.abs(np.array(moved["history"]) / np.array(base["history"]) - 1.0)
    print("relative change of the log-likelihoods", rel.max(), "eigenvalues", base["eig"])
    assert rel.max() <= 1e-11
    for x, g in zip(xs, graphs):
        assert np.array_equal(LR.align(x, g, base), LR.align(x, g, moved))
    assert np.diff(base["eig"]).max() < 0.0 and base["eig"][-1] > 0.05     # distinct, well above the null space of S_B
