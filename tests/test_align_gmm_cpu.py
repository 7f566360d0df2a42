"""CPU: the numpy oracle of the aligner's Gaussian-mixture emissions (tests/align_gmm_ref.py) against the single-Gaussian oracle
(tests/align_ref.py) at M = 1 and against its own invariants, and the product's host-side update and split rule
(fastspeech2_amd.align.m_step_gmm, split_classes) against the oracle's."""
import numpy as np
import pytest

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_gmm_corpus as GC
from tests import align_gmm_ref as GR
from tests import align_ref as R

SEED, N_UTT, ITERS = 1234, 12, 3


def prepared(lex, utts):
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    return graphs, [R.features(u["mel"]) for u in utts], len(ids) * C.STATES


@pytest.fixture(scope="module")
def single():
    graphs, xs, n_classes = prepared(*C.corpus(SEED, N_UTT))
    return graphs, xs, n_classes, R.fit(xs, graphs, n_classes, ITERS)


def random_tables(rng, n_classes, M, D, ncomp):
    w, mu, var = np.zeros((n_classes, M)), np.zeros((n_classes, M, D)), np.ones((n_classes, M, D))
    for c, K in enumerate(ncomp):
        w[c, :K] = rng.dirichlet(np.ones(K))
        mu[c, :K], var[c, :K] = 0.3 * rng.randn(K, D), 0.5 + rng.rand(K, D)
    return w, mu, var


def test_one_component_is_the_single_gaussian_oracle_exactly(single):
    graphs, xs, n_classes, (mu, var, history) = single
    w, gmu, gvar, ncomp, ghistory, stages, (smu, svar) = GR.fit(xs, graphs, n_classes, ITERS, mixtures=1)
    assert ghistory == history and stages == [] and (ncomp == 1).all() and (w == 1.0).all()
    assert np.array_equal(gmu[:, 0], mu) and np.array_equal(gvar[:, 0], var)
    assert np.array_equal(smu, mu) and np.array_equal(svar, var)
    for x, g in zip(xs, graphs):
        E, r = GR.emissions(x, g["sid"], w, gmu, gvar)
        assert np.array_equal(E, R.emissions(x, g["sid"], mu, var)) and (r == 1.0).all()
        assert np.array_equal(GR.align(x, g, w, gmu, gvar), R.align(x, g, mu, var))


def test_inactive_components_change_nothing(single):
    """the one-component stage inside wider tables (w = 0, mu = 0, var = 1 beyond K_c = 1) gives the same numbers"""
    graphs, xs, n_classes, (mu, var, history) = single
    _, _, _, _, ghistory, _, (smu, svar) = GR.fit(xs, graphs, n_classes, ITERS, mixtures=3, mix_iters=0)
    assert ghistory == history and np.array_equal(smu, mu) and np.array_equal(svar, var)


@pytest.fixture(scope="module")
def mixture():
    graphs, xs, n_classes = prepared(*GC.corpus(SEED, N_UTT))
    rng = np.random.RandomState(5)
    M = 3
    ncomp = rng.randint(1, M + 1, n_classes)
    w, mu, var = random_tables(rng, n_classes, M, xs[0].shape[1], ncomp)
    w[0, :ncomp[0]] = ([1.0] + [0.0] * (ncomp[0] - 1))                     # active components of weight exactly 0
    return graphs, xs, n_classes, M, ncomp, w, mu, var


def test_responsibilities_sum_to_one_and_partials_sum_to_the_single_ones(mixture):
    graphs, xs, n_classes, M, ncomp, w, mu, var = mixture
    for x, g in zip(xs[:4], graphs[:4]):
        E, r = GR.emissions(x, g["sid"], w, mu, var)
        assert np.isfinite(E).all() and np.abs(r.sum(axis=2) - 1.0).max() <= 1e-12
        assert (r[:, :, 1:][:, g["sid"] == 0] == 0.0).all()                # w = 0 gives exactly 0
        for j, c in enumerate(g["sid"]):
            assert (r[:, j, ncomp[c]:] == 0.0).all()
        gamma = R.posteriors(E, g)[0]
        P, want = GR.partials(gamma, r, x), R.partials(gamma, x)
        assert P.shape == (len(g["sid"]), M, want.shape[1])
        assert np.abs(P.sum(axis=1) - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


def test_weights_stay_a_distribution_through_fit():
    graphs, xs, n_classes = prepared(*GC.corpus(SEED, N_UTT))
    floor = 1e-2 * np.concatenate(xs).var(axis=0)
    w, mu, var, ncomp, history, stages, _ = GR.fit(xs, graphs, n_classes, 2, mixtures=3, mix_iters=2, min_split_occ=20.0)
    assert len(history) == 2 + 2 * 2 and len(stages) == 2 and np.isfinite(history).all()
    assert (stages[0] <= 2).all() and (stages[1] <= 3).all() and (stages[1] >= stages[0]).all() and stages[1].max() == 3
    # every update on the way: replay the last stage's passes
    for it in range(3):
        parts = []
        for x, g in zip(xs, graphs):
            E, r = GR.emissions(x, g["sid"], w, mu, var)
            parts.append(GR.partials(R.posteriors(E, g)[0], r, x))
        sums = GR.class_sums(parts, graphs, n_classes)
        for fn in (GR.update, A.m_step_gmm):
            w2, mu2, var2 = fn(sums, w, mu, var, ncomp, floor)
            assert (w2 >= 0.0).all() and np.abs(w2.sum(axis=1) - 1.0).max() <= 1e-12
            for c in range(n_classes):
                assert (w2[c, ncomp[c]:] == 0.0).all() and (mu2[c, ncomp[c]:] == 0.0).all() and (var2[c, ncomp[c]:] == 1.0).all()
        w, mu, var = GR.update(sums, w, mu, var, ncomp, floor)


def test_host_update_equals_oracle_update():
    rng = np.random.RandomState(3)
    C_, M, D = 6, 4, 5
    ncomp = np.array([4, 1, 2, 3, 2, 4])
    w, mu, var = random_tables(rng, C_, M, D, ncomp)
    sums = np.abs(rng.randn(C_, M, 1 + 2 * D)) + 0.5
    sums[:, :, 1 + D:] += 4.0
    sums[:, :, 0] = [[5.0, 0.2, 1.0, 0.999], [3.0, 0, 0, 0], [0.4, 0.5, 0, 0], [0.0, 7.0, 2.0, 0], [0.6, 0.6, 0, 0], [9.0, 9.0, 0.0, 1.5]]
    sums[3, 1, 1 + D:] = (sums[3, 1, 1:1 + D] / 7.0) ** 2 * 7.0            # zero variance: the floor holds
    floor = np.full(D, 0.01)
    got, want = A.m_step_gmm(sums, w, mu, var, ncomp, floor), GR.update(sums, w, mu, var, ncomp, floor)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    gw, gmu, gvar = got
    assert np.array_equal(gw[2], w[2]) and np.array_equal(gmu[2], mu[2])   # n_c = 0.9 < 1: everything kept
    assert np.allclose(gw[4, :2], 0.5) and np.array_equal(gmu[4], mu[4])   # n_c >= 1 with both components below 1: weights only
    assert gw[3, 0] == 0.0 and np.array_equal(gmu[3, 0], mu[3, 0]) and np.allclose(gvar[3, 1], 0.01)
    assert np.array_equal(A.m_step_gmm(sums.reshape(C_ * M, -1), w, mu, var, ncomp, floor)[1], gmu)   # rows c M + m


def test_split_rule():
    rng = np.random.RandomState(4)
    C_, M, D = 6, 4, 3
    ncomp = np.array([1, 2, 2, 3, 1, 2])
    w, mu, var = random_tables(rng, C_, M, D, ncomp)
    w[1, :2] = 0.5                                                          # a tie: the lower index splits
    w[2, :2] = [0.3, 0.7]
    occ = np.full((C_, M), 100.0)
    occ[4, 0] = 39.9                                                        # below min_split_occ: never splits
    occ[5, 1], w[5, :2] = 100.0, [0.9, 0.1]
    occ[5, 0] = 10.0                                                        # the heaviest component decides, not the fullest
    k = 2                                                                   # target: 3 components
    for fn in (GR.split, A.split_classes):
        w2, mu2, var2, n2 = fn(w, mu, var, ncomp, occ, k, 40.0)
        assert n2.tolist() == [2, 3, 3, 3, 1, 2]
        assert np.abs(w2.sum(axis=1) - 1.0).max() <= 1e-15                  # the class's weight is conserved
        assert np.abs((w2[:, :, None] * mu2).sum(axis=1) - (w[:, :, None] * mu).sum(axis=1)).max() <= 1e-15   # and its mean
        assert w2[1, 0] == 0.25 and w2[1, 2] == 0.25 and w2[1, 1] == 0.5
        assert np.array_equal(mu2[1, 2], mu[1, 0] + 0.2 * np.sqrt(var[1, 0])) and np.array_equal(mu2[1, 0], mu[1, 0] - 0.2 * np.sqrt(var[1, 0]))
        assert np.array_equal(var2[1, 2], var[1, 0]) and np.array_equal(var2[1, 0], var[1, 0]) and np.array_equal(mu2[1, 1], mu[1, 1])
        assert w2[2, 1] == 0.35 and w2[2, 2] == 0.35 and w2[2, 0] == 0.3
        for c in (3, 4, 5):                                                 # full for this step, too empty, heaviest too empty
            assert np.array_equal(w2[c], w[c]) and np.array_equal(mu2[c], mu[c]) and np.array_equal(var2[c], var[c])
    a, b = GR.split(w, mu, var, ncomp, occ, k, 40.0), A.split_classes(w, mu, var, ncomp, occ, k, 40.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    full = A.split_classes(w, mu, var, np.full(C_, M), occ, M, 40.0)        # a full table cannot grow
    assert np.array_equal(full[0], w) and (full[3] == M).all()


def test_batches_by_bytes_default_is_unchanged():
    frames, states = [900, 100, 500, 500, 40], [300, 40, 200, 180, 20]
    for budget in (1, 2 * 900 * 300 * 17 + 2 * 900 * 160 * 8 + 2 * 300 * 321 * 8, 1 << 30):
        assert list(A.batches_by_bytes(frames, states, 160, budget, mixtures=1)) == list(A.batches_by_bytes(frames, states, 160, budget))
    one = 900 * 300 * (17 + 8 * 4) + 900 * 160 * 8 + 300 * 4 * 321 * 8
    assert list(A.batches_by_bytes(frames, states, 160, one, mixtures=4))[0] == [0]
    assert len(list(A.batches_by_bytes(frames, states, 160, 2 * one, mixtures=4))) < len(list(A.batches_by_bytes(frames, states, 160, one, mixtures=4)))


def test_bimodal_corpus_is_seeded_and_bimodal():
    lex, utts = GC.corpus(SEED, 3)
    lex2, utts2 = GC.corpus(SEED, 3)
    assert lex == lex2 and all(np.array_equal(a["mel"], b["mel"]) and a["segments"] == b["segments"] for a, b in zip(utts, utts2))
    for u in utts:
        assert u["mel"].shape == (C.N_MEL, sum(d for _, d in u["segments"])) and len(u["variants"]) == len(u["segments"])
    assert {v for u in utts for v in u["variants"]} == {0, 1}
