"""No GPU: the speaker-similarity oracle tests/spk_ref.py against things it shares no code with (direct Gaussian densities, brute
force, hand-worked answers), the host-side report of fastspeech2_amd/speaker.py against the oracle's, and the committed bars
against the script that writes them."""
import json

import numpy as np
import pytest

from tests import spk_corpus as SC
from tests import spk_ref as R
from tests.golden import make_spk_bars as MB

LD = np.longdouble


def test_expanded_score_is_the_gaussian_log_density():
    rng = np.random.RandomState(0)
    x, w, mu, var = rng.randn(7, 5), rng.rand(3) + 0.1, rng.randn(3, 5), 0.5 + rng.rand(3, 5)
    w /= w.sum()
    L = R.comp_scores(x, *R.tables(w, mu, var, LD), LD)
    xl, ml, vl = x.astype(LD), mu.astype(LD), var.astype(LD)
    direct = np.log(w.astype(LD))[None] + (-((xl[:, None] - ml[None]) ** 2) / (2 * vl[None]) - np.log(2 * LD(np.pi) * vl[None]) / 2).sum(-1)
    assert np.abs(L - direct).max() < 1e-15 * np.abs(direct).max()        # pi is a double in `direct`: 1e-16 relative
    assert R.tables(np.array([0.0, 1.0]), mu[:2], var[:2])[2][0] == -np.inf


@pytest.mark.parametrize("M", [1, 2, 3])
def test_lse_against_brute_force(M):
    rng = np.random.RandomState(M)
    L = 5 * rng.randn(9, M)
    brute = np.array([np.log(sum(np.exp(LD(v)) for v in row)) for row in L])
    assert np.abs(R.lse(L, LD) - brute).max() < 1e-17 * 50
    assert (R.lse(np.full((2, M), -np.inf)) == -np.inf).all()
    assert (R.posteriors(np.full((2, M), -np.inf), np.full(2, -np.inf)) == 0).all()
    p = R.posteriors(L, R.lse(L))
    assert np.abs(p.sum(1) - 1).max() < 1e-14


def test_a_model_against_itself_scores_zero_exactly():
    rng = np.random.RandomState(3)
    X = rng.randn(40, 4)
    ubm = R.fit_ubm(X, 4, 2)
    llr, _ = R.llr_matrix(X, [0, 25], [25, 15], ubm, [ubm["mu"], ubm["mu"]])
    assert (llr == 0).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_em_never_lowers_the_training_likelihood(seed):
    rng = np.random.RandomState(seed)
    X = np.concatenate([rng.randn(150, 3) + c for c in (0, 3, -3)])
    fit = R.fit_ubm(X, 8, 4, min_occ=0.0)
    assert len(fit["history"]) == 3 and [len(h) for h in fit["history"]] == [4, 4, 5]
    for stage in fit["history"]:
        assert all(b >= a - 1e-12 for a, b in zip(stage, stage[1:])), stage
    assert abs(fit["w"].sum() - 1) < 1e-12 and (fit["var"] >= 0.01 * X.var(0) * (1 - 1e-12)).all()


def test_low_occupancy_is_reseeded_from_the_heaviest():
    stats = np.array([[10.0, 10.0, 20.0], [0.5, 0.0, 0.0], [5.0, -5.0, 10.0]])
    w, mu, var = R.em_update(stats, 15.5, np.ones(3) / 3, np.zeros((3, 1)), np.ones((3, 1)), np.array([0.01]), 3.0)
    sd = 1.0                                                               # component 0: mean 1, variance 20 / 10 - 1 = 1
    assert mu[0, 0] == 1 + 0.2 * sd and mu[1, 0] == 1 - 0.2 * sd and var[1, 0] == var[0, 0] == 1.0
    assert w[0] == w[1] and abs(w.sum() - 1) < 1e-15


def test_map_limits():
    rng = np.random.RandomState(4)
    mu = rng.randn(3, 2)
    stats = np.concatenate([np.array([[4.0], [0.0], [2.5]]), rng.randn(3, 4)], 1)
    ex = stats[:, 1:3] / np.array([[4.0], [1.0], [2.5]])
    tiny = R.map_means(stats, mu, 1e-300)
    assert np.allclose(tiny[[0, 2]], ex[[0, 2]], rtol=1e-15, atol=0) and (tiny[1] == mu[1]).all()    # n_m = 0 keeps the UBM mean
    assert np.abs(R.map_means(stats, mu, 1e12) - mu).max() < 1e-10
    half = R.map_means(stats, mu, 4.0)
    assert np.allclose(half[0], 0.5 * ex[0] + 0.5 * mu[0], rtol=1e-15)


def test_deltas_of_a_ramp():
    c = 3.0 * np.arange(9)[:, None] + np.array([[1.0, 2.0]])
    d = R.deltas(c)
    assert (d[2:-2] == 3.0).all()
    # clamped: t = 0: (c1 - c0) + 2 (c2 - c0) = 15 over 10; t = 1: (c2 - c0) + 2 (c3 - c0) = 24 over 10
    assert np.allclose(d[0], 1.5) and np.allclose(d[1], 2.4) and np.allclose(d[-1], 1.5) and np.allclose(d[-2], 2.4)
    assert (R.deltas(np.ones((1, 2))) == 0).all()


def test_feature_selection_and_the_zero_variance_rule():
    rng = np.random.RandomState(5)
    cep = rng.randn(12, 4)
    cep[:, 0] = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -9.9, -10.1]
    f = R.features(cep, 10.0)
    assert f["n_kept"] == 11 and not f["keep"][11] and f["keep"][10]
    assert np.abs(f["x"].mean(0)).max() < 1e-14 and np.abs((f["x"] ** 2).mean(0) - 1).max() < 1e-13
    cep[:, 0] = [5] + [-20] * 11                                           # one frame passes: fewer than 2 keep none
    assert R.features(cep, 10.0)["n_kept"] == 0
    const = np.ones((8, 4))                                                # a constant utterance: variance 0, keeps none
    out = R.features(const, 10.0)
    assert out["n_kept"] == 0 and (out["var"] == 0).all() and out["x"].shape == (0, 6)
    assert R.features(np.zeros((0, 4)), 10.0)["n_kept"] == 0
    assert abs(R.default_energy_floor(80) - np.sqrt(80) * np.log(10 ** 1.5)) < 1e-12


def test_eer_on_hand_made_lists():
    from fastspeech2_amd import speaker as S
    for fn in (R.eer, S.equal_error_rate):
        assert fn([2, 3], [0, 1]) == 0.0                                   # perfect separation
        assert fn([0, 1], [0, 1]) == 0.5                                   # the same distribution
        # targets 1 3 4 5, non-targets 0 2: at threshold 2 (FRR, FAR) = (1/4, 1/2), at 3 (1/4, 0): d = -1/4, +1/4, t = 1/2 -> 1/4
        assert fn([1, 3, 4, 5], [0, 2]) == 0.25
        # targets 1 2 4, non-targets 0 3: at 2 (1/3, 1/2), at 3 (2/3, 1/2): t = 1/2 -> 1/3 + 1/6
        assert abs(fn([1, 2, 4], [0, 3]) - 0.5) < 1e-15
        assert fn([], [1.0]) is None
    rng = np.random.RandomState(6)
    for _ in range(20):
        t, n = np.round(rng.randn(9), 1), np.round(rng.randn(14) - 0.5, 1)
        assert abs(R.eer(t, n) - S.equal_error_rate(t, n)) < 1e-15


def test_rank_ties_go_to_the_lower_index():
    from fastspeech2_amd import speaker as S
    row = np.array([1.0, 2.0, 2.0, 0.5, 2.0])
    assert [R.rank_of(row, g) for g in range(5)] == [4, 1, 2, 5, 3]
    for g in range(5):
        rank, rival, margin = S.rank_and_rival(row, g)
        assert rank == R.rank_of(row, g) and rival == R.rival_of(row, g)
    assert S.rank_and_rival(row, 1)[1:] == (2, 0.0) and S.rank_and_rival(row, 2)[1:] == (1, 0.0)
    assert S.rank_and_rival(np.array([3.0]), 0) == (1, None, None)


def test_host_tables_match_the_oracle():
    from fastspeech2_amd import speaker as S
    rng = np.random.RandomState(7)
    w, mu, var = np.array([0.25, 0.0, 0.75]), rng.randn(3, 4), 0.5 + rng.rand(3, 4)
    for got, want in zip(S.expand(w, mu, var), R.tables(w, mu, var, LD)):
        fin = np.isfinite(want)
        assert (got[~fin] == want[~fin]).all() and np.abs(got[fin] - want[fin]).max() < 1e-14 * np.abs(want[fin]).max()
    assert np.abs(S.dct_table0(80, 5) - R.dct_rows(80, 5)).max() < 1e-15
    assert abs(S.default_energy_floor(80) - R.default_energy_floor(80)) < 1e-12


def test_committed_bars_are_what_the_script_measures():
    bars = json.load(open(MB.PATH))
    rho_lse, rho_post = MB.measure_rho()
    assert bars["rho_lse"] == rho_lse and bars["rho_post"] == rho_post and 0 < rho_lse < 1 and 0 < rho_post < 1
    run = MB.pipeline(SC.SEEDS[0])
    rec = bars["seeds"][str(SC.SEEDS[0])]
    assert abs(run["report"]["accuracy"] - rec["accuracy"]) < 1e-12 and abs(run["report"]["eer"] - rec["eer"]) < 1e-12
    assert all(r["accuracy"] == 1.0 for r in bars["seeds"].values())      # the oracle identifies every held-out utterance
    assert min(bars["candidates"][str(SC.EPSILON)]) == 1.0 and all(min(v) < 1.0 for k, v in bars["candidates"].items() if float(k) < SC.EPSILON)
    assert bars["accuracy_bar"] == 1.0 - 1.0 / (SC.N_HELD * SC.N_SPEAKERS) and bars["eer_bar"] == max(r["eer"] for r in bars["seeds"].values()) + 0.02
    for r in bars["seeds"].values():                                       # the known answers hold for the oracle
        b = r["blend_target_llr"]
        assert b[0] > b[1] > b[2] and r["blend_rank_b_at_1"] == 1 and r["llr_at_r_1e12"] < 1e-8
