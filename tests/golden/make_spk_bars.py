"""Writes tests/golden/spk_bars.json: what the speaker-similarity tests (tests/test_spk_cpu.py, tests/test_spk_gpu.py) hold the GPU to
beyond the derived bounds of tests/spk_ref.py.  Run from the repository root: python -m tests.golden.make_spk_bars

  rho_lse, rho_post   the exp / log share of the bounds.  On every kernel test shape and seed below the scores L are taken from the
                      longdouble oracle, rounded to fp64 and pushed through the fp64 restatement of lse and of the posteriors; the
                      worst |fp64 - longdouble| / T (T as in spk_ref's docstring) is recorded.  A GPU test allows 2 P + 4 rho T.
  e2e                 the oracle pipeline on the corpus of tests/spk_corpus.py for the seeds 4321, 17, 99: accuracy, EER and final
                      log-likelihood per frame per seed; accuracy_bar = the worst accuracy minus one utterance, eer_bar = the worst
                      EER + 0.02.  `candidates` shows the distortion strengths tried: EPSILON is the smallest at which every
                      held-out utterance is identified on all three seeds.
  ll_tol, mean_tol    how far the final log-likelihood per frame and the component means (nearest neighbour, Euclidean) move when
                      the training frames are perturbed by 1e-9 relative noise: a million times a rounding error, so a GPU run that
                      differs from the oracle only by roundings stays well inside; both are floored at 1e-9."""
import json
import os

import numpy as np

from tests import spk_corpus as SC
from tests import spk_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "spk_bars.json")
# (N, D, M, G): every N in {0, 1, 15, 16, 17, 63, 64, 65, 130}, D in {1, 2, 13, 38, 64}, M in {1, 3, 16, 17, 64, 65, 257}, G in {1, 2, 5}
LOGLIK_SHAPES = [(0, 13, 16, 1), (1, 1, 1, 1), (15, 2, 3, 2), (16, 13, 16, 5), (17, 38, 17, 1), (63, 64, 64, 2), (64, 38, 65, 1),
                 (65, 13, 257, 2), (130, 64, 257, 1), (130, 38, 64, 5), (65, 1, 65, 5), (17, 2, 1, 5), (64, 64, 1, 1), (130, 13, 3, 1)]
# (N, D, M): N = 16, 17 one and two chunks, 511 thirty-two, 513 seventeen with a last chunk of one row
ACCUM_SHAPES = [(0, 13, 16), (1, 1, 1), (16, 2, 3), (17, 38, 17), (511, 64, 64), (513, 38, 65), (513, 13, 257), (17, 64, 65), (511, 1, 16)]


def draw_mixture(rng, G, M, D):
    """tables of G groups of M components: means within the data's range, variances in [0.5, 2], random weights"""
    a, b, c = [], [], []
    for _ in range(G):
        w = rng.rand(M) + 0.1
        t = R.tables(w / w.sum(), 1.5 * rng.randn(M, D), 0.5 + 1.5 * rng.rand(M, D), np.longdouble)
        for lst, v in zip((a, b, c), t):
            lst.append(np.asarray(v, np.float64))
    return np.concatenate(a), np.concatenate(b), np.concatenate(c)


def loglik_case(i):
    """-> (x (N, D), a, b (G M, D), c (G M,), G) of LOGLIK_SHAPES[i], float64, seeded by i"""
    N, D, M, G = LOGLIK_SHAPES[i]
    rng = np.random.RandomState(1000 + i)
    return (rng.randn(N, D) * (0.5 + rng.rand(D)) + 0.3 * rng.randn(D),) + draw_mixture(rng, G, M, D) + (G,)


def accum_case(i):
    """-> (post (N, M) with exact zeros and one row of zeros, x (N, D))"""
    N, D, M = ACCUM_SHAPES[i]
    rng = np.random.RandomState(2000 + i)
    post = rng.rand(N, M) * (rng.rand(N, M) < 0.7)
    if N > 2:
        post[N // 2] = 0.0
    return post, rng.randn(N, D) * (0.5 + rng.rand(D)) + 0.3 * rng.randn(D)


def measure_rho():
    rho_lse = rho_post = 0.0
    for i, (N, D, M, G) in enumerate(LOGLIK_SHAPES):
        if N == 0:
            continue
        x, a, b, c, _ = loglik_case(i)
        for g in range(G):
            sl = slice(g * M, (g + 1) * M)
            L = R.comp_scores(x, a[sl], b[sl], c[sl], np.longdouble)
            l_ld = R.lse(L, np.longdouble)
            L64 = np.asarray(L, np.float64)
            l64 = R.lse(L64)
            _, T = R.lse_bounds(x, a[sl], b[sl], c[sl])
            rho_lse = max(rho_lse, float((np.abs(l64 - l_ld) / T).max()))
            _, Tp = R.post_bounds(x, a[sl], b[sl], c[sl])
            rho_post = max(rho_post, float((np.abs(R.posteriors(L64, l64) - R.posteriors(L, l_ld, np.longdouble)) / Tp).max()))
    return rho_lse, rho_post


# ------------------------------------------------------------------------------------------------ the oracle pipeline
def corpus_features(utts, dtype=np.float64):
    """[(kept normalised frames (n, D))] of the corpus utterances, through the DCT rows 0 .. N_CEP and spk_ref.features"""
    table = R.dct_rows(SC.N_MEL, SC.N_CEP)
    floor = R.default_energy_floor(SC.N_MEL)
    return [R.features(u["mel"].T.astype(np.float64) @ table.T, floor, dtype)["x"] for u in utts]


def pool(feats, utts):
    return [np.concatenate([f for f, u in zip(feats, utts) if u["speaker"] == s]) for s in range(SC.N_SPEAKERS)]


def pack(feats):
    n = [len(f) for f in feats]
    return np.concatenate(feats), [int(v) for v in np.cumsum([0] + n[:-1])], n


def pipeline(seed, epsilon=None, relevance=16.0, perturb=0.0):
    train, held = SC.corpus(seed, epsilon)
    ft, fh = corpus_features(train), corpus_features(held)
    pools = pool(ft, train)
    if perturb:
        rng = np.random.RandomState(5)
        pools = [p * (1 + perturb * rng.randn(*p.shape)) for p in pools]
    ubm = R.fit_ubm(np.concatenate(pools), SC.M, SC.ITERS)
    means = [R.enrol(p, ubm, relevance) for p in pools]
    X, offs, n = pack(fh)
    llr, _ = R.llr_matrix(X, offs, n, ubm, means)
    return {"train": train, "held": held, "ubm": ubm, "means": means, "llr": llr, "claimed": [u["speaker"] for u in held],
            "report": R.report(llr, [u["speaker"] for u in held])}


def blend_llr(run, a, b, alphas=(0.0, 0.5, 1.0)):
    """The first held-out utterance of speaker a pushed through (1 - alpha) M_a + alpha M_b -> the llr rows, one per alpha"""
    Dm = SC.distortions()
    utt = next(u for u in run["held"] if u["speaker"] == a)
    rows = []
    for al in alphas:
        f = corpus_features([{"mel": SC.distort(utt["base"], (1 - al) * Dm[a] + al * Dm[b])}])
        X, offs, n = pack(f)
        rows.append(R.llr_matrix(X, offs, n, run["ubm"], run["means"])[0][0])
    return np.stack(rows)


def nearest(mu_a, mu_b):
    """the largest distance from a row of mu_a to its nearest row of mu_b"""
    return float(np.sqrt(((mu_a[:, None] - mu_b[None]) ** 2).sum(-1)).min(1).max())


def main():
    rho_lse, rho_post = measure_rho()
    out = {"rho_lse": rho_lse, "rho_post": rho_post, "candidates": {}, "seeds": {}}
    for eps in (0.5, 1.0, 2.0, 3.0):
        out["candidates"][str(eps)] = [pipeline(seed, eps)["report"]["accuracy"] for seed in SC.SEEDS]
    ll_tol = mean_tol = 1e-9
    for seed in SC.SEEDS:
        run, moved = pipeline(seed), pipeline(seed, perturb=1e-9)
        rep = dict(run["report"], loglik=run["ubm"]["history"][-1][-1])
        b = blend_llr(run, 0, 1)
        rep["blend_target_llr"] = [float(v) for v in b[:, 0]]
        rep["blend_rank_b_at_1"] = R.rank_of(b[2], 1)
        rep["llr_at_r_1e12"] = float(np.abs(pipeline(seed, relevance=1e12)["llr"]).max())
        out["seeds"][str(seed)] = rep
        ll_tol = max(ll_tol, abs(moved["ubm"]["history"][-1][-1] - rep["loglik"]))
        mean_tol = max(mean_tol, nearest(run["ubm"]["mu"], moved["ubm"]["mu"]))
    n_held = SC.N_HELD * SC.N_SPEAKERS
    out["accuracy_bar"] = min(r["accuracy"] for r in out["seeds"].values()) - 1.0 / n_held
    out["eer_bar"] = max(r["eer"] for r in out["seeds"].values()) + 0.02
    out["ll_tol"], out["mean_tol"] = ll_tol, mean_tol
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
