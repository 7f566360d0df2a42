"""CPU: the forced aligner's trained transition and optional-silence probabilities.  The host side (fastspeech2_amd.align `arc_costs`,
`trans_step`) and the numpy oracle tests/align_trans_ref.py: the oracle against brute-force path enumeration, the arc costs as
proper distributions, the harmless start at 0.5, the mass identity of the arc posteriors, the update's keep and clip rules and the
recovery of a known model from sampled state sequences."""
import numpy as np
import pytest

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_ref as R
from tests import align_trans_ref as T
from tests.test_align_cpu import _paths, _tie_rule_best

LEX = {"a": ["X"], "bc": ["Y", "Z"]}
IDS = A.phone_table(LEX)


def tables(rng, n_classes):
    return rng.uniform(0.05, 0.95, n_classes), rng.uniform(0.05, 0.95, 3)


def without_final_sil(g, S):
    """the graph with its last (optional) block cut off: the last block is mandatory"""
    J = len(g["sid"]) - S
    return {"sid": g["sid"][:J], "skip": g["skip"][:J], "block": g["block"][:J], "alt": (g["alt"][0], -1), "blocks": g["blocks"][:-1],
            "mandatory": g["mandatory"]}


def single_block(cls, S):
    return {"sid": np.arange(cls * S, (cls + 1) * S, dtype=np.int32), "skip": np.full(S, -1, np.int32), "block": np.zeros(S, np.int32),
            "alt": (-1, -1), "blocks": [("X", 0, False)], "mandatory": S}


def arc_of(g, a, b):
    return 0 if b == a else (1 if b == a + 1 else 2)


def test_oracle_against_path_enumeration():
    """Two one-phone words, one state per phone, six frames: sil X sp X sil.  Every path is listed with its emissions, its arc costs,
    its start and its end edge; loglik, gamma, xi and the Viterbi path follow from the list."""
    g = A.utterance_graph(["a", "a"], LEX, IDS, 1)
    Tn, J = 6, len(g["sid"])
    rng = np.random.RandomState(11)
    loop, opt = tables(rng, len(IDS))
    w, edge = T.arc_costs(g, loop, opt)
    E = 3.0 * rng.randn(Tn, J)
    paths = list(_paths(g, Tn))
    assert len(paths) > 20
    start, end = dict(T.start_edges(g, edge)), dict(T.end_edges(g, edge))
    scores = [start[p[0]] + end[p[-1]] + sum(E[t, j] for t, j in enumerate(p)) + sum(w[arc_of(g, a, b), b] for a, b in zip(p, p[1:]))
              for p in paths]
    m = max(scores)
    total = m + np.log(sum(np.exp(s - m) for s in scores))
    gamma, xi, alpha, ll = T.posteriors(E, g, w, edge)
    assert abs(ll - total) <= 1e-12 * max(1.0, abs(total))
    want_g, want_x = np.zeros((Tn, J)), np.zeros((J, 5))
    for p, s in zip(paths, scores):
        pr = np.exp(s - total)
        for t, j in enumerate(p):
            want_g[t, j] += pr
        for a, b in zip(p, p[1:]):
            want_x[b, arc_of(g, a, b)] += pr
        want_x[p[0], 3] += pr
        want_x[p[-1], 4] += pr
    assert np.abs(gamma - want_g).max() <= 1e-12 and np.abs(xi - want_x).max() <= 1e-12
    assert want_x[:, 2].sum() > 1e-3 and want_x[g["alt"][0], 3] > 1e-6 and want_x[g["alt"][1], 4] > 1e-6      # every kind of arc carries mass
    bp, e, frames, score = T.viterbi(E, g, w, edge)
    best = _tie_rule_best(paths, scores)
    assert e == best[-1] and abs(score - max(scores)) <= 1e-12 * abs(score)
    assert frames.tolist() == [sum(1 for j in best if g["block"][j] == k) for k in range(len(g["blocks"]))]
    j = e
    for t in range(Tn - 1, 0, -1):
        j = (j, j - 1, g["skip"][j])[bp[t, j]]
        assert j == best[t - 1]
    assert T.viterbi(E, g, np.zeros_like(w), np.zeros(4))[2].tolist() == R.viterbi(E, g)[2].tolist()      # zero costs: the default decoder


def graphs_for(S):
    ids = A.phone_table(LEX)
    full = [A.utterance_graph(words, LEX, ids, S) for words in (["a"], ["a", "bc"], ["bc", "a", "zz", "a"])]
    return full + [without_final_sil(full[1], S), without_final_sil(full[2], S), single_block(2, S)], len(ids) * S


@pytest.mark.parametrize("S", [1, 2, 3])
def test_arc_costs_are_a_proper_distribution_at_every_state(S):
    graphs, n_classes = graphs_for(S)
    loop, opt = tables(np.random.RandomState(S), n_classes)
    for g in graphs:
        w, edge = A.arc_costs(g, loop, opt)
        wr, er = T.arc_costs(g, loop, opt)
        assert w.shape == (3, len(g["sid"])) and edge.shape == (4,) and np.isfinite(w).all() and np.isfinite(edge).all()
        assert np.abs(w - wr).max() <= 1e-15 and np.abs(edge - er).max() <= 1e-15                     # the product's and the oracle's
        J, alt = len(g["sid"]), g["alt"]
        for i in range(J):
            out = np.exp(w[0, i])
            if i + 1 < J:
                out += np.exp(w[1, i + 1])
            out += sum(np.exp(w[2, j]) for j in range(J) if g["skip"][j] == i)
            if i == J - 1:
                out += np.exp(edge[2])
            if i == alt[1]:
                out += np.exp(edge[3])
            assert abs(out - 1.0) <= 1e-14, (S, i, out)
        assert abs(np.exp(edge[0]) + (np.exp(edge[1]) if alt[0] >= 0 else 0.0) - 1.0) <= 1e-14
        assert w[1, 0] == 0.0 and (w[2][g["skip"] < 0] == 0.0).all()
    kinds = A.block_kinds(graphs[2])
    assert kinds.tolist() == T.kinds(graphs[2]) and kinds[0] == 0 and kinds[-1] == 2 and sorted(set(kinds.tolist())) == [-1, 0, 1, 2]
    assert A.block_kinds(graphs[4])[-1] == -1 and A.block_kinds(graphs[5]).tolist() == [-1]


@pytest.fixture(scope="module")
def utterances():
    lex, utts = C.corpus(1234, 6)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    n_classes = len(ids) * C.STATES
    rng = np.random.RandomState(8)                                         # emissions of magnitude 3: many paths matter, and |loglik| stays
    return graphs, xs, [3.0 * rng.randn(len(x), len(g["sid"])) for x, g in zip(xs, graphs)], n_classes      # near 1e2 (see below)


def test_at_one_half_the_posteriors_are_the_default_ones(utterances):
    """With every table at 0.5 all paths of an utterance carry (T + optional blocks) log 0.5: the posteriors do not move.  They are
    compared to 1e-12 absolute.  gamma = exp(alpha + beta - loglik) carries the rounding of sums of the size of loglik, a few ulp of
    it, and the two recursions round differently (one adds log 0.5 at every step); 1e-12 is therefore attainable only where
    ulp(loglik) is well below it: on these emissions |loglik| is a few hundred (ulp 5.7e-14), on the corpus's own 160-dimensional
    Gaussians it is 3e4 (ulp 3.6e-12) and no fp64 implementation could be held to 1e-12 there."""
    graphs, _, Es, n_classes = utterances
    for E, g in zip(Es, graphs):
        w, edge = T.arc_costs(g, np.full(n_classes, 0.5), np.full(3, 0.5))
        gamma, xi, _, ll = T.posteriors(E, g, w, edge)
        g0, _, ll0 = R.posteriors(E, g)
        n_opt = sum(1 for b in g["blocks"] if b[2])
        assert np.abs(gamma - g0).max() <= 1e-12
        assert abs(ll - (ll0 + (len(E) + n_opt) * np.log(0.5))) <= 1e-12 * abs(ll)
        assert T.viterbi(E, g, w, edge)[2].tolist() == R.viterbi(E, g)[2].tolist()


def test_arc_posteriors_and_start_mass_add_up_to_the_occupancy(utterances):
    graphs, _, Es, n_classes = utterances
    loop, opt = tables(np.random.RandomState(5), n_classes)
    for E, g in zip(Es, graphs):
        gamma, xi, _, _ = T.posteriors(E, g, *T.arc_costs(g, loop, opt))
        assert np.abs(xi[:, :3].sum(axis=1) + xi[:, 3] - gamma.sum(axis=0)).max() <= 1e-10
        assert abs(xi[:, 3].sum() - 1.0) <= 1e-12 and abs(xi[:, 4].sum() - 1.0) <= 1e-12
        enter, skipped = T.opt_masses(xi, g)
        n_sp = sum(1 for k in T.kinds(g) if k == 1)
        assert np.abs(enter + skipped - [1.0, n_sp, 1.0]).max() <= 1e-10      # every optional block is taken or skipped, once


def test_update_keeps_and_clips():
    n = np.array([5.0, 0.999, 1.0, 0.0, 8.0, 2.0])
    s = np.array([2.5, 0.9, 0.0, 0.0, 7.99, 1.0])
    loop = np.array([0.3, 0.31, 0.32, 0.33, 0.34, 0.35])
    opt = np.array([0.2, 0.3, 0.4])
    enter, skipped = np.array([0.4, 0.001, 30.0]), np.array([0.5, 40.0, 0.0])
    new_loop, new_opt = A.trans_step(n, s, enter, skipped, loop, opt)
    assert np.array_equal(new_loop, [0.5, 0.31, A.TRANS_FLOOR, 0.33, 1.0 - A.TRANS_FLOOR, 0.5])      # n < 1 keeps, the floor clips
    assert np.array_equal(new_opt, [0.2, A.TRANS_FLOOR, 1.0 - A.TRANS_FLOOR])                        # enter + skipped < 1 keeps
    ref_loop, ref_opt = T.update(n, s, enter, skipped, loop, opt)
    assert np.array_equal(new_loop, ref_loop) and np.array_equal(new_opt, ref_opt)
    assert A.TRANS_FLOOR == T.FLOOR == 0.01
    assert np.array_equal(loop, [0.3, 0.31, 0.32, 0.33, 0.34, 0.35]) and np.array_equal(opt, [0.2, 0.3, 0.4])    # the inputs are not written


def sample(rng, g, loop, opt):
    """one state sequence of the HMM that `arc_costs` describes"""
    kind, J = T.kinds(g), len(g["sid"])
    to = {int(s): j for j, s in enumerate(g["skip"]) if s >= 0}
    j = 0 if (g["alt"][0] < 0 or rng.rand() < opt[0]) else g["alt"][0]
    path = [j]
    while True:
        if rng.rand() < loop[g["sid"][j]]:
            path.append(j)
            continue
        if j == J - 1:
            return path
        if j == g["alt"][1] and rng.rand() >= opt[2]:
            return path
        if j in to and rng.rand() >= opt[kind[g["block"][j + 1]]]:
            j = to[j]
        else:
            j += 1
        path.append(j)


def test_a_known_model_is_recovered():
    """120 utterances of 2 to 5 words sampled from loop in [0.3, 0.8] and opt = (0.7, 0.1, 0.6): a corpus with almost no inter-word
    pauses.  Class means 2.5 N(0, 1) in 6 dimensions, unit noise: posteriors nearly hard.  Three passes from 0.5 with the Gaussians at
    their true values.  The largest distance between an estimate and the empirical fraction of the sampled sequences (classes with at
    least 30 frames; the three kinds) measured 1.453e-2; the test allows twice that."""
    rng = np.random.RandomState(2024)
    lex = {f"w{i}": [["X", "Y", "Z", "V"][k] for k in rng.randint(0, 4, rng.randint(1, 4))] for i in range(8)}
    ids = A.phone_table(lex)
    S, D = 2, 6
    n_classes = len(ids) * S
    true_loop, true_opt = rng.uniform(0.3, 0.8, n_classes), np.array([0.7, 0.1, 0.6])
    means = 2.5 * rng.randn(n_classes, D)
    graphs, xs, stay, frames, enter, skipped = [], [], np.zeros(n_classes), np.zeros(n_classes), np.zeros(3), np.zeros(3)
    for _ in range(120):
        g = A.utterance_graph([sorted(lex)[k] for k in rng.randint(0, len(lex), rng.randint(2, 6))], lex, ids, S)
        path = sample(rng, g, true_loop, true_opt)
        graphs.append(g)
        xs.append(means[g["sid"][path]] + rng.randn(len(path), D))
        np.add.at(frames, g["sid"][path], 1.0)
        np.add.at(stay, g["sid"][[b for a, b in zip(path, path[1:]) if a == b]], 1.0)
        visited = set(g["block"][path].tolist())
        for k, kind in enumerate(T.kinds(g)):
            if kind >= 0:
                enter[kind] += k in visited
                skipped[kind] += k not in visited
    mu, var = means.copy(), np.ones((n_classes, D))
    loop, opt = np.full(n_classes, 0.5), np.full(3, 0.5)
    for _ in range(3):
        parts, s, e, k, _ = T._pass(xs, graphs, n_classes, loop, opt, lambda f, sid: (R.emissions(f, sid, mu, var), None),
                                    lambda gamma, _, f: R.partials(gamma, f))
        loop, opt = T.update(R.class_sums(parts, graphs, n_classes)[:, 0], s, e, k, loop, opt)
    seen = frames >= 30
    assert seen.sum() >= n_classes - 4 and (enter + skipped >= 100).all()
    dist = max(np.abs(loop[seen] - np.clip(stay[seen] / frames[seen], T.FLOOR, 1 - T.FLOOR)).max(),
               np.abs(opt - np.clip(enter / (enter + skipped), T.FLOOR, 1 - T.FLOOR)).max())
    print("distance to the empirical fractions", dist, "opt", opt, "empirical", enter / (enter + skipped))
    assert dist <= 2 * 1.453e-2
    assert opt[1] < 0.5 and abs(opt[1] - true_opt[1]) < 0.05              # the direction: pauses are rare and the model says so
