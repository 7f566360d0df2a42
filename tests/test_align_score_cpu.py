"""CPU: the confidence oracle (tests/align_score_ref.py), the host reductions of fastspeech2_amd.align against it, and the seeded
inputs of tests/align_score_cases.py that the GPU tests rely on: the substituted-transcript property and the near-tie census."""
import json

import numpy as np

from fastspeech2_amd import align as A
from tests import align_ref as R
from tests import align_score_cases as K
from tests import align_score_ref as SR


def _scored(graph_index):
    mu, var, n_classes, cases = K.substitution()
    phone = SR.class_phone_mono(n_classes, 2)
    return [(c, SR.score(c[0], c[graph_index], *SR.as_mixture(mu, var), phone, SR.plain_decode)) for c in cases], mu, var, phone


def test_gop_is_never_positive_and_zero_where_the_aligned_class_wins():
    scored, mu, var, phone = _scored(1)
    exact = 0
    for (x, g, _, _, _), (frames, red, (state, own, best, arg, _)) in scored:
        assert np.array_equal(frames, R.align(x, g, mu, var)) and np.array_equal(SR.run_lengths(g, state), frames)
        assert (own <= best).all() and red["gop"] <= 0.0 and red["frames"] == len(x)
        cls, blk = g["sid"][state], g["block"][state]
        for k, n in enumerate(frames):
            if n == 0:
                assert np.isnan(red["blocks"][k]).all()
                continue
            assert red["blocks"][k, 1] <= 0.0 and 0.0 <= red["blocks"][k, 2] <= 1.0
            if (arg[blk == k] == cls[blk == k]).all():
                assert red["blocks"][k, 1] == 0.0 and red["blocks"][k, 2] == 1.0
                exact += 1
        # the product's host reductions are the oracle's
        got = A.utterance_scores(g, state, cls, own, best, arg, phone, red["viterbi"] * len(x))
        for key in ("frames", "viterbi", "loglik", "gop", "match"):
            assert np.isclose(got[key], red[key], rtol=1e-12, atol=0), key
        assert np.allclose(got["blocks"], red["blocks"], rtol=1e-12, atol=0, equal_nan=True)
        assert got["scored_frames"] == sum(n for n, b in zip(frames, g["blocks"]) if not b[2])
    assert exact >= 20                                                     # most blocks of a right transcript win every frame


def test_a_substituted_word_scores_below_the_untouched_words():
    """K = 8 utterances, one inner word replaced by a word that shares no phone with it, the table of the true transcripts: in every
    utterance the frame-weighted mean gop of the wrong word's blocks is below that of the other words (fixed seeds; the GPU test
    asserts the same on the same cases)."""
    scored, _, _, _ = _scored(2)
    right, _, _, _ = _scored(1)
    assert len(scored) == K.K == 8
    for ((_, _, gs, sub, rest), (frames, red, _)), (_, (_, red0, _)) in zip(scored, right):
        assert sub and rest and not set(sub) & set(rest)
        wrong, others = SR.block_mean(red, frames, sub), SR.block_mean(red, frames, rest)
        print("gop of the substituted word", wrong, "of the others", others, "utterance", red["gop"], "true transcript", red0["gop"])
        assert wrong < others
        assert red["gop"] < red0["gop"]


def test_near_tie_census_of_the_gpu_comparison():
    """The GPU test compares arg where the oracle's margin exceeds MARGIN |best|; on these very inputs that leaves out at most 1 %."""
    total = out = 0
    for i in range(len(K.SHAPES)):
        fs, cs, w, mu, var, want = K.frame_case(i)
        assert [len(f) for f in fs] == list(K.LENS)
        assert (w.sum(axis=1) > 0).all() and ((w == 0) == (var == 1).all(axis=2)).all()
        for own, best, arg, margin in want:
            assert (own <= best).all() and np.isfinite(best).all()
            total += len(best)
            out += int(np.sum(~(margin > K.MARGIN * np.abs(best))))
    print("frames", total, "left out of the arg comparison", out)
    assert out <= 0.01 * total
    assert {s[0] for s in K.SHAPES} >= {1, 33, 67, K.CLASS_TILE - 1, K.CLASS_TILE, K.CLASS_TILE + 1}
    assert {s[1] for s in K.SHAPES} >= {1, 33, 40, 160} and {s[2] for s in K.SHAPES} >= {1, 3, 8}
    assert set(K.LENS) >= {1, 31, 32, 33, 70, K.FRAME_TILE - 1, K.FRAME_TILE, K.FRAME_TILE + 1}


def test_oracle_scores_are_the_emission_oracles():
    """F restricted to a graph's classes is align_ref's (single Gaussian) and align_gmm_ref's (mixture) emission matrix."""
    from tests import align_gmm_ref as GR
    fs, cs, w, mu, var, _ = K.frame_case(1)
    sid = np.arange(mu.shape[0])
    F = SR.class_scores(fs[4], w, mu, var)
    assert np.allclose(F, GR.emissions(fs[4], sid, w, mu, var)[0], rtol=1e-12, atol=0)
    F1 = SR.class_scores(fs[4], *SR.as_mixture(mu[:, 0], var[:, 0]))
    assert np.allclose(F1, R.emissions(fs[4], sid, mu[:, 0], var[:, 0]), rtol=1e-12, atol=0)
    dup = SR.class_scores(fs[4], w[[0, 1, 0]], mu[[0, 1, 0]], var[[0, 1, 0]])
    own, best, arg, margin = SR.frame_scores(dup, np.array([2, 5, -1] + [0] * (len(fs[4]) - 3)))
    assert (arg != 2).all() and (margin[arg == 0] == 0).all()              # equal rows tie, the lower index wins
    assert own[0] == dup[0, 2] and np.isnan(own[1]) and np.isnan(own[2])


def test_path_states_of_a_broken_chain():
    lex = {"a": ["X"], "bc": ["Y", "Z"]}
    g = A.utterance_graph(["a", "bc"], lex, A.phone_table(lex), 1)
    E = np.random.RandomState(0).randn(9, len(g["sid"]))
    bp, end, frames = R.viterbi(E, g)
    state = SR.path_states(bp, end, g)
    assert np.array_equal(SR.run_lengths(g, state), frames) and (np.diff(state) >= 0).all()
    bad = bp.copy()
    bad[5, state[5]] = 2 if g["skip"][state[5]] < 0 else 7                 # a skip where there is none / no code at all
    broken = SR.path_states(bad, end, g)
    assert np.array_equal(broken[5:], state[5:]) and (broken[:5] == -1).all()
    assert (SR.path_states(bp, len(g["sid"]), g) == -1).all()


def test_class_phone():
    al = A.Aligner.__new__(A.Aligner)
    al.triphones, al.n_classes, al.n_mono, al.states, al.tree = 0, 6, 6, 2, None
    assert al.class_phone().tolist() == [0, 0, 1, 1, 2, 2] == SR.class_phone_mono(6, 2).tolist()
    # two phones of two states: root 0 splits into nodes 4 (split again into 6, 7) and 5; leaves in ascending node order
    question = np.array([0, -1, -1, -1, 1, -1, -1, -1])
    yes, no = np.array([4, -1, -1, -1, 6, -1, -1, -1]), np.array([5, -1, -1, -1, 7, -1, -1, -1])
    leaf = np.array([-1, 0, 1, 2, -1, 3, 4, 5])
    al.triphones, al.n_classes, al.n_mono = 6, 6, 4
    al.tree = {"question": question, "yes": yes, "no": no, "leaf": leaf, "n_leaves": 6}
    assert al.class_phone().tolist() == [0, 1, 1, 0, 0, 0] == SR.class_phone_tree(question, yes, no, leaf, 4, 2).tolist()


def test_scores_summary(tmp_path):
    rows = [{"speaker": "s", "basename": f"u{i}", "frames": 10, "scored_frames": 5 + i, "viterbi": -1.0, "loglik": -2.0, "gop": -0.1 * i,
             "match": 1.0, "phones": []} for i in range(12)]
    path = tmp_path / "scores.jsonl"
    path.write_text("".join(json.dumps(r) + "\n" for r in rows))
    text = A.scores_summary(str(path))
    assert text.startswith("scores: 12 utterances, mean gop ") and text.count("s/u") == 10 and "s/u11 -1.1000, s/u10" in text
    assert f"{sum(-0.1 * i * (5 + i) for i in range(12)) / sum(5 + i for i in range(12)):.4f}" in text
