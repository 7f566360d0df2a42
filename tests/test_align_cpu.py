"""CPU: the host side of the forced aligner (fastspeech2_amd/align.py: lexicon, text, graphs, TextGrid writer) and its numpy oracle
(tests/align_ref.py) against brute-force path enumeration and on a synthetic corpus whose boundaries are known."""
import itertools

import numpy as np
import pytest

from fastspeech2_amd import align as A
from fastspeech2_amd import preprocess as P
from tests import align_corpus as C
from tests import align_ref as R

SEED, N_UTT, ITERS = 1234, 60, 12


def config(root, lexicon_path=None):
    return {"dataset": "Synth", "path": {"raw_path": f"{root}/raw", "preprocessed_path": f"{root}/pre", "lexicon_path": lexicon_path},
            "preprocessing": {"val_size": 2, "text": {"text_cleaners": ["english_cleaners"], "language": "en"},
                              "audio": {"sampling_rate": 22050, "max_wav_value": 32768.0},
                              "stft": {"filter_length": 1024, "hop_length": 256, "win_length": 1024},
                              "mel": {"n_mel_channels": 80, "mel_fmin": 0, "mel_fmax": 8000},
                              "pitch": {"feature": "phoneme_level", "normalization": True},
                              "energy": {"feature": "phoneme_level", "normalization": True}}}


def test_lexicon_and_words(tmp_path):
    path = tmp_path / "lex.txt"
    path.write_text("HELLO  HH AH0 L OW1\nhello HH EH0 L OW1\nWorld\tW ER1 L D\n\ndon't D OW1 N T\n")
    lex = A.read_lexicon(str(path))
    assert lex == {"hello": ["HH", "AH0", "L", "OW1"], "world": ["W", "ER1", "L", "D"], "don't": ["D", "OW1", "N", "T"]}
    assert A.words_of("Hello, world -- don't  stop!?\n") == ["Hello", "world", "don't", "stop"]
    assert A.words_of(' "quoted" (word). ') == ["quoted", "word"]
    ids = A.phone_table(lex)
    assert sorted(ids.values()) == list(range(len(ids))) and {"sil", "sp", "spn"} <= set(ids)
    g = A.utterance_graph(["HELLO", "zzz"], lex, ids, 1)
    assert [b[0] for b in g["blocks"]] == ["sil", "HH", "AH0", "L", "OW1", "sp", "spn", "sil"]       # case-folded; OOV -> spn
    with pytest.raises(ValueError):
        A.utterance_graph([], lex, ids, 2)
    with pytest.raises(ValueError):
        A.utterance_graph(["hello"], lex, ids, 4)


def test_graph_arrays():
    lex = {"a": ["X"], "bc": ["Y", "Z"]}
    ids = A.phone_table(lex)                                               # X 0, Y 1, Z 2, sil 3, sp 4, spn 5
    assert ids == {"X": 0, "Y": 1, "Z": 2, "sil": 3, "sp": 4, "spn": 5}
    g = A.utterance_graph(["a"], lex, ids, 1)                              # sil X sil
    assert g["sid"].tolist() == [3, 0, 3] and g["skip"].tolist() == [-1, -1, -1] and g["block"].tolist() == [0, 1, 2]
    assert g["alt"] == (1, 1) and g["mandatory"] == 1
    g = A.utterance_graph(["a", "bc"], lex, ids, 2)                        # sil X sp Y Z sil, two states each
    assert g["sid"].tolist() == [6, 7, 0, 1, 8, 9, 2, 3, 4, 5, 6, 7]
    assert g["block"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert g["skip"].tolist() == [-1, -1, -1, -1, -1, -1, 3, -1, -1, -1, -1, -1]     # first state of Y skips sp from X's last state
    assert g["alt"] == (2, 9) and g["mandatory"] == 6
    assert [b[1] for b in g["blocks"]] == [-1, 0, -1, 1, 1, -1] and [b[2] for b in g["blocks"]] == [True, False, True, False, False, True]
    g = A.utterance_graph(["a", "a", "a"], lex, ids, 1)                    # sil X sp X sp X sil
    assert g["skip"].tolist() == [-1, -1, -1, 1, -1, 3, -1] and g["alt"] == (1, 5)
    assert A.flat_assignment(g, 7).tolist() == [1, 1, 1, 3, 3, 5, 5] and A.flat_assignment(g, 3).tolist() == [1, 3, 5]


def _paths(graph, T):
    """every admissible state sequence of length T"""
    J, skip = len(graph["sid"]), graph["skip"]
    ok = lambda a, b: b == a or b == a + 1 or skip[b] == a                # noqa: E731
    for p in itertools.product(range(J), repeat=T):
        if p[0] in R.starts(graph) and p[-1] in R.ends(graph) and all(ok(a, b) for a, b in zip(p, p[1:])):
            yield p


def _tie_rule_best(paths, scores):
    """the path Viterbi's tie rule picks among the best: the lowest end state, then, walking back, the lowest backpointer code, which
    is the highest predecessor state"""
    best = [p for p, s in zip(paths, scores) if s == max(scores)]
    for t in range(len(best[0]) - 1, -1, -1):
        pick = min(p[t] for p in best) if t == len(best[0]) - 1 else max(p[t] for p in best)
        best = [p for p in best if p[t] == pick]
    assert len(best) == 1
    return best[0]


@pytest.mark.parametrize("words,S,T,integer", [(["a"], 1, 5, False), (["a"], 1, 1, False), (["a", "a"], 1, 7, False),
                                               (["a", "a"], 1, 6, True), (["bc"], 1, 7, True), (["a"], 2, 2, False),
                                               (["a", "a"], 1, 2, False), (["bc"], 1, 6, False), (["a", "a"], 1, 7, True)])
def test_oracle_against_path_enumeration(words, S, T, integer):
    lex = {"a": ["X"], "bc": ["Y", "Z"]}
    g = A.utterance_graph(words, lex, A.phone_table(lex), S)
    J = len(g["sid"])
    assert J <= 6 and T <= 7
    rng = np.random.RandomState(T * 10 + J)
    E = rng.randint(-2, 1, (T, J)).astype(np.float64) if integer else 3.0 * rng.randn(T, J)   # small integers: exact ties
    paths = list(_paths(g, T))
    assert paths
    scores = [sum(E[t, j] for t, j in enumerate(p)) for p in paths]
    m = max(scores)
    total = m + np.log(sum(np.exp(s - m) for s in scores))
    gamma, alpha, ll = R.posteriors(E, g)
    assert abs(ll - total) <= 1e-12 * max(1.0, abs(total))
    want = np.zeros((T, J))
    for p, s in zip(paths, scores):
        for t, j in enumerate(p):
            want[t, j] += np.exp(s - total)
    assert np.abs(gamma - want).max() <= 1e-12
    assert np.abs(gamma.sum(axis=1) - 1).max() <= 1e-12
    bp, end, frames = R.viterbi(E, g)
    best = _tie_rule_best(paths, scores)
    assert end == best[-1]
    assert frames.tolist() == [sum(1 for j in best if g["block"][j] == k) for k in range(len(g["blocks"]))]
    j = end
    for t in range(T - 1, 0, -1):                                          # the backpointers along the path are that path
        j = (j, j - 1, g["skip"][j])[bp[t, j]]
        assert j == best[t - 1]


def test_textgrid_round_trip(tmp_path):
    lex = {"a": ["X"], "bc": ["Y", "Z"]}
    g = A.utterance_graph(["bc", "a", "zz"], lex, A.phone_table(lex), 2)   # sil Y Z sp X sp spn sil
    frames = [3, 4, 2, 0, 7, 5, 2, 6]
    words, phones, xmax = A.intervals(g, ["bc", "a", "zz"], frames, 256, 22050)
    f = lambda n: n * 256 / 22050                                         # noqa: E731
    assert [p[2] for p in phones] == ["sil", "Y", "Z", "X", "sp", "spn", "sil"] and xmax == f(29)
    assert [w[2] for w in words] == ["", "bc", "a", "", "zz", ""]
    assert words[1][:2] == (f(3), f(9)) and phones[0][0] == 0.0
    path = tmp_path / "u.TextGrid"
    A.write_textgrid(str(path), words, phones, xmax)
    tiers = P.read_textgrid(str(path))
    assert tiers["phones"] == phones                                       # times come back bit for bit
    assert tiers["words"] == [w for w in words if w[2]]
    assert P.read_textgrid(str(path), include_empty_intervals=True)["words"] == words
    pp = P.Preprocessor(config(str(tmp_path)), device="cpu", pitch_fn=lambda *a: None)
    ph, dur, start, end = pp.get_alignment(tiers["phones"])
    assert ph == ["Y", "Z", "X"] and dur == [4, 2, 7]                      # leading sil and the trailing sp / spn / sil trimmed
    assert (start, end) == (f(3), f(16))
    ph, dur, _, _ = pp.get_alignment([(s, e, "Q") for s, e, _ in phones])  # nothing is silence: the durations telescope
    assert dur == [n for n in frames if n] and sum(dur) == 29


@pytest.fixture(scope="module")
def oracle_run():
    lex, utts = C.corpus(SEED, N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    mu, var, history = R.fit(xs, graphs, len(ids) * C.STATES, ITERS)
    return utts, graphs, xs, mu, var, history


def test_oracle_em_on_synthetic_corpus(oracle_run):
    """Seed 1234, 60 utterances, 12 passes, mean separation 0.5 sigma per dimension over 80 dimensions: the log-likelihood per frame
    never falls and A_ref, the share of true phone boundaries found within +-1 frame, measured 0.9947 (the bar is 0.95)."""
    utts, graphs, xs, mu, var, history = oracle_run
    assert len(history) == ITERS and np.all(np.diff(history) >= -1e-9), history
    got = [R.align(x, g, mu, var) for x, g in zip(xs, graphs)]
    for u, fr in zip(utts, got):
        assert fr.sum() == u["mel"].shape[1]
    a_ref = C.accuracy([[d for _, d in u["segments"]] for u in utts], got, 1)
    print("A_ref", a_ref)
    assert a_ref >= 0.95, a_ref


def test_oracle_is_stable_under_one_ulp(oracle_run):
    """The GPU test allows the durations of 2 % of the utterances to differ from the oracle's (a boundary may flip where two paths tie
    to rounding).  That cap must hold for the oracle against itself when every emission moves by one ulp in a random direction, in
    training and in decoding: on this seed no utterance of the 60 changes."""
    utts, graphs, xs, mu, var, history = oracle_run
    rng = np.random.RandomState(SEED + 1)
    ulp = lambda E: np.nextafter(E, np.where(rng.rand(*E.shape) < 0.5, -np.inf, np.inf))     # noqa: E731
    mu2, var2, history2 = R.fit(xs, graphs, len(mu), ITERS, perturb=ulp)
    assert np.abs(np.array(history2) / np.array(history) - 1).max() <= 1e-6
    differ = sum(1 for x, g in zip(xs, graphs) if not np.array_equal(R.align(x, g, mu, var), R.align(x, g, mu2, var2, perturb=ulp)))
    print("utterances that differ under 1 ulp", differ)
    assert differ <= 0.02 * len(utts), differ


def test_host_update_equals_oracle_update():
    rng = np.random.RandomState(3)
    C_, D = 7, 5
    sums = np.abs(rng.randn(C_, 1 + 2 * D)) + 0.5
    sums[:, 0] = [5.0, 0.2, 1.0, 0.999, 3.0, 0.0, 8.0]
    sums[:, 1 + D:] += 4.0
    sums[4, 1 + D:] = (sums[4, 1:1 + D] / 3.0) ** 2 * 3.0                  # zero variance: the floor holds
    mu, var, floor = rng.randn(C_, D), np.abs(rng.randn(C_, D)) + 1, np.full(D, 0.01)
    m1, v1 = A.m_step(sums, mu, var, floor)
    m2, v2 = R.update(sums, mu, var, floor)
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    assert np.array_equal(m1[[1, 3, 5]], mu[[1, 3, 5]]) and np.allclose(v1[4], 0.01)


def test_batches_by_bytes():
    frames, states = [900, 100, 500, 500, 40], [300, 40, 200, 180, 20]
    batches = list(A.batches_by_bytes(frames, states, 160, 2 * 900 * 300 * 17 + 2 * 900 * 160 * 8 + 2 * 300 * 321 * 8))
    assert batches[0] == [0, 2] and sorted(i for b in batches for i in b) == [0, 1, 2, 3, 4]
    assert list(A.batches_by_bytes(frames, states, 160, 1)) == [[0], [2], [3], [1], [4]]      # a batch always takes one utterance


def test_cpu_device_fails_loudly(tmp_path):
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.Aligner(6, 4, 2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.features(torch.zeros(1, 4, 9), [9])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.build(config(str(tmp_path), str(tmp_path / "lex.txt")), device="cpu")
