"""CPU: the numpy oracle of the phone-loop recogniser (tests/align_loop_ref.py) against brute-force enumeration of all paths, and
the host side of fastspeech2_amd/recognize.py (`phone_bigram`, `edit_counts`) against the oracle's restatement, brute force and
hand-made cases."""
import itertools

import numpy as np
import pytest

from fastspeech2_amd import recognize as RC
from tests import align_loop_ref as LR

NINF = -np.inf


def _paths(P, S, T):
    """every path of the loop as [(state, code that entered it)], the code of frame 0 being 0"""
    def grow(path):
        if len(path) == T:
            if path[-1][0] % S == S - 1:
                yield path
            return
        j = path[-1][0]
        p, s = divmod(j, S)
        yield from grow(path + [(j, 0)])
        if s < S - 1:
            yield from grow(path + [(j + 1, 1)])
        else:
            for q in range(P):
                yield from grow(path + [(q * S, 2 + p)])
    for q in range(P):
        yield from grow([(q * S, 0)])


def _score(path, E, self_, next_, link, init, final_, S):
    j0 = path[0][0]
    total = init[j0 // S] + E[0, j0]
    for t in range(1, len(path)):
        j, code = path[t]
        total += (self_[j] if code == 0 else next_[j] if code == 1 else link[code - 2][j // S]) + E[t, j]
    return total + final_[path[-1][0] // S]


def _tie_rule_best(paths, scores):
    """the path the tie rules pick among the best: the lowest end state, then, walking back, the lowest backpointer code"""
    best = [p for p, s in zip(paths, scores) if s == max(scores)]
    pick = min(p[-1][0] for p in best)
    best = [p for p in best if p[-1][0] == pick]
    for t in range(len(best[0]) - 1, 0, -1):
        pick = min(p[t][1] for p in best)
        best = [p for p in best if p[t][1] == pick]
    assert len(best) == 1
    return best[0]


def _costs(rng, P, S, kind):
    C = P * S
    if kind == "zero":
        return np.zeros(C), np.zeros(C), np.zeros((P, P)), np.zeros(P), np.zeros(P)
    if kind == "integer":                                                  # small integers: exact sums, ties everywhere
        draw = lambda *n: rng.randint(-2, 1, n).astype(np.float64)        # noqa: E731
    else:
        draw = lambda *n: 2.0 * rng.randn(*n)                             # noqa: E731
    return draw(C), draw(C), draw(P, P), draw(P), draw(P)


@pytest.mark.parametrize("kind", ["random", "integer", "zero"])
@pytest.mark.parametrize("P,S,T", [(2, 1, 4), (2, 2, 5), (3, 2, 6), (3, 3, 6)])
def test_oracle_against_path_enumeration(P, S, T, kind):
    rng = np.random.RandomState(100 * P + 10 * S + T)
    costs = _costs(rng, P, S, kind)
    E = np.zeros((T, P * S)) if kind == "zero" else (rng.randint(-2, 1, (T, P * S)).astype(np.float64) if kind == "integer"
                                                    else 3.0 * rng.randn(T, P * S))
    paths = list(_paths(P, S, T))
    assert paths
    scores = [_score(p, E, *costs, S) for p in paths]
    bp, end, score = LR.loop_viterbi(E, *costs, P, S)
    segs = LR.loop_backtrack(bp, end, P, S)
    assert abs(score - max(scores)) <= 1e-12 * max(1.0, abs(score))
    if kind == "random":                                                   # the sums associate differently: the oracle's path is a best one
        best = [p for p, s in zip(paths, scores) if abs(s - max(scores)) <= 1e-12 * max(1.0, abs(score))]
        assert len(best) == 1
        best = best[0]
    else:
        assert score == max(scores)
        best = _tie_rule_best(paths, scores)
    assert end == best[-1][0]
    j = end
    for t in range(T - 1, 0, -1):                                          # the backpointers along the path are that path
        assert bp[t, j] == best[t][1]
        j = best[t - 1][0]
    want = [(best[0][0] // S, 0)] + [(j // S, t) for t, (j, code) in enumerate(best) if code >= 2]
    assert segs == want
    got, _ = LR.decode(E, *costs, P, S)
    assert [(p, a) for p, a, _ in got] == want and sum(n for _, _, n in got) == T and all(n >= S for _, _, n in got)


def test_forbidden_arcs_are_never_taken():
    P, S, T = 3, 2, 9
    rng = np.random.RandomState(4)
    self_, next_, link, init, final_ = _costs(rng, P, S, "random")
    init[0] = NINF                                                         # phone 0 may not start
    link[1, 2] = NINF                                                      # 2 may not follow 1
    final_[2] = NINF
    E = 3.0 * rng.randn(T, P * S)
    E[:, 0:2] += 50.0                                                      # phone 0 is by far the best everywhere
    segs, score = LR.decode(E, self_, next_, link, init, final_, P, S)
    phones = [p for p, _, _ in segs]
    assert np.isfinite(score) and phones[0] != 0 and phones[-1] != 2 and (1, 2) not in zip(phones, phones[1:]) and 0 in phones
    paths = list(_paths(P, S, T))
    scores = [_score(p, E, self_, next_, link, init, final_, S) for p in paths]
    assert abs(score - max(scores)) <= 1e-12 * abs(score)


@pytest.mark.parametrize("P,S,T", [(2, 2, 1), (3, 3, 2), (1, 3, 0), (2, 1, 0)])
def test_too_few_frames_have_no_path(P, S, T):
    E = np.zeros((T, P * S))
    bp, end, score = LR.loop_viterbi(E, np.zeros(P * S), np.zeros(P * S), np.zeros((P, P)), np.zeros(P), np.zeros(P), P, S)
    assert T < S and end == -1 and score == NINF and LR.loop_backtrack(bp, end, P, S) == []
    assert LR.decode(E, np.zeros(P * S), np.zeros(P * S), np.zeros((P, P)), np.zeros(P), np.zeros(P), P, S) == ([], NINF)


def test_backtrack_refuses_a_chain_that_leaves_the_table():
    P, S = 2, 2
    bp = np.zeros((4, 4), np.uint8)
    assert LR.loop_backtrack(bp, 3, P, S) == [(1, 0)]
    assert LR.loop_backtrack(bp, 4, P, S) is None                          # an end outside the table
    bad = bp.copy()
    bad[3, 3], bad[2, 2] = 1, 1                                            # code 1 at a first state
    assert LR.loop_backtrack(bad, 3, P, S) is None
    bad = bp.copy()
    bad[3, 3] = 2                                                          # an entry code at a last state
    assert LR.loop_backtrack(bad, 3, P, S) is None
    bad = bp.copy()
    bad[3, 3], bad[2, 2] = 1, 2 + P                                        # an entry from a phone outside the table
    assert LR.loop_backtrack(bad, 3, P, S) is None


# ------------------------------------------------------------------------------------------------ edit distance
def _brute_distance(ref, hyp):
    if not ref or not hyp:
        return len(ref) + len(hyp)
    return min(_brute_distance(ref[1:], hyp[1:]) + (ref[0] != hyp[0]), _brute_distance(ref[1:], hyp) + 1, _brute_distance(ref, hyp[1:]) + 1)


def _check_ops(ref, hyp, counts, ops):
    hits, sub, dele, ins = counts
    assert hits + sub + dele == len(ref) and hits + sub + ins == len(hyp)
    assert [o[1] for o in ops if o[1] is not None] == list(range(len(ref)))
    assert [o[2] for o in ops if o[2] is not None] == list(range(len(hyp)))
    for kind, a, b in ops:
        assert {"hit": ref[a] == hyp[b] if kind == "hit" else None, "sub": ref[a] != hyp[b] if kind == "sub" else None,
                "del": b is None, "ins": a is None}[kind]


def test_edit_counts_against_brute_force():
    n = 0
    for la, lb in itertools.product(range(5), range(6)):
        for ref in itertools.product("ab", repeat=la):
            for hyp in itertools.product("abc", repeat=min(lb, 4)):
                counts, ops = RC.edit_counts(ref, hyp)
                assert sum(counts[1:]) == _brute_distance(ref, hyp)
                _check_ops(ref, hyp, counts, ops)
                assert (counts, ops) == LR.edit_counts(list(ref), list(hyp))
                n += 1
    assert n > 5000
    rng = np.random.RandomState(0)
    for _ in range(50):
        ref, hyp = rng.randint(0, 3, rng.randint(0, 6)).tolist(), rng.randint(0, 3, rng.randint(0, 6)).tolist()
        counts, ops = RC.edit_counts(ref, hyp)
        assert sum(counts[1:]) == _brute_distance(ref, hyp) and (counts, ops) == LR.edit_counts(ref, hyp)


def test_edit_counts_identities_and_backtrace_order():
    seq = ["AA", "B", "CH", "B"]
    assert RC.edit_counts(seq, seq) == ((4, 0, 0, 0), [("hit", i, i) for i in range(4)])
    assert RC.edit_counts([], seq) == ((0, 0, 0, 4), [("ins", None, i) for i in range(4)])
    assert RC.edit_counts(seq, []) == ((0, 0, 4, 0), [("del", i, None) for i in range(4)])
    assert RC.edit_counts([], []) == ((0, 0, 0, 0), [])
    # "ab" -> "b": deleting a or substituting then deleting cost the same 1 / 2; the only distance-1 script deletes a
    assert RC.edit_counts("ab", "b") == ((1, 0, 1, 0), [("del", 0, None), ("hit", 1, 0)])
    # "aa" -> "a": the backtrace takes the diagonal at the end first, so the deletion comes first in sequence order
    assert RC.edit_counts("aa", "a")[1] == [("del", 0, None), ("hit", 1, 0)]
    assert RC.edit_counts("a", "aa")[1] == [("ins", None, 0), ("hit", 0, 1)]
    # a tie between a substitution and a deletion + insertion never arises at unit costs; sub before del at equal cost
    assert RC.edit_counts("ab", "ca")[0] == (0, 2, 0, 0)


# ------------------------------------------------------------------------------------------------ bigram
def test_phone_bigram_counts_and_rows():
    P = 4
    corpus = [[3, 0, 1, 3], [3, 0, 0, 2], [1], []]
    counts, logp = RC.phone_bigram(corpus, P, 0.5)
    want = np.zeros((P + 1, P + 1))
    want[P, 3], want[P, 1] = 2, 1                                          # starts
    want[3, 0], want[0, 1], want[1, 3], want[0, 0], want[0, 2] = 2, 1, 1, 1, 1
    want[3, P], want[2, P], want[1, P] = 1, 1, 1                           # ends
    assert np.array_equal(counts, want)
    assert np.abs(np.exp(logp).sum(axis=1) - 1.0).max() <= 1e-12
    assert logp[P, P] == NINF and np.isfinite(logp[:P]).all() and np.isfinite(logp[P, :P]).all()
    assert abs(np.exp(logp[3, 0]) - 2.5 / (3 + 2.5)) <= 1e-12 and abs(np.exp(logp[P, 3]) - 2.5 / (3 + 2.0)) <= 1e-12
    c2, l2 = LR.phone_bigram(corpus, P, 0.5)
    assert np.array_equal(counts, c2) and np.array_equal(logp, l2)
    assert np.array_equal(RC.bigram_logprob(counts, 0.5), logp)
    with pytest.raises(ValueError):
        RC.phone_bigram([[0, P]], P)
