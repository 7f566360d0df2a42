"""CPU: the numpy oracle of the aligner's triphone stage (tests/align_tri_ref.py) on the context-dependent corpus of
tests/align_tri_corpus.py, and the product's host code (fastspeech2_amd.align: contexts, generated questions, the questions file,
tree, replay, walk) against its defining properties and against the oracle's.  `kernel_case` builds the seeded inputs that
tests/test_align_tri_gpu.py gives the kernel; here the oracle's own margins on them are checked."""
import functools

import numpy as np
import pytest

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_ref as R
from tests import align_tri_corpus as TC
from tests import align_tri_ref as TR

# the accuracy measurement: 30 utterances, 6 passes, 54 leaves (30 roots and fixed leaves + one split per real root), 3 passes on them
ACC_SEEDS, ACC_N_UTT, ACC_ITERS, ACC_LEAVES, ACC_TRI_ITERS, ACC_MIN_OCC = (1234, 1235, 1236), 30, 6, 54, 3, 20.0
ACC_MONO = {1234: 0.8278, 1235: 0.7484, 1236: 0.7347}
ACC_TRI = {1234: 0.8576, 1235: 0.7981, 1236: 0.7703}
# the end-to-end comparison on the GPU
E2E_SEED, E2E_N_UTT, E2E_ITERS, E2E_LEAVES, E2E_TRI_ITERS, E2E_MIN_OCC = 1234, 30, 6, 54, 3, 20.0

LEX = {"ab": ["AA", "B"], "solo": ["K"], "abc": ["AA", "B", "CH"], "sil": ["sil"]}
IDS = A.phone_table(LEX)


def prepared(lex, utts):
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    return ids, graphs, [R.features(u["mel"]) for u in utts]


@functools.lru_cache(maxsize=None)
def mono(seed, n, iters):
    """the monophone oracle of TC.corpus(seed, n), shared by the tests: (ids, graphs, xs, true durations, model, front)"""
    lex, utts = TC.corpus(seed, n)
    ids, graphs, xs = prepared(lex, utts)
    m = TR.fit(xs, graphs, ids, C.STATES, iters, 0)
    front = (xs, m["mu"], m["var"], 1e-2 * np.concatenate(xs).var(axis=0), m["history"], 0.0)
    return ids, graphs, xs, [[d for _, d in u["segments"]] for u in utts], m, front


@functools.lru_cache(maxsize=None)
def tri(seed):
    """the triphone oracle of the accuracy measurement (and of the GPU end-to-end comparison) on top of `mono`"""
    ids, graphs, xs, _, _, front = mono(seed, ACC_N_UTT, ACC_ITERS)
    return TR.fit(xs, graphs, ids, C.STATES, ACC_ITERS, ACC_LEAVES, ACC_TRI_ITERS, ACC_MIN_OCC, front=front)


def test_triphones_zero_is_the_monophone_oracle():
    ids, graphs, xs, _, m, _ = mono(E2E_SEED, 6, 2)
    mu, var, hist = R.fit(xs, graphs, len(ids) * C.STATES, 2)
    assert np.array_equal(m["mu"], mu) and np.array_equal(m["var"], var) and m["history"] == hist and "tree" not in m
    assert all(np.array_equal(TR.align(x, g, m), R.align(x, g, mu, var)) for x, g in zip(xs, graphs))


def test_contexts_at_word_edges_one_phone_words_spn_and_sp():
    bnd = len(IDS)
    g = A.utterance_graph(["abc", "solo", "zzz", "ab"], LEX, IDS, 2)       # sil AA B CH sp K sp spn sp AA B sil
    assert [b[0] for b in g["blocks"]] == ["sil", "AA", "B", "CH", "sp", "K", "sp", "spn", "sp", "AA", "B", "sil"]
    ctx = A.triphone_contexts(g, IDS, 2)
    assert ctx.shape == (24, 4) and ctx.dtype == np.int32 and np.array_equal(ctx, TR.contexts(g, IDS, 2))
    want = [(bnd, "sil", bnd), (bnd, "AA", IDS["B"]), (IDS["AA"], "B", IDS["CH"]), (IDS["B"], "CH", bnd), (bnd, "sp", bnd),
            (bnd, "K", bnd), (bnd, "sp", bnd), (bnd, "spn", bnd), (bnd, "sp", bnd), (bnd, "AA", IDS["B"]), (IDS["AA"], "B", bnd),
            (bnd, "sil", bnd)]
    for k, (l, p, r) in enumerate(want):
        for s in range(2):
            assert tuple(ctx[2 * k + s]) == (l, IDS[p], r, s), (k, s)
    # the context does not depend on whether an optional sp is taken: it is a function of the transcript alone, and the graph's
    # topology is what utterance_graph made
    keys = set(A.utterance_graph(["ab"], LEX, IDS, 2))
    assert keys == {"sid", "skip", "block", "alt", "blocks", "mandatory"}
    for states in (1, 3):
        g3 = A.utterance_graph(["abc", "ab"], LEX, IDS, states)
        c3 = A.triphone_contexts(g3, IDS, states)
        assert np.array_equal(c3, TR.contexts(g3, IDS, states)) and np.array_equal(c3[:, 1] * states + c3[:, 3], g3["sid"])
    with pytest.raises(ValueError):
        A.triphone_contexts(g, IDS, 3)


@functools.lru_cache(maxsize=None)
def small():
    """item sums of a small corpus under a briefly trained monophone table: (ids, items, sums, floor, pooled monophone sums)"""
    ids, graphs, xs, _, m, front = mono(E2E_SEED, 12, 2)
    ctxs = [TR.contexts(g, ids, C.STATES) for g in graphs]
    items = TR.item_table(ctxs)
    parts = [R.partials(R.posteriors(R.emissions(x, g["sid"], m["mu"], m["var"]), g)[0], x) for x, g in zip(xs, graphs)]
    sums = TR.item_sums(parts, ctxs, items)
    pooled = np.zeros((len(ids) * C.STATES, sums.shape[1]))
    for i, k in enumerate(items):
        pooled[k[0] * C.STATES + k[1]] += sums[i]
    return ids, items, sums, front[3], pooled


def real_phones(ids):
    return [p for name, p in ids.items() if name not in TR.CI]


def test_generated_questions():
    ids, items, sums, floor, pooled = small()
    P, n_sym = len(real_phones(ids)), len(ids) + 1
    names, member = A.phone_questions(pooled, real_phones(ids), C.STATES, floor, n_sym)
    assert member.shape == (2 * P - 1, n_sym) and member.dtype == np.uint8 and len(names) == 2 * P - 1
    sets = [frozenset(np.nonzero(r)[0]) for r in member]
    assert sets[:P] == [frozenset([p]) for p in sorted(real_phones(ids))] and sets[-1] == frozenset([n_sym - 1])
    assert frozenset(real_phones(ids)) not in sets and len(set(sets)) == len(sets)
    for a in sets:                                                         # nested: two sets are disjoint or one holds the other
        for b in sets:
            assert not (a & b) or a <= b or b <= a
    assert max(len(s) for s in sets) < P and all(not (s & {ids[c] for c in TR.CI}) for s in sets)
    assert np.array_equal(A.phone_questions(pooled, real_phones(ids), C.STATES, floor, n_sym)[1], member)     # deterministic
    assert np.array_equal(TR.questions(pooled, real_phones(ids), C.STATES, floor, n_sym), member)             # and the oracle's


def test_questions_file(tmp_path):
    path = tmp_path / "q.txt"
    path.write_text("vowel AA\n\nstops B  K CH\nedge #\n")
    names, member = A.read_questions(str(path), IDS)
    assert names == ["vowel", "stops", "edge"] and member.shape == (3, len(IDS) + 1) and member.dtype == np.uint8
    assert [sorted(np.nonzero(r)[0]) for r in member] == [[IDS["AA"]], sorted([IDS["B"], IDS["K"], IDS["CH"]]), [len(IDS)]]
    for text in ("vowel AA XX\n", "lonely\n", "\n"):
        path.write_text(text)
        with pytest.raises(ValueError):
            A.read_questions(str(path), IDS)


def oracle_gains_of(items, sums, member, floor, min_occ):
    left, right = np.array([k[2] for k in items]), np.array([k[3] for k in items])
    return lambda nodes: TR.best(TR.gains(sums, left, right, nodes, member, floor, min_occ)[0])


@functools.lru_cache(maxsize=None)
def small_tree(min_occ=5.0):
    ids, items, sums, floor, pooled = small()
    member = TR.questions(pooled, real_phones(ids), C.STATES, floor, len(ids) + 1)
    fixed = sorted(ids[p] * C.STATES + s for p in TR.CI for s in range(C.STATES))
    nodes = TR.grow(items, C.STATES, len(ids), set(fixed), sums, member, floor, min_occ, 0.0)
    keys = np.array(items)
    full = A.tree_build(keys, keys[:, 0] * C.STATES + keys[:, 1], len(ids) * C.STATES, fixed, member,
                        oracle_gains_of(items, sums, member, floor, min_occ))
    return ids, items, sums, floor, member, nodes, full


def test_tree_splits_gain_and_conserve_the_sums():
    ids, items, sums, floor, member, nodes, full = small_tree()
    n_roots = len(ids) * C.STATES
    assert len(nodes) > n_roots + 20 and len(full["question"]) == len(nodes)
    assert max(len(n["items"]) for n in nodes[n_roots:]) > 1               # more than one level
    for m, n in enumerate(nodes):                                          # the product's tree is the oracle's
        assert (full["question"][m], full["yes"][m], full["no"][m]) == (n["q"], n["yes"], n["no"])
        assert np.array_equal(full["items"][m], n["items"])
        if n["q"] >= 0:
            assert n["gain"] > 0.0 and full["gain"][m] == n["gain"]
            y, no = nodes[n["yes"]]["items"], nodes[n["no"]]["items"]
            assert sorted(np.concatenate([y, no])) == sorted(n["items"]) and len(y) and len(no)
            assert sums[y, 0].sum() >= 5.0 and sums[no, 0].sum() >= 5.0
            tot = sums[n["items"]].sum(axis=0)
            assert np.abs(sums[y].sum(axis=0) + sums[no].sum(axis=0) - tot).max() <= 1e-9 * np.abs(tot).max()
    for p in TR.CI:                                                        # sil, sp and spn are never split
        for s in range(C.STATES):
            assert nodes[ids[p] * C.STATES + s]["q"] == -1


def test_replay_is_best_first_splitting():
    ids, items, sums, floor, member, nodes, full = small_tree()
    n_roots, n_splits = len(ids) * C.STATES, sum(1 for n in nodes if n["q"] >= 0)
    for budget in (n_roots, n_roots + 1, n_roots + 7, n_roots + n_splits // 2, n_roots + n_splits, n_roots + n_splits + 50):
        question, yes, no, leaf, total = A.tree_replay(full, n_roots, budget)
        rq, ry, rn, rl, rt = TR.replay(nodes, n_roots, budget)
        assert np.array_equal(question, rq) and np.array_equal(yes, ry) and np.array_equal(no, rn) and np.array_equal(leaf, rl)
        assert total == rt
        split = TR.best_first(nodes, n_roots, budget)
        assert set(np.nonzero(question >= 0)[0]) == split
        n_leaves = int(leaf.max()) + 1
        assert n_leaves == min(budget, n_roots + n_splits) == n_roots + len(split)
        assert sorted(leaf[leaf >= 0]) == list(range(n_leaves))
        got = A.tree_leaves(question, yes, no, leaf, member, np.array(items), C.STATES)
        assert np.array_equal(got, [TR.walk((rq, ry, rn, rl), member, k, C.STATES) for k in items])
    with pytest.raises(ValueError):
        A.tree_replay(full, n_roots, n_roots - 1)
    with pytest.raises(ValueError):
        TR.replay(nodes, n_roots, n_roots - 1)


def test_an_unseen_triple_reaches_a_leaf():
    ids, items, sums, floor, member, nodes, full = small_tree()
    n_roots = len(ids) * C.STATES
    question, yes, no, leaf, _ = A.tree_replay(full, n_roots, n_roots + 40)
    seen, bnd = set(items), len(ids)
    unseen = [(p, s, l, r) for p in real_phones(ids) for s in range(C.STATES) for l in real_phones(ids) + [bnd] for r in real_phones(ids) + [bnd]
              if (p, s, l, r) not in seen]
    assert len(unseen) > 1000
    got = A.tree_leaves(question, yes, no, leaf, member, np.array(unseen), C.STATES)
    assert (got >= 0).all() and (got <= leaf.max()).all()
    for k, lf in list(zip(unseen, got))[::97]:
        assert lf == TR.walk((question, yes, no, leaf), member, k, C.STATES)
        m = int(np.nonzero(leaf == lf)[0][0])                              # the leaf hangs under the triple's own root
        assert full["root"][m] == k[0] * C.STATES + k[1]


@pytest.mark.parametrize("seed", ACC_SEEDS)
def test_triphones_beat_the_monophones_on_context_dependent_means(seed):
    """Share of the true phone boundaries found within +-1 frame by the two oracles on TC.corpus(seed, 30) (SEP 0.1, VSEP 4, GSEP 2),
    6 passes, then 54 leaves with tri_min_occ = 20 and 3 passes on them, measured on the host:
        seed 1234: monophones 0.8278, triphones 0.8576
        seed 1235: monophones 0.7484, triphones 0.7981
        seed 1236: monophones 0.7347, triphones 0.7703
    The smallest gap is 0.0298 (seed 1234); the triphones have to win by half of it, because the gap varies by seed."""
    gap = min(ACC_TRI[s] - ACC_MONO[s] for s in ACC_SEEDS)
    assert abs(gap - 0.0298) < 1e-9
    ids, graphs, xs, true, m0, front = mono(seed, ACC_N_UTT, ACC_ITERS)
    a_mono = C.accuracy(true, [TR.align(x, g, m0) for x, g in zip(xs, graphs)], 1)
    m1 = tri(seed)
    a_tri = C.accuracy(true, [TR.align(x, g, m1) for x, g in zip(xs, graphs)], 1)
    print("seed", seed, "monophones", a_mono, "triphones", a_tri, "leaves", m1["n_leaves"], "items", len(m1["items"]), "gain", m1["tree"][4])
    assert m1["n_leaves"] == ACC_LEAVES and len(m1["history"]) == ACC_ITERS + 1 + ACC_TRI_ITERS and np.isfinite(m1["history"]).all()
    assert a_tri >= a_mono + 0.5 * gap, (a_mono, a_tri)


# ------------------------------------------------------------------------------------------------ the kernel's test inputs
KERNEL_DIMS, KERNEL_SETS, KERNEL_MIN_OCC = (3, 16, 40, 160), (1, 15, 16, 17, 33), 8.0
N_SYM = 9
GENERIC = (1, 3, 4, 5, 17, 65)                                             # items per node: under, at and over the instruction's k = 4


def kernel_case(D, n_sets, seed=0):
    """Seeded inputs of one launch -> dict(sums (N, 1 + 2 D), left, right, nodes, member, floor, special).  Six generic nodes of 1, 3,
    4, 5, 17 and 65 items with continuous n in [3, 12), class-like means and variances, random contexts, one item of the 17 with n = 0
    (an all-zero row); then four special nodes whose n are small multiples of 2^-50, so that every partial sum of them is exact in
    any order: `all_yes` (every item answers yes to question 0), `at` (the yes side of question 0 has n = 8 = min_occ exactly, the no
    side more), `below` (the yes side has n = 8 - 2^-50) and `no_at` (the no side has n = 8 exactly).  Set 0 holds symbol 0 and not
    symbol 1; the special nodes use those two symbols on the left."""
    rng = np.random.RandomState(1000 * D + n_sets + 7919 * seed)
    member = (rng.rand(n_sets, N_SYM) < 0.5).astype(np.uint8)
    member[0, 0], member[0, 1] = 1, 0
    special_n = {"all_yes": ([3.0, 5.0, 4.0, 6.0], [0, 0, 0, 0]), "at": ([3.0, 5.0, 9.0, 2.0], [0, 0, 1, 1]),
                 "below": ([3.0, np.nextafter(5.0, 0.0), 9.0, 2.0, 7.0], [0, 0, 1, 1, 1]), "no_at": ([6.0, 7.0, 3.0, 5.0], [0, 0, 1, 1])}
    N = sum(GENERIC) + sum(len(v[0]) for v in special_n.values())
    n = rng.uniform(3.0, 12.0, N)
    left, right = rng.randint(0, N_SYM, N), rng.randint(0, N_SYM, N)
    nodes, at = [], 0
    for size in GENERIC:
        nodes.append(np.arange(at, at + size))
        at += size
    n[nodes[4][5]] = 0.0
    special = {}
    for name, (ns, ls) in special_n.items():
        idx = np.arange(at, at + len(ns))
        n[idx], left[idx] = ns, ls
        special[name] = len(nodes)
        nodes.append(idx)
        at += len(ns)
    mean = rng.randn(N, D) + 0.5 * rng.randn(D)[None, :]
    var = rng.uniform(0.5, 1.5, (N, D))
    sums = np.concatenate([n[:, None], n[:, None] * mean, n[:, None] * (var + mean * mean)], axis=1)
    order = rng.permutation(N)                                             # the rows of the table in another order than the lists
    inv = np.argsort(order)
    return {"sums": sums[order], "left": left[order].astype(np.int32), "right": right[order].astype(np.int32),
            "nodes": [inv[it] for it in nodes], "member": member, "floor": np.full(D, 1e-2) * rng.uniform(0.5, 1.5, D), "special": special}


@functools.lru_cache(maxsize=None)
def kernel_reference(D, n_sets):
    """-> (case, oracle gains, n_yes, n_no, bound, unsure, bound of n_yes), computed once and shared.  At the special nodes every n
    is a small multiple of 2^-50 and every partial sum of them is exact in any order, so eligibility is exact there whatever the
    bound says: `unsure` is cleared for them."""
    c = kernel_case(D, n_sets)
    g, ny, nn = TR.gains(c["sums"], c["left"], c["right"], c["nodes"], c["member"], c["floor"], KERNEL_MIN_OCC)
    bound, unsure, eny = TR.gain_bounds(c["sums"], c["left"], c["right"], c["nodes"], c["member"], c["floor"], KERNEL_MIN_OCC)
    for m in c["special"].values():
        unsure[m] = False
    return c, g, ny, nn, bound, unsure, eny


def decided(c, g, bound, unsure):
    """per node the question the kernel must report, or -2 where the oracle cannot tell.  Two questions that part a node's items the
    same way (or the other way round: the two sides change places) have the same sums in the same order, so their gains are equal
    bit for bit, in the oracle and in the kernel, and the lowest of them is reported; the best partition must lead every other one
    by more than twice the bound (of either), no side of the node may be `unsure`, and -1 is expected when no split is eligible."""
    out = np.full(len(g), -2)
    for m, items in enumerate(c["nodes"]):
        if unsure[m].any():
            continue
        if not np.isfinite(g[m]).any():
            out[m] = -1
            continue
        ans = TR._answers(c["member"], c["left"], c["right"], items)
        key = [min(tuple(a), tuple(~a)) for a in ans]
        top = int(np.argmax(g[m]))
        others = [q for q in range(len(key)) if key[q] != key[top] and np.isfinite(g[m, q])]
        if all(g[m, top] - g[m, q] > 2.0 * max(bound[m, top], bound[m, q]) for q in others):
            out[m] = top
    return out


def test_kernel_inputs_leave_the_oracle_decided():
    """What the best-question comparison of tests/test_align_tri_gpu.py rests on: on the seeded inputs at most 5 % of the nodes have a
    top-two margin within twice the bound (or a side within its bound of the threshold), and the special nodes are what the
    docstring of `kernel_case` says."""
    total = left_out = 0
    for D in KERNEL_DIMS:
        for n_sets in KERNEL_SETS:
            c, g, ny, nn, bound, unsure, _ = kernel_reference(D, n_sets)
            want = decided(c, g, bound, unsure)
            total, left_out = total + len(want), left_out + int((want == -2).sum())
            sp = c["special"]
            assert ny[sp["all_yes"], 0] == 18.0 and nn[sp["all_yes"], 0] == 0.0 and g[sp["all_yes"], 0] == -np.inf
            assert ny[sp["at"], 0] == 8.0 and nn[sp["at"], 0] == 11.0 and np.isfinite(g[sp["at"], 0])
            assert ny[sp["below"], 0] == 8.0 - 2.0 ** -50 and g[sp["below"], 0] == -np.inf
            assert nn[sp["no_at"], 0] == 8.0 and ny[sp["no_at"], 0] == 13.0 and np.isfinite(g[sp["no_at"], 0])
            fin = np.isfinite(g)
            assert fin.sum() >= 2 and np.isfinite(bound[fin]).all() and (bound[fin] < 1e-6 * np.maximum(np.abs(g[fin]), 1.0)).all()
    print("nodes", total, "left out", left_out)
    assert left_out <= 0.05 * total
