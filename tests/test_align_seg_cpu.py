"""CPU: the segmental oracle (tests/align_seg_ref.py) against a brute-force enumeration and the relations of the "Segmental scores"
paragraph, the host layer of fastspeech2_amd.align against it (segment table, candidates, reductions, the scores file's rows and
summary, the byte budget), and the census of the seeded inputs of tests/align_seg_cases.py that the GPU test relies on."""
import json

import numpy as np
import pytest

from fastspeech2_amd import align as A
from tests import align_corpus as C
from tests import align_score_cases as K
from tests import align_score_ref as SR
from tests import align_seg_cases as GK
from tests import align_seg_ref as GR
from tests import align_trans_ref as TR

TOL = 1e-9                                                                 # two fp64 orders of summation of at most 200 terms


def test_recursion_is_the_brute_force_maximum():
    """every path is scored in the recursion's own order and fp64 addition is monotone, so the two are equal bit for bit"""
    rng = np.random.RandomState(3)
    n_checked = 0
    for S in (1, 2, 3):
        for n in range(max(S - 1, 1), 8):
            for _ in range(6):
                Fc = 5.0 * rng.randn(n, S)
                loop = rng.uniform(0.05, 0.95, S)
                for ws, wn in ((np.zeros(S), np.zeros(S)), (np.log(loop), np.log(1.0 - loop))):
                    V, mag = GR.scan(Fc, ws, wn)
                    assert V == GR.brute(Fc, ws, wn), (S, n)
                    assert (V == -np.inf) == (n < S)
                    n_checked += 1
    for i in range(len(GK.CASES)):                                         # and every short segment of the committed cases
        case = GK.seg_case(i)
        S = case["S"]
        for f, seg, cand, (V, _) in zip(case["fs"], case["seg"], case["cand"], case["want"]):
            F = SR.class_scores(f, case["w"], case["mu"], case["var"])
            for k, (a, n) in enumerate(seg):
                if not 0 < n <= 7 or np.isnan(V[k]).all():
                    continue
                for q in range(min(case["P"], 12)):
                    c = cand[k, q * S:(q + 1) * S]
                    assert V[k, q] == GR.brute(F[a:a + n][:, c], case["arc"][c, 0], case["arc"][c, 1])
                    n_checked += 1
    assert n_checked > 400


def test_cases_cover_what_the_kernel_makes_special():
    assert {c[0] for c in GK.CASES} == {1, 2, 3} and {c[2] for c in GK.CASES} == {1, 17, 40} and {c[3] for c in GK.CASES} == {1, 3}
    assert {c[0] * c[1] for c in GK.CASES} >= {1, 63, 64, 66, 3 * GK.COLUMN_TILE + 3}
    for i, (S, P, D, M, arcs, tri) in enumerate(GK.CASES):
        case = GK.seg_case(i)
        ns = {int(n) for seg in case["seg"] for n in seg[:, 1]}
        assert ns >= {S - 1, S, S + 1, 15, 16, 17, 64, 65, 130, 0}
        assert (case["arc"] != 0).any() == arcs and (case["w"] == 0).any() == (M > 1)
        lens = [len(f) for f in case["fs"]]
        assert lens[2] + 7 < max(lens)                                     # a row shorter than the batch
        for f, seg, cand, (V, mag) in zip(case["fs"], case["seg"], case["cand"], case["want"]):
            real = seg[:, 1] > 0
            assert seg[real, 1].sum() - (10 if len(f) == lens[2] else 0) == len(f)             # the blocks partition the frames
            absent = np.isnan(V).all(axis=1)
            bad = (seg[:, 1] <= 0) | (seg[:, 0] + seg[:, 1] > len(f)) | (cand < 0).any(axis=1)
            assert np.array_equal(absent, bad) and not np.isnan(V[~absent]).any()
            assert np.array_equal(np.isneginf(V[~absent]).all(axis=1), seg[~absent, 1] < S)
            assert np.isfinite(V[~absent][seg[~absent, 1] >= S]).all()
        assert (case["cand"][0] < 0).any() and (case["seg"][2][-1].sum() > lens[2])
        if tri:
            assert any((c[0] != c[1]).any() for c in case["cand"])         # the candidates depend on the block


def test_rival_census_of_the_gpu_comparison():
    """The GPU test compares the rival where its lead over the next candidate exceeds MARGIN |V|; on these inputs that leaves out at
    most 1 % of the segments."""
    total = out = 0
    for i in range(len(GK.CASES)):
        case = GK.seg_case(i)
        for seg, phone, (V, _) in zip(case["seg"], case["phone"], case["want"]):
            for k, (a, n) in enumerate(seg):
                if np.isnan(V[k]).any() or n < case["S"] or case["P"] < 3:
                    continue
                r, margin, gop_seg, gap = GR.rival(V[k], int(phone[k]), int(n))
                total += 1
                out += int(not gap > GK.MARGIN * abs(V[k, r]))
                assert gop_seg <= 0.0 and gop_seg == min(margin, 0.0) and r != phone[k]
    print("segments", total, "left out of the rival comparison", out)
    assert total >= 50 and out <= 0.01 * total


@pytest.mark.parametrize("transitions", (0, 1))
def test_relations_on_a_decoded_path(transitions):
    """On the reference's own decode of the substituted-word utterances: V[k, p] is the forced path's score over the segment
    (never below it, equal up to rounding) and, without transitions, gop <= gop_seg <= 0 per block."""
    mu, var, n_classes, cases = K.substitution()
    S, P = C.STATES, n_classes // C.STATES
    phone = SR.class_phone_mono(n_classes, S)
    rng = np.random.RandomState(5)
    loop, opt = (rng.uniform(0.2, 0.8, n_classes), np.array([0.4, 0.3, 0.6])) if transitions else (np.full(n_classes, 0.5), np.full(3, 0.5))
    arc = np.stack([np.log(loop), np.log(1.0 - loop)], 1) if transitions else np.zeros((n_classes, 2))
    decode = (lambda E, g: TR.viterbi(E, g, *TR.arc_costs(g, loop, opt))) if transitions else SR.plain_decode
    tables = SR.as_mixture(mu, var)
    blocks = 0
    for x, _, gs, _, _ in cases[:4]:
        frames, red, (state, own, best, arg, _) = SR.score(x, gs, *tables, phone, decode)
        F = SR.class_scores(x, *tables)
        want = GR.utterance(F, gs, gs, state, GR.candidates(gs, A.phone_table({"w": C.PHONES}), S), arc, S)
        assert np.array_equal(want["seg"][:, 1], frames)
        for k, n in enumerate(frames):
            if n == 0:
                assert np.isnan(want["blocks"][k]).all()
                continue
            p = int(gs["sid"][k * S]) // S
            scale = want["mag"][k, p]
            assert want["V"][k, p] >= want["forced"][k] - TOL * scale and abs(want["V"][k, p] - want["forced"][k]) <= TOL * scale
            gop_seg = want["blocks"][k, 0]
            assert gop_seg <= 0.0
            if not transitions:
                assert red["blocks"][k, 1] <= gop_seg + TOL * scale / n
                assert (want["V"][k] <= np.cumsum(best[want["seg"][k, 0]:][:n])[-1] + TOL * scale).all()
            blocks += 1
        assert want["gop_seg"] <= 0.0
        # the product's host layer is the oracle's
        assert np.array_equal(A.segment_table(gs, state), want["seg"])
        got, utt = A.segment_reductions(gs, want["seg"], want["V"])
        assert np.allclose(got, want["blocks"], rtol=1e-12, atol=0, equal_nan=True) and np.isclose(utt, want["gop_seg"], rtol=1e-12, atol=0)
    assert blocks > 40


def test_a_substituted_word_loses_to_a_rival_on_the_reference():
    """The 8 cases of `align_score_cases.substitution()` on the reference alone: the frame-weighted mean `margin` of the substituted
    word's phones is negative and below the mean over the untouched words in all 8 (-8.79 / 9.87, -9.98 / 9.13, -9.34 / 8.27,
    -11.35 / 8.68, -9.39 / 8.64, -6.25 / 9.33, -5.62 / 10.07, -8.55 / 5.17): the ordering the GPU test asserts."""
    mu, var, n_classes, cases = K.substitution()
    S, ids = C.STATES, A.phone_table({"w": C.PHONES})
    tables, phone, arc = SR.as_mixture(mu, var), SR.class_phone_mono(n_classes, C.STATES), np.zeros((n_classes, 2))
    assert len(cases) == 8
    for x, _, gs, sub, rest in cases:
        fr, _, (state, _, _, _, _) = SR.score(x, gs, *tables, phone, SR.plain_decode)
        want = GR.utterance(SR.class_scores(x, *tables), gs, gs, state, GR.candidates(gs, ids, S), arc, S)
        mean = lambda ks: sum(want["blocks"][k, 2] * fr[k] for k in ks if fr[k] > 0) / sum(fr[k] for k in ks if fr[k] > 0)  # noqa: E731
        print("margin of the substituted word", mean(sub), "of the others", mean(rest), "utterance gop_seg", want["gop_seg"])
        assert mean(sub) < 0.0 < mean(rest)


def small_tree_aligner():
    """phones X, Y, Z, sil, sp, spn with two states; three splits: root (X, 0) on the left context, its yes child on the right
    context, root (Y, 1) on the right context.  Sets: {X, #}, {Z}, {Y, Z}."""
    lex = {"xyz": ["X", "Y", "Z"], "zx": ["Z", "X"], "yy": ["Y", "Y"]}
    ids = A.phone_table(lex)
    S, n_roots, bnd = 2, len(ids) * 2, len(ids)
    member = np.zeros((3, bnd + 1), np.uint8)
    member[0, [ids["X"], bnd]] = 1
    member[1, ids["Z"]] = 1
    member[2, [ids["Y"], ids["Z"]]] = 1
    n = n_roots + 6
    question, yes, no = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    question[0], yes[0], no[0] = 0, n_roots, n_roots + 1                   # (X, 0): is l in {X, #}?
    question[ids["Y"] * S + 1], yes[ids["Y"] * S + 1], no[ids["Y"] * S + 1] = 3 + 1, n_roots + 2, n_roots + 3      # (Y, 1): is r in {Z}?
    question[n_roots], yes[n_roots], no[n_roots] = 3 + 2, n_roots + 4, n_roots + 5                                  # is r in {Y, Z}?
    leaf = np.full(n, -1)
    is_leaf = question < 0
    leaf[is_leaf] = np.arange(int(is_leaf.sum()))
    al = A.Aligner.__new__(A.Aligner)
    al.states, al.n_mono, al.n_classes, al.triphones, al.phone_ids = S, n_roots, int(is_leaf.sum()), int(is_leaf.sum()), ids
    al.tree = {"question": question, "yes": yes, "no": no, "leaf": leaf, "member": member, "n_leaves": int(is_leaf.sum())}
    return al, lex, ids


def test_segment_table_and_candidates():
    al, lex, ids = small_tree_aligner()
    S, P = 2, len(ids)
    g = A.utterance_graph(["xyz", "unknown", "zx", "yy"], lex, ids, S)
    # a path that skips the first sil and the sp before the last word
    frames = np.array([0, 2, 3, 2, 1, 2, 1, 2, 2, 0, 3, 2, 4])
    assert len(frames) == len(g["blocks"])
    state = np.concatenate([[k * S] * (n - n // 2) + [k * S + 1] * (n // 2) for k, n in enumerate(frames)]).astype(np.int64)
    seg = A.segment_table(g, state)
    assert np.array_equal(seg, GR.segment_table(g, state)) and np.array_equal(seg[:, 1], frames)
    assert np.array_equal(seg[frames > 0, 0], np.cumsum(frames)[frames > 0] - frames[frames > 0])

    mono = A.Aligner.__new__(A.Aligner)
    mono.states, mono.n_mono, mono.triphones = S, P * S, 0
    assert np.array_equal(mono.candidates(g), GR.candidates(g, ids, S)) and mono.candidates(g).dtype == np.int32
    assert (mono.candidates(g) == np.arange(P * S)).all()

    got, want = al.candidates(g), GR.candidates(g, ids, S, al.tree)
    assert got.shape == (len(g["blocks"]), P * S) and got.dtype == np.int32 and np.array_equal(got, want)
    assert (got >= 0).all() and (got < al.n_classes).all()
    # the transcript's own phone gets the classes the path is decoded on
    sid = al._leaf_graph(g)["sid"]
    for k in range(len(g["blocks"])):
        p = int(g["sid"][k * S]) // S
        assert np.array_equal(got[k, p * S:(p + 1) * S], sid[k * S:(k + 1) * S])
    # contexts no transcript of this lexicon has: X before Y at a word's start (block 10, the first Y of `yy`, has l = #, r = Y)
    x, y, z, bnd = ids["X"], ids["Y"], ids["Z"], len(ids)
    k = 10
    assert g["blocks"][k][0] == "Y" and g["blocks"][k + 1][0] == "Y"
    assert got[k, x * S] == GR.leaf_of(al.tree, 3, x, 0, bnd, y, S)        # l = # is in {X, #}, then r = Y is in {Y, Z}
    k = 2                                                                  # Y of `xyz`: l = X, r = Z
    assert got[k, y * S + 1] == GR.leaf_of(al.tree, 3, y, 1, x, z, S) != got[10, y * S + 1]
    assert got[k, x * S] == GR.leaf_of(al.tree, 3, x, 0, x, z, S)
    # context-independent on either side: `#` both ways
    spn_block = 5
    assert g["blocks"][spn_block][0] == A.SPN
    assert got[spn_block, x * S] == GR.leaf_of(al.tree, 3, x, 0, bnd, bnd, S)
    assert (got[:, ids[A.SIL] * S] == got[0, ids[A.SIL] * S]).all()


def test_rows_and_summary_of_a_hand_written_file(tmp_path):
    rows = [{"speaker": "s", "basename": f"u{i}", "frames": 10, "scored_frames": 5 + i, "viterbi": -1.0, "loglik": -2.0, "gop": -0.1 * i,
             "match": 1.0, "gop_seg": -0.01 * i,
             "phones": [["AH", 0.0, 0.1, -2.0, -0.1, 1.0, -0.5, "IY", -0.5], ["B", 0.1, 0.2, -2.0, 0.0, 1.0, 0.0, "D", 0.25],
                        ["AH", 0.2, 0.3, -2.0, -0.1, 1.0, -0.5, "IY" if i % 2 else "EH", -0.5], ["sp", 0.3, 0.4, -2.0, 0.0, 1.0, None, None, 0]]}
            for i in range(4)]
    path = tmp_path / "scores.jsonl"
    path.write_text("".join(json.dumps(r) + "\n" for r in rows))
    text = A.scores_summary(str(path))
    mean = sum(-0.01 * i * (5 + i) for i in range(4)) / sum(5 + i for i in range(4))
    assert text.startswith("scores: 4 utterances, mean gop ") and f"; mean gop_seg {mean:.4f}; " in text
    assert text.endswith("intervals that lose to a rival: 8; most frequent: AH -> IY 6, AH -> EH 2")
    plain = [{k: v for k, v in r.items() if k != "gop_seg"} for r in rows]
    for r in plain:
        r["phones"] = [p[:6] for p in r["phones"]]
    path.write_text("".join(json.dumps(r) + "\n" for r in plain))
    assert "gop_seg" not in A.scores_summary(str(path)) and text.startswith(A.scores_summary(str(path)))
    # 25 pairs: the 20 most frequent, ties in label order
    many = dict(rows[0], phones=[[f"P{j:02d}", 0.0, 0.1, -2.0, -0.1, 1.0, -0.5, "R", -0.5] for j in range(25)] * 2)
    path.write_text(json.dumps(many) + "\n")
    text = A.scores_summary(str(path))
    assert text.count(" -> R 2") == 20 and "P19 -> R 2" in text and "P20" not in text


def test_reductions_of_one_phone_and_of_ties():
    g = {"blocks": [("a", 0, False), ("a", 0, False)], "sid": np.array([0, 0], np.int32)}
    got, utt = A.segment_reductions(g, np.array([[0, 3], [0, 0]]), np.array([[-7.0], [np.nan]]))
    assert np.isnan(got[0, :2]).all() and got[0, 2] == 0.0 and np.isnan(got[1]).all() and np.isnan(utt)
    g = {"blocks": [("b", 0, False), ("a", 1, True)], "sid": np.array([1, 0], np.int32)}
    V = np.array([[-5.0, -9.0, -5.0, -6.0], [-4.0, -4.0, -4.0, -8.0]])
    got, utt = A.segment_reductions(g, np.array([[0, 4], [4, 2]]), V)
    assert got[0].tolist() == [-1.0, 0.0, -1.0] and got[1].tolist() == [0.0, 1.0, 0.0] and utt == -1.0    # the lowest rival on ties
    for k, p, n in ((0, 1, 4), (1, 0, 2)):
        r, margin, gop_seg, _ = GR.rival(V[k], p, n)
        assert got[k].tolist() == [gop_seg, r, margin]


def test_byte_budget_counts_the_segment_buffers():
    frames, states = [400] * 8, [120] * 8
    batches = lambda budget, **kw: [list(b) for b in A.batches_by_bytes(frames, states, 160, budget, **kw)]     # noqa: E731
    plain = batches(40 << 20)
    assert batches(40 << 20, seg_phones=0) == plain
    more = batches(40 << 20, seg_phones=256, block_states=2)
    assert len(more) >= len(plain) and sorted(i for b in more for i in b) == list(range(8))
    # 60 blocks x (8 + 256 x (4 x 2 + 8)) bytes an utterance: a budget that held all eight without them holds fewer with them
    base = 400 * 120 * 17 + 400 * 160 * 8 + 120 * 321 * 8
    budget = 8 * base + 1000
    assert len(batches(budget)) == 1
    assert len(batches(budget, seg_phones=256, block_states=2)) > 1
    assert len(batches(budget + 8 * 60 * (8 + 256 * 16), seg_phones=256, block_states=2)) == 1
