"""GPU: the segmental-score kernel (csrc/fs2_align_seg.hip: fs2_align_segment_scores), `Aligner.score(segmental=True)` and
`build(..., seg_scores=1)` against the numpy oracle tests/align_seg_ref.py, on the seeded inputs tests/test_align_seg_cpu.py pins."""
import json
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib, align as A
from fastspeech2_amd import preprocess as P
from tests import align_corpus as C
from tests import align_ref as R
from tests import align_score_cases as K
from tests import align_score_ref as SR
from tests import align_seg_cases as GK
from tests import align_seg_ref as GR
from tests.test_align_cpu import config
from tests.test_align_gpu import RTOL, padded

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 77.0


def up(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def close_to(got, want, scale):
    """the bar of `rel_close` (tests/test_align_gpu.py), taken against the sum of |F| along the reference's best path instead of
    |want|, so that scores of mixed sign cannot tighten it by cancellation"""
    got, want = np.asarray(got), np.asarray(want)
    bad = ~(np.abs(got - want) <= RTOL * np.asarray(scale))
    assert not bad.any(), (np.nonzero(bad), got[bad][:4], want[bad][:4])


def run_segment_scores(dev, case):
    """the ragged batch with NaN padding beyond every T, V a strided view of a wider buffer of guard cells -> numpy V, the buffer"""
    S, P = case["S"], case["P"]
    lens = [len(f) for f in case["fs"]]
    f = padded(case["fs"], NAN, np.float64, dev)
    Kmax = max(len(s) for s in case["seg"])
    seg = np.zeros((len(lens), Kmax, 2), np.int32)
    cand = np.zeros((len(lens), Kmax, P * S), np.int32)
    for b, (s, c) in enumerate(zip(case["seg"], case["cand"])):
        seg[b, :len(s)], cand[b, :len(c)] = s, c
    wide = torch.full((len(lens), Kmax + 2, P + 3), GUARD, dtype=torch.float64, device=dev)
    out = wide[:, :Kmax, :P]
    out.fill_(NAN)
    seg_d, cand_d = up(dev, seg, cand.reshape(len(lens), Kmax, P, S))
    got = A.segment_scores(f, lens, seg_d, cand_d, *up(dev, case["w"], case["mu"], case["var"], case["arc"]), out=out)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy(), wide.cpu().numpy()


def check_against_oracle(case, V):
    compared = total = 0
    for b, (seg, phone, (want, mag)) in enumerate(zip(case["seg"], case["phone"], case["want"])):
        got = V[b, :len(seg)]
        assert np.array_equal(np.isnan(got), np.isnan(want))               # NaN stays where nothing is to be written
        assert np.array_equal(np.isneginf(got), np.isneginf(want))         # -inf exactly where n < S
        fin = np.isfinite(want)
        close_to(got[fin], want[fin], mag[fin])
        assert np.isnan(V[b, len(seg):]).all()                             # the padding blocks (0 frames)
        for k, (a, n) in enumerate(seg):
            if not fin[k].all() or case["P"] < 3:
                continue
            r, _, _, gap = GR.rival(want[k], int(phone[k]), int(n))
            total += 1
            if gap > GK.MARGIN * abs(want[k, r]):
                assert GR.rival(got[k], int(phone[k]), int(n))[0] == r
                compared += 1
    return compared, total


@pytest.mark.parametrize("case", range(len(GK.CASES)), ids=GK.IDS)
def test_segment_scores_against_oracle(dev, case):
    case = GK.seg_case(case)
    V, wide = run_segment_scores(dev, case)
    compared, total = check_against_oracle(case, V)
    print("segments", total, "rival compared on", compared)
    assert compared >= 0.99 * total
    Kmax, P_ = V.shape[1:]
    assert (wide[:, Kmax:] == GUARD).all() and (wide[:, :, P_:] == GUARD).all()    # the guard cells of the wider buffer
    again, _ = run_segment_scores(dev, case)
    assert np.array_equal(V, again, equal_nan=True)                        # a second run is identical


@pytest.mark.parametrize("M", (1, 3))
def test_equal_rows_give_equal_bits_and_the_lower_phone_is_the_rival(dev, M):
    case, (lo, twins) = GK.twin_case(M)
    V, _ = run_segment_scores(dev, case)
    check_against_oracle(case, V)
    for k, (a, n) in enumerate(case["seg"][0]):
        for q in twins:
            assert V[0, k, q] == V[0, k, lo]                               # bit for bit, across column tiles
        assert np.argmax(V[0, k]) == lo and GR.rival(V[0, k], int(case["phone"][0][k]), int(n))[0] == lo
        seg = np.array([[a, n]])
        got, _ = A.segment_reductions({"blocks": [("p", 0, False)], "sid": np.array([case["phone"][0][k] * 3] * 3)}, seg, V[0, k:k + 1])
        assert got[0, 1] == lo and got[0, 0] < 0


# ------------------------------------------------------------------ Aligner.score(segmental=True)
@pytest.fixture(scope="module")
def small_corpus(dev):
    lex, utts = C.corpus(77, 20)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    spk = [b % 2 for b in range(len(xs))]
    return lex, ids, graphs, xs, [len(x) for x in xs], padded(xs, NAN, np.float64, dev), spk


@pytest.mark.parametrize("name,kw", [("single", {}), ("mixtures", {"mixtures": 3, "mix_iters": 2}),
                                     ("triphones", {"triphones": 40, "tri_iters": 2, "tri_min_occ": 10}), ("transitions", {"transitions": 1}),
                                     ("lda-fmllr", {"lda": 12, "splice": 1, "lda_iters": 2, "fmllr": 1, "fmllr_rounds": 1, "fmllr_iters": 1,
                                                    "fmllr_min_frames": 50})])
def test_aligner_segmental_scores(dev, small_corpus, name, kw):
    """a real decode: V[k, p] is the forced path's own score plus its arcs, gop <= gop_seg <= 0 without transitions, and every
    output is the oracle's on the same features and the same path"""
    lex, ids, graphs, xs, lens, feats, spk = small_corpus
    S, P_ = C.STATES, len(ids)
    n_classes = P_ * S
    al = A.Aligner(n_classes, 2 * C.N_MEL, S, dev, phone_ids=ids if "triphones" in kw else None, **kw)
    speakers = spk if al.fmllr else None
    al.fit([(feats, lens, graphs)], 3, [speakers] if al.fmllr else None)
    frames, plain = al.score(feats, lens, graphs, speakers)
    frames2, scores = al.score(feats, lens, graphs, speakers, segmental=True)
    assert all(np.array_equal(a, b) for a, b in zip(frames, frames2))
    for a, b in zip(plain, scores):                                        # nothing else changes, nothing new without the switch
        assert set(b) - set(a) == {"seg", "V", "gop_seg"}
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)

    host = lambda t: t.cpu().numpy()                                       # noqa: E731
    tables = (host(al.gw), host(al.gmu), host(al.gvar)) if al.mixtures > 1 else SR.as_mixture(host(al.mu), host(al.var))
    x, _, G, bp, end, _ = al._decode(feats, lens, graphs, speakers)       # the features the decoding model sees, and its path
    state = host(A.path(bp, lens, G, end)[0])
    x = host(x)
    arc = np.stack([np.log(al.loop), np.log(1.0 - al.loop)], 1) if al.transitions else np.zeros((al.n_classes, 2))
    tree = al.tree if al.triphones else None
    blocks = 0
    for b, (g, n) in enumerate(zip(graphs, lens)):
        gp = al._leaf_graph(g) if al.triphones else g
        F = SR.class_scores(x[b, :n], *tables)
        want = GR.utterance(F, gp, g, state[b, :n], GR.candidates(g, ids, S, tree), arc, S)
        got = scores[b]
        assert np.array_equal(want["seg"][:, 1], frames[b]) and got["V"].shape == (len(g["blocks"]), P_)
        live = frames[b] > 0
        assert np.array_equal(np.isnan(got["V"]).all(axis=1), ~live) and not np.isnan(got["V"][live]).any()
        fin = np.isfinite(want["V"])
        assert np.array_equal(np.isfinite(got["V"]), fin)
        close_to(got["V"][fin], want["V"][fin], want["mag"][fin])
        assert np.array_equal(np.isnan(got["seg"]), np.isnan(want["blocks"])) and np.array_equal(np.isnan(got["seg"][:, 0]), ~live)
        for k in np.nonzero(live)[0]:
            p, nk = int(g["sid"][k * S]) // S, int(frames[b][k])
            scale = want["mag"][k, p]
            assert abs(got["V"][k, p] - want["forced"][k]) <= RTOL * scale                     # the own sum plus arcs
            gop_seg, rival, margin = got["seg"][k]
            assert gop_seg <= 0.0 and gop_seg == min(margin, 0.0) and rival != p
            if not al.transitions:
                assert got["blocks"][k, 1] <= gop_seg + RTOL * scale / nk                      # gop <= gop_seg
            if want["gap"][k] > GK.MARGIN * abs(want["V"][k, int(want["blocks"][k, 1])]):
                assert rival == want["blocks"][k, 1]
                assert abs(margin - want["blocks"][k, 2]) <= 2 * RTOL * scale / nk
                blocks += 1
        assert abs(got["gop_seg"] - want["gop_seg"]) <= 2 * RTOL * np.nanmax(want["mag"]) and got["gop_seg"] <= 0.0
    assert blocks > 100
    if al.triphones:
        assert al.tree["n_leaves"] > n_classes                             # the tree did split


def test_bad_arguments_raise_before_any_launch(dev):
    case = GK.seg_case(1)
    S, P_ = case["S"], case["P"]
    lens = [len(f) for f in case["fs"]]
    f = padded(case["fs"], NAN, np.float64, dev)
    Kmax = 2
    seg = torch.tensor([[[0, 5], [5, 4]]] * 3, dtype=torch.int32, device=dev)
    cand = torch.arange(P_ * S, dtype=torch.int32, device=dev).reshape(1, 1, P_, S).repeat(3, Kmax, 1, 1)
    tw, tm, tv, ta = up(dev, case["w"], case["mu"], case["var"], case["arc"])
    C_, M, D = case["mu"].shape
    out = torch.full((3, Kmax, P_), GUARD, dtype=torch.float64, device=dev)
    with pytest.raises((RuntimeError, ValueError), match="no CPU fallback"):
        A.segment_scores(f.cpu(), lens, seg, cand, tw, tm, tv, ta, out=out)
    with pytest.raises((RuntimeError, ValueError), match="no CPU fallback"):
        A.segment_scores(f, lens, seg, cand.cpu(), tw, tm, tv, ta, out=out)
    with pytest.raises(ValueError, match="candidate phones"):             # P > 256
        A.segment_scores(f, lens, seg, torch.zeros(3, Kmax, 257, 1, dtype=torch.int32, device=dev), tw, tm, tv, ta)
    with pytest.raises(ValueError, match="candidate phones"):             # S = 4
        A.segment_scores(f, lens, seg, torch.zeros(3, Kmax, 4, 4, dtype=torch.int32, device=dev), tw, tm, tv, ta)
    high = cand.clone()
    high[1, 1, 3, 0] = C_
    with pytest.raises(ValueError, match="cand holds class"):
        A.segment_scores(f, lens, seg, high, tw, tm, tv, ta, out=out)
    with pytest.raises(ValueError):
        A.segment_scores(f, lens, seg[:, :1], cand, tw, tm, tv, ta, out=out)           # seg and cand of different blocks
    with pytest.raises(ValueError):
        A.segment_scores(f, lens, seg, cand, tw, tm, tv, ta[:-1], out=out)             # arcs of another table
    with pytest.raises(ValueError):
        A.segment_scores(f, lens, seg, cand, tw, tm, tv, ta, out=out[:, :, :P_ - 1])   # V too narrow
    # the ABI itself refuses before any launch: the output keeps its sentinel
    ws = torch.empty(C_ * M * (D + 1), dtype=torch.float64, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)

    def call(M=M, D=D, C_=C_, P_=P_, S=S, ldf_t=f.stride(1), lds=seg.stride(0), ldc_k=cand.stride(1), ldv_k=out.stride(1), n_ws=ws.numel(),
             B=3, arc=ta.data_ptr()):
        _lib.call("fs2_align_segment_scores", f.data_ptr(), f.stride(0), ldf_t, lens_d.data_ptr(), seg.data_ptr(), lds, cand.data_ptr(),
                  cand.stride(0), ldc_k, tw.data_ptr(), tm.data_ptr(), tv.data_ptr(), C_, M, D, arc, ws.data_ptr(), n_ws, out.data_ptr(),
                  out.stride(0), ldv_k, B, f.shape[1], Kmax, P_, S, None)
    for kw in ({"M": 0}, {"M": A.max_mixtures() + 1}, {"D": 0}, {"C_": 0}, {"P_": 0}, {"P_": A.max_seg_phones() + 1}, {"S": 0}, {"S": 4},
               {"ldf_t": D - 1}, {"lds": 2 * Kmax - 1}, {"ldc_k": P_ * S - 1}, {"ldv_k": P_ - 1}, {"n_ws": ws.numel() - 1}, {"B": 65536},
               {"C_": 1 << 28}, {"arc": None}):
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()
    assert (out == GUARD).all()
    lib = _lib.load()
    assert lib.fs2_align_segment_scores_ws(C_, M, D) == ws.numel() == lib.fs2_align_frame_scores_ws(C_, M, D)
    assert lib.fs2_align_segment_scores_ws(C_, 9, D) == 0 and A.max_seg_phones() == 256
    call()                                                                 # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------ substituted words
def margin_means(blocks, frames, sub, rest):
    mean = lambda ks: sum(blocks[k, 2] * frames[k] for k in ks if frames[k] > 0) / sum(frames[k] for k in ks if frames[k] > 0)  # noqa: E731
    return mean(sub), mean(rest)


def test_substituted_words_on_the_gpu(dev):
    """The 8 cases of `align_score_cases.substitution()`.  The reference alone (tests/test_align_seg_cpu.py) gives, per case, the
    frame-weighted mean `margin` of the substituted word's phones against that of the untouched words': -8.79 / 9.87, -9.98 / 9.13,
    -9.34 / 8.27, -11.35 / 8.68, -9.39 / 8.64, -6.25 / 9.33, -5.62 / 10.07, -8.55 / 5.17.  The substituted word's mean is negative and
    below the others' in all 8, so that ordering is asserted on the GPU, beside agreement with the reference's values."""
    mu, var, n_classes, cases = K.substitution()
    S = C.STATES
    ids = A.phone_table({"w": C.PHONES})
    al = A.Aligner(n_classes, mu.shape[1], S, dev)
    al._set(mu, var)
    xs, lens = [c[0] for c in cases], [len(c[0]) for c in cases]
    frames, scores = al.score(padded(xs, NAN, np.float64, dev), lens, [c[2] for c in cases], segmental=True)
    tables, phone = SR.as_mixture(mu, var), SR.class_phone_mono(n_classes, S)
    arc = np.zeros((n_classes, 2))
    for i, ((x, _, gs, sub, rest), fr, sc) in enumerate(zip(cases, frames, scores)):
        want_frames, _, (state, _, _, _, _) = SR.score(x, gs, *tables, phone, SR.plain_decode)
        assert np.array_equal(fr, want_frames)
        want = GR.utterance(SR.class_scores(x, *tables), gs, gs, state, GR.candidates(gs, ids, S), arc, S)
        ref_sub, ref_rest = margin_means(want["blocks"], fr, sub, rest)
        got_sub, got_rest = margin_means(sc["seg"], fr, sub, rest)
        print("case", i, "margin of the substituted word", got_sub, "of the others", got_rest, "reference", ref_sub, ref_rest)
        scale = 2 * np.nanmax(want["mag"]) / min(n for n in fr if n > 0)   # a margin is the difference of two V over n frames
        assert abs(got_sub - ref_sub) <= RTOL * scale and abs(got_rest - ref_rest) <= RTOL * scale
        assert ref_sub < 0.0 and ref_sub < ref_rest                        # what the reference alone satisfies in all 8 cases
        assert got_sub < 0.0 and got_sub < got_rest


# ------------------------------------------------------------------ build
def test_build_writes_segmental_scores_and_changes_nothing_else(dev, tmp_path):
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 5, 6)
    cfg = config(root, lexicon_path)
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    grids = lambda: {name: open(tg(name), "rb").read() for name in truth}                        # noqa: E731
    paths = [os.path.join(root, n) for n in ("omitted.jsonl", "zero.jsonl", "seg.jsonl")]
    A.build(cfg, device=dev, iters=4, num_workers=2, scores=paths[0])
    before = grids()
    A.build(cfg, device=dev, iters=4, num_workers=2, overwrite=True, scores=paths[1], seg_scores=0)
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read() and grids() == before    # seg_scores=0 is the parameter omitted
    done = A.build(cfg, device=dev, iters=4, num_workers=2, overwrite=True, scores=paths[2], seg_scores=1)
    assert done[0] == 6 and grids() == before                              # byte-identical TextGrids
    with pytest.raises(ValueError, match="needs `scores`"):
        A.build(cfg, device=dev, iters=4, num_workers=2, overwrite=True, seg_scores=1)
    plain = [json.loads(line) for line in open(paths[0])]
    rows = [json.loads(line) for line in open(paths[2])]
    labels = set(A.phone_table(A.read_lexicon(lexicon_path)))
    for r0, r in zip(plain, rows):
        assert {k: v for k, v in r.items() if k not in ("gop_seg", "phones")} == {k: v for k, v in r0.items() if k != "phones"}
        assert [p[:6] for p in r["phones"]] == r0["phones"] and all(len(p) == 9 for p in r["phones"])
        iv = P.read_textgrid(tg(r["basename"]))["phones"]
        assert [(p[1], p[2], p[0]) for p in r["phones"]] == [tuple(i) for i in iv]
        for label, _, _, _, gop, _, gop_seg, rival, margin in r["phones"]:
            assert rival in labels and rival != label and np.isfinite(margin) and gop_seg == min(margin, 0.0)
            assert gop <= gop_seg + 1e-6 * abs(r["loglik"]) * 100                             # arcs cost 0 here: gop <= gop_seg
        assert r["gop"] <= r["gop_seg"] + 1e-9 <= 1e-9
    text = A.scores_summary(paths[2])
    assert text.startswith(A.scores_summary(paths[0])) and "; mean gop_seg " in text and "intervals that lose to a rival: " in text
