"""GPU: the confidence kernels (csrc/fs2_align_score.hip: fs2_align_path, fs2_align_frame_scores), `Aligner.score` and
`build(..., scores=)` against the numpy oracle tests/align_score_ref.py, on the seeded inputs tests/test_align_score_cpu.py pins."""
import json
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib, align as A
from fastspeech2_amd import preprocess as P
from tests import align_corpus as C
from tests import align_lda_ref as LR
from tests import align_ref as R
from tests import align_score_cases as K
from tests import align_score_ref as SR
from tests import align_trans_ref as TR
from tests.test_align_cpu import config
from tests.test_align_gpu import RTOL, padded, ragged, rel_close  # noqa: F401  (ragged: the fixture of the scan tests' shapes)

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev_tables(dev, *tables):
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in tables]


def run_frame_scores(dev, fs, cs, w, mu, var):
    """the ragged batch with NaN padding, cls and the outputs strided views of wider buffers -> numpy (own, best, arg), lens"""
    lens = [len(f) for f in fs]
    B, Tmax = len(fs), max(lens)
    f = padded(fs, NAN, np.float64, dev)
    cls = padded([c[:, None] for c in cs], -5, np.int32, dev)[:, :, 0]
    wide = torch.full((B, Tmax + 5), -5, dtype=torch.int32, device=dev)
    wide[:, :Tmax] = cls
    own = torch.full((B, Tmax + 3), NAN, dtype=torch.float64, device=dev)[:, :Tmax]
    best = torch.full((B, Tmax + 1), NAN, dtype=torch.float64, device=dev)[:, :Tmax]
    arg = torch.full((B, Tmax + 2), -7, dtype=torch.int32, device=dev)[:, :Tmax]
    got = A.frame_scores(f, lens, wide[:, :Tmax], *dev_tables(dev, w, mu, var), out=(own, best, arg))
    assert got[0].data_ptr() == own.data_ptr()
    return own.cpu().numpy(), best.cpu().numpy(), arg.cpu().numpy(), lens


@pytest.mark.parametrize("case", range(len(K.SHAPES)), ids=[f"C{c}-D{d}-M{m}" for c, d, m in K.SHAPES])
def test_frame_scores_against_oracle(dev, case):
    fs, cs, w, mu, var, want = K.frame_case(case)
    own, best, arg, lens = run_frame_scores(dev, fs, cs, w, mu, var)
    compared = total = 0
    for b, (wo, wb, wa, margin) in enumerate(want):
        n = lens[b]
        rel_close(own[b, :n], wo)
        rel_close(best[b, :n], wb)
        sure = margin > K.MARGIN * np.abs(wb)
        assert np.array_equal(arg[b, :n][sure], wa[sure])
        compared, total = compared + int(sure.sum()), total + n
        assert (own[b, :n] <= best[b, :n]).all()                           # exact properties, bitwise
        same = arg[b, :n] == cs[b]
        assert np.array_equal(own[b, :n][same], best[b, :n][same]) and (own[b, :n][~same] <= best[b, :n][~same]).all()
        assert np.isnan(own[b, n:]).all() and np.isnan(best[b, n:]).all() and (arg[b, n:] == -7).all()   # never written
    print("frames", total, "arg compared on", compared)
    assert compared >= 0.99 * total
    again = run_frame_scores(dev, fs, cs, w, mu, var)
    for a, b in zip((own, best, arg), again[:3]):
        assert np.array_equal(a, b, equal_nan=True)                        # a second run is identical


@pytest.mark.parametrize("M", (1, 3))
def test_equal_rows_tie_and_the_lower_class_wins(dev, M):
    """copies of one class row at the lower and the upper end of different class tiles, at both ends of a lane's rows and in the
    last, partial tile: the frames drawn around that row score all copies alike, bit for bit, and the lowest index is returned"""
    n_classes, D = 3 * K.CLASS_TILE + 8, 24
    rng = np.random.RandomState(11)
    for copies in ((K.CLASS_TILE - 1, K.CLASS_TILE, 3 * K.CLASS_TILE - 1), (0, 2 * K.CLASS_TILE - 1, n_classes - 1), (15, 16, K.CLASS_TILE + 2),
                   (K.CLASS_TILE, K.CLASS_TILE + 17, 3 * K.CLASS_TILE + 7)):
        w, mu, var, _ = K.tables(rng, n_classes, D, M)
        for c in copies[1:]:
            w[c], mu[c], var[c] = w[copies[0]], mu[copies[0]], var[copies[0]]
        fs = [mu[copies[0], 0] + 0.1 * rng.randn(T, D) for T in (5, K.FRAME_TILE + 1)]
        cs = [np.full(len(f), c, np.int32) for f, c in zip(fs, copies[1:])]
        own, best, arg, lens = run_frame_scores(dev, fs, cs, w, mu, var)
        for b, n in enumerate(lens):
            assert (arg[b, :n] == copies[0]).all(), (copies, arg[b, :n])
            assert np.array_equal(own[b, :n], best[b, :n])                 # the copy scores what the original scores


def test_classes_outside_the_table_and_bad_arguments(dev):
    fs, cs, w, mu, var, want = K.frame_case(1)
    own, best, arg, lens = run_frame_scores(dev, fs, cs, w, mu, var)
    bad = [c.copy() for c in cs]
    for c in bad:
        c[::2] = -1
        c[1::4] = mu.shape[0]
    own2, best2, arg2, _ = run_frame_scores(dev, fs, bad, w, mu, var)
    assert np.array_equal(best, best2, equal_nan=True) and np.array_equal(arg, arg2)
    for b, n in enumerate(lens):
        out = (bad[b] < 0) | (bad[b] >= mu.shape[0])
        assert np.isnan(own2[b, :n][out]).all() and np.array_equal(own2[b, :n][~out], own[b, :n][~out])

    f = padded(fs[:2], NAN, np.float64, dev)
    cls = torch.zeros(2, f.shape[1], dtype=torch.int32, device=dev)
    tw, tm, tv = dev_tables(dev, w, mu, var)
    with pytest.raises((RuntimeError, ValueError), match="no CPU fallback"):
        A.frame_scores(f.cpu(), lens[:2], cls, tw, tm, tv)
    with pytest.raises(ValueError):
        A.frame_scores(f, lens[:2], cls[:, :3], tw, tm, tv)                # cls shorter than the frames
    with pytest.raises(ValueError):
        A.frame_scores(f, lens[:2], cls, tw, tm[:, :, :5], tv)             # tables of another dimension
    with pytest.raises(ValueError, match="mixture components"):
        A.frame_scores(f, lens[:2], cls, *dev_tables(dev, np.ones((4, 9)), np.zeros((4, 9, f.shape[2])), np.ones((4, 9, f.shape[2]))))
    with pytest.raises(ValueError):
        A.frame_scores(f, lens[:2], cls, tw, tm, tv, out=(torch.zeros(2, 3, dtype=torch.float64, device=dev),) * 2 + (cls,))
    # the ABI itself refuses before any launch: the outputs keep their sentinel
    C_, M, D = mu.shape
    ws = torch.empty(C_ * M * (D + 1), dtype=torch.float64, device=dev)
    o = torch.full((2, f.shape[1]), 77.0, dtype=torch.float64, device=dev)
    lens_d = torch.tensor(lens[:2], dtype=torch.int32, device=dev)

    def call(M=M, D=D, C_=C_, ldf_t=f.stride(1), ldo=o.stride(0), n_ws=ws.numel(), B=2):
        _lib.call("fs2_align_frame_scores", f.data_ptr(), f.stride(0), ldf_t, lens_d.data_ptr(), cls.data_ptr(), cls.stride(0),
                  tw.data_ptr(), tm.data_ptr(), tv.data_ptr(), C_, M, D, ws.data_ptr(), n_ws, o.data_ptr(), ldo, o.data_ptr(), o.stride(0),
                  cls.data_ptr(), cls.stride(0), B, f.shape[1], None)
    for kw in ({"M": 0}, {"M": A.max_mixtures() + 1}, {"D": 0}, {"C_": 0}, {"ldf_t": D - 1}, {"ldo": f.shape[1] - 1}, {"n_ws": ws.numel() - 1},
               {"B": 65536}, {"C_": 1 << 28}):
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()
    assert (o == 77.0).all() and (cls == 0).all()
    assert _lib.load().fs2_align_frame_scores_ws(C_, M, D) == ws.numel() and _lib.load().fs2_align_frame_scores_ws(C_, 9, D) == 0


def test_path_against_oracle_and_backtrack(dev, ragged):  # noqa: F811
    """the shapes of the scan tests: corpus utterances, a single block, T = the mandatory states, J = 1024"""
    graphs, xs, lens, mu, var, Es, n_classes = ragged
    G = A.Graphs(graphs, dev)
    E = padded(Es, NAN, np.float64, dev)
    bp, end, _ = A.viterbi(E, lens, G)
    frames = A.backtrack(bp, lens, G, end).cpu().numpy()
    state, cls = (v.cpu().numpy() for v in A.path(bp, lens, G, end))
    bph, endh = bp.cpu().numpy(), end.cpu().numpy()
    for b, g in enumerate(graphs):
        n = lens[b]
        want = SR.path_states(bph[b, :n, :G.jl[b]], endh[b], g)
        assert np.array_equal(state[b, :n], want) and (want >= 0).all(), b
        assert np.array_equal(cls[b, :n], g["sid"][want])
        assert np.array_equal(SR.run_lengths(g, state[b, :n]), frames[b, :len(g["blocks"])])
        assert (state[b, n:] == -1).all() and (cls[b, n:] == -1).all()
    # own is the emission of the path's state: the scoring kernel against the emission kernel
    x = padded(xs, NAN, np.float64, dev)
    tm, tv = dev_tables(dev, mu, var)
    own, best, arg = A.frame_scores(x, lens, torch.from_numpy(cls).to(dev), torch.ones(n_classes, 1, dtype=torch.float64, device=dev),
                                    tm.unsqueeze(1), tv.unsqueeze(1))
    Eg = A.emit(x, lens, G, tm, tv).cpu().numpy()
    own = own.cpu().numpy()
    for b, n in enumerate(lens):
        rel_close(own[b, :n], Eg[b, np.arange(n), state[b, :n]])

    # a corrupted chain: a skip where the graph has none, and an end state outside the graph
    b = 0
    t = max(t for t in range(1, lens[b] // 2 + 1) if graphs[b]["skip"][state[b, t]] < 0)
    bad = bp.clone()
    bad[b, t, int(state[b, t])] = 2
    bad_end = end.clone()
    bad_end[1] = G.jl[1]
    s2, c2 = (v.cpu().numpy() for v in A.path(bad, lens, G, bad_end))
    assert np.array_equal(s2[b, t:lens[b]], state[b, t:lens[b]]) and (s2[b, :t] == -1).all() and (c2[b, :t] == -1).all()
    assert (s2[1] == -1).all() and (c2[1] == -1).all()
    assert np.array_equal(s2[2:], state[2:]) and np.array_equal(c2[2:], cls[2:])


def test_own_against_the_mixture_emissions(dev):
    fs, cs, w, mu, var, _ = K.frame_case(2)                                # 67 classes, 8 components, ragged
    states = 4
    graphs = [{"sid": np.arange(k * states, (k + 1) * states, dtype=np.int32), "skip": np.full(states, -1, np.int32),
               "block": np.zeros(states, np.int32), "alt": (-1, -1), "blocks": [("X", 0, False)], "mandatory": states} for k in range(len(fs))]
    lens = [len(f) for f in fs]
    G = A.Graphs(graphs, dev)
    x = padded(fs, NAN, np.float64, dev)
    tw, tm, tv = dev_tables(dev, w, mu, var)
    E = A.emit_gmm(x, lens, G, tw, tm, tv).cpu().numpy()
    for s in range(states):
        cls = np.full((len(fs), max(lens)), -1, np.int32)
        for b, n in enumerate(lens):
            cls[b, :n] = graphs[b]["sid"][s]
        own = A.frame_scores(x, lens, torch.from_numpy(cls).to(dev), tw, tm, tv)[0].cpu().numpy()
        for b, n in enumerate(lens):
            rel_close(own[b, :n], E[b, :n, s])


# ------------------------------------------------------------------ Aligner.score
@pytest.fixture(scope="module")
def small_corpus(dev):
    lex, utts = C.corpus(77, 20)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    lens = [len(x) for x in xs]
    return lex, ids, graphs, xs, lens, padded(xs, NAN, np.float64, dev)


def check_scores(got, want, frames, want_frames):
    assert np.array_equal(frames, want_frames)
    for key in ("frames", "viterbi", "loglik", "gop", "match"):
        rel_close(got[key], want[key])
    assert np.array_equal(np.isnan(got["blocks"]), np.isnan(want["blocks"]))
    assert np.array_equal(np.isnan(got["blocks"][:, 0]), frames == 0)     # NaN for a block of 0 frames, and only there
    ok = frames > 0
    rel_close(got["blocks"][ok], want["blocks"][ok])


@pytest.mark.parametrize("name,kw", [("single", {}), ("mixtures", {"mixtures": 3, "mix_iters": 2}), ("lda", {"lda": 12, "splice": 1, "lda_iters": 2}),
                                     ("triphones", {"triphones": 40, "tri_iters": 2, "tri_min_occ": 10}), ("transitions", {"transitions": 1})])
def test_aligner_score_against_oracle(dev, small_corpus, name, kw):
    """`score` on a trained Aligner against the oracle fed the Aligner's own tables: the same frames as `align`, the block and
    utterance numbers to RTOL."""
    lex, ids, graphs, xs, lens, feats = small_corpus
    n_classes = len(ids) * C.STATES
    al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev, phone_ids=ids if "triphones" in kw else None, **kw)
    al.fit([(feats, lens, graphs)], 3)
    frames, scores = al.score(feats, lens, graphs)
    again = al.align(feats, lens, graphs)
    assert all(np.array_equal(a, b) for a, b in zip(frames, again))       # exactly `align`'s frames

    host = lambda t: t.cpu().numpy()                                       # noqa: E731
    if al.mixtures > 1:
        tables = (host(al.gw), host(al.gmu), host(al.gvar))
    else:
        tables = SR.as_mixture(host(al.mu), host(al.var))
    assert tables[1].shape[0] == al.n_classes
    fs = [LR.project(LR.splice(x, C.N_MEL, al.splice), host(al.P), host(al.o)) for x in xs] if al.lda else xs
    gs = [al._leaf_graph(g) for g in graphs] if al.triphones else graphs
    if al.triphones:
        t = al.tree
        assert t["n_leaves"] > n_classes                                   # the tree did split
        phone = SR.class_phone_tree(t["question"], t["yes"], t["no"], t["leaf"], n_classes, C.STATES)
    else:
        phone = SR.class_phone_mono(n_classes, C.STATES)
    assert np.array_equal(al.class_phone(), phone)
    decode = (lambda E, g: TR.viterbi(E, g, *TR.arc_costs(g, al.loop, al.opt))) if al.transitions else SR.plain_decode
    for b, (f, g) in enumerate(zip(fs, gs)):
        want_frames, want, _ = SR.score(f, g, *tables, phone, decode)
        check_scores(scores[b], want, frames[b], want_frames)
        assert scores[b]["gop"] <= 0.0


def test_substituted_words_on_the_gpu(dev):
    mu, var, n_classes, cases = K.substitution()
    al = A.Aligner(n_classes, mu.shape[1], C.STATES, dev)
    al._set(mu, var)
    phone = SR.class_phone_mono(n_classes, C.STATES)
    xs, lens = [c[0] for c in cases], [len(c[0]) for c in cases]
    frames, scores = al.score(padded(xs, NAN, np.float64, dev), lens, [c[2] for c in cases])
    for (x, _, gs, sub, rest), fr, sc in zip(cases, frames, scores):
        want_frames, want, _ = SR.score(x, gs, *SR.as_mixture(mu, var), phone, SR.plain_decode)
        check_scores(sc, want, fr, want_frames)
        assert SR.block_mean(sc, fr, sub) < SR.block_mean(sc, fr, rest)


def test_build_writes_scores_beside_unchanged_textgrids(dev, tmp_path):
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 5, 6)
    cfg = config(root, lexicon_path)
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    plain = A.build(cfg, device=dev, iters=4, num_workers=2)
    before = {name: open(tg(name), "rb").read() for name in truth}
    path = os.path.join(root, "scores.jsonl")
    scored = A.build(cfg, device=dev, iters=4, num_workers=2, overwrite=True, scores=path)
    assert len(scored) == 3 and scored[0] == plain[0] == 6 and scored[2] == plain[2]
    assert before == {name: open(tg(name), "rb").read() for name in truth}                   # byte-identical TextGrids
    rows = [json.loads(line) for line in open(path)]
    assert sorted(r["basename"] for r in rows) == sorted(truth) and all(r["speaker"] == "spk" for r in rows)
    for r in rows:
        iv = P.read_textgrid(tg(r["basename"]))["phones"]
        assert [(p[1], p[2], p[0]) for p in r["phones"]] == [tuple(i) for i in iv]             # the same intervals, the same boundaries
        vals = np.array([p[3:] for p in r["phones"]], np.float64)
        assert vals.shape == (len(iv), 3) and np.isfinite(vals).all() and (vals[:, 1] <= 0).all()
        assert r["gop"] <= 0 and 0 <= r["match"] <= 1 and r["frames"] == int(round(iv[-1][1] * C.SR / C.HOP))
    text = A.scores_summary(path)
    assert text.startswith("scores: 6 utterances, mean gop ")
