"""GPU: the phone-loop recogniser (fastspeech2_amd.recognize, csrc/fs2_align_loop.hip) against the numpy oracle
tests/align_loop_ref.py, bit for bit, on ragged batches whose padding is NaN; model files (`Aligner.save` / `load`,
`build(save_model=...)` / `build(model=...)`); training, decoding and PER on the synthetic corpus of tests/align_corpus.py against
the bars of tests/golden/align_loop_bars.json; recognize.py end to end on a corpus of tone sequences."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import _lib, align as A
from fastspeech2_amd import recognize as RC
from tests import align_corpus as C
from tests import align_loop_ref as LR
from tests.golden import make_align_loop_bars as MB
from tests.test_align_cpu import config
from tests.test_align_gpu import padded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, NINF = float("nan"), -np.inf
TMAX = 64


# ------------------------------------------------------------------------------------------------ kernel against oracle
def draw_costs(rng, P, S, kind="random"):
    C_ = P * S
    if kind == "zero":
        return [np.zeros(C_), np.zeros(C_), np.zeros((P, P)), np.zeros(P), np.zeros(P)]
    if kind == "integer":
        return [rng.randint(-2, 1, n).astype(np.float64) for n in (C_, C_, (P, P), P, P)]
    return [2.0 * rng.randn(*n) for n in ((C_,), (C_,), (P, P), (P,), (P,))]


def run_case(dev, P, S, costs, Es, wide):
    """Viterbi and backtrack on the batch Es [(T_b, C)] against the oracle; `wide`: every buffer is a strided view of a larger one.
    -> the device outputs, for the determinism test."""
    C_, B, lens = P * S, len(Es), [len(e) for e in Es]
    pt, pc, pl = (2, 5, 3) if wide else (0, 0, 0)
    Ebuf = torch.full((B, TMAX + pt, C_ + pc), NAN, dtype=torch.float64, device=dev)
    for b, e in enumerate(Es):
        Ebuf[b, :lens[b], :C_] = torch.from_numpy(e)
    bpbuf = torch.full((B, TMAX + pt, C_ + pc), 77, dtype=torch.uint8, device=dev)
    linkbuf = torch.full((P, P + pl), NAN, dtype=torch.float64, device=dev)
    linkbuf[:, :P] = torch.from_numpy(costs[2])
    segbuf = torch.full((2, B, TMAX + pt), -7, dtype=torch.int32, device=dev)
    up = lambda v: torch.from_numpy(v).to(dev)                             # noqa: E731
    bp, end, score = RC.loop_viterbi(Ebuf[:, :TMAX], lens, up(costs[0]), up(costs[1]), linkbuf[:, :P], up(costs[3]), up(costs[4]), P, S,
                                     out=bpbuf[:, :TMAX])
    phone, start, n_seg = RC.loop_backtrack(bp, lens, end, P, S, out=(segbuf[0], segbuf[1]))
    assert bp.data_ptr() == bpbuf.data_ptr() and phone.data_ptr() == segbuf.data_ptr()
    bph, endh, scoreh, segh, nh = bpbuf.cpu().numpy(), end.cpu().numpy(), score.cpu().numpy(), segbuf.cpu().numpy(), n_seg.cpu().numpy()
    for b, e in enumerate(Es):
        wbp, wend, wscore = LR.loop_viterbi(e, *costs, P, S)
        wsegs = LR.loop_backtrack(wbp, wend, P, S)
        T = lens[b]
        assert np.array_equal(bph[b, :T, :C_], wbp), (P, S, b)
        assert (bph[b, T:] == 77).all() and (bph[b, :, C_:] == 77).all(), (P, S, b)          # padding is never written
        assert endh[b] == wend and (scoreh[b] == wscore or (np.isnan(scoreh[b]) and np.isnan(wscore))), (P, S, b, scoreh[b], wscore)
        assert nh[b] == len(wsegs) <= T, (P, S, b)
        assert [(int(p), int(a)) for p, a in zip(segh[0, b, :nh[b]], segh[1, b, :nh[b]])] == wsegs, (P, S, b)
        assert (segh[:, b, nh[b]:] == -7).all(), (P, S, b)
        if T < S:
            assert wend == -1 and wscore == NINF and wsegs == []
    return bpbuf, end, score, segbuf, n_seg


def batch_of(rng, P, S, integer=False):
    lens = [0, 1, S - 1, S, 2, 37, TMAX]
    if integer:
        return [rng.randint(-2, 1, (T, P * S)).astype(np.float64) for T in lens]
    return [3.0 * rng.randn(T, P * S) for T in lens]


SHAPES = [(1, 1), (3, 1), (5, 2), (14, 2), (85, 3), (86, 3), (253, 1), (253, 3)]


@pytest.mark.parametrize("wide", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("P,S", SHAPES)
def test_kernel_against_oracle(dev, P, S, wide):
    """(85, 3) is the last 256-lane case and the largest link table that is staged in LDS (57.8 KB beside 4.1 KB of rows), (86, 3) the
    first 512-lane case and the first that reads link from global memory, (253, .) the limit of P, (253, 3) the 1024-lane case.
    `padded` gives every buffer a wider stride than its extent (link: ldl = P + 3, on both paths)."""
    rng = np.random.RandomState(1000 * P + S)
    run_case(dev, P, S, draw_costs(rng, P, S), batch_of(rng, P, S), wide)


@pytest.mark.parametrize("P,S", [(5, 2), (14, 1), (86, 3)])
def test_forbidden_arcs_and_ties(dev, P, S):
    rng = np.random.RandomState(P + S)
    costs = draw_costs(rng, P, S)
    costs[3][0] = NINF                                                     # a forbidden start phone
    costs[2][1 % P, 2 % P] = NINF                                          # a forbidden bigram
    costs[2][:, P - 1] = NINF                                              # a phone that can only start an utterance
    costs[4][P // 2] = NINF                                                # a forbidden last phone
    run_case(dev, P, S, costs, batch_of(rng, P, S), True)
    run_case(dev, P, S, draw_costs(rng, P, S, "integer"), batch_of(rng, P, S, integer=True), False)   # exact ties everywhere
    Es = [np.zeros((T, P * S)) for T in (0, 1, S - 1, S, 2, 37, TMAX)]
    run_case(dev, P, S, draw_costs(rng, P, S, "zero"), Es, True)           # all ties: the rules alone decide
    none = draw_costs(rng, P, S)
    none[3][:] = NINF                                                      # nothing may start: no path at any length
    out = run_case(dev, P, S, none, batch_of(rng, P, S), False)
    assert (out[1].cpu().numpy() == -1).all() and (out[4].cpu().numpy() == 0).all()


def test_two_runs_are_bitwise_equal(dev):
    for P, S in ((14, 2), (253, 3)):
        rng = np.random.RandomState(3)
        costs, Es = draw_costs(rng, P, S, "integer"), batch_of(rng, P, S, integer=True)
        a, b = run_case(dev, P, S, costs, Es, True), run_case(dev, P, S, costs, Es, True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refusals_before_launch(dev):
    """P above 253, S above 3 and P S above `max_states()` raise; with P and S inside their limits P S is at most 759, so the last
    check can only be reached with a P that the first one refuses: the ABI is called with P = 400."""
    assert RC.max_loop_phones() == 253
    E = torch.zeros(1, 4, 1100, dtype=torch.float64, device=dev)
    z = lambda *n: torch.zeros(*n, dtype=torch.float64, device=dev)       # noqa: E731
    for P, S in ((254, 1), (3, 4), (0, 1), (3, 0)):
        with pytest.raises(ValueError, match="supported"):
            RC.loop_viterbi(E, [4], z(P * S), z(P * S), z(P, P), z(P), z(P), P, S)
        with pytest.raises(ValueError, match="supported"):
            RC.loop_backtrack(torch.zeros(1, 4, 1100, dtype=torch.uint8, device=dev), [4], torch.zeros(1, dtype=torch.int32, device=dev), P, S)
    bp = torch.zeros(1, 4, 1200, dtype=torch.uint8, device=dev)
    i32 = torch.zeros(8, dtype=torch.int32, device=dev)
    big = z(400, 400)
    wide = z(1, 4, 1200)
    for P, S in ((254, 1), (3, 4), (400, 3)):
        with pytest.raises(ValueError):
            _lib.call("fs2_align_loop_viterbi", wide.data_ptr(), wide.stride(0), wide.stride(1), i32.data_ptr(), big.data_ptr(), big.data_ptr(),
                      big.data_ptr(), 400, big.data_ptr(), big.data_ptr(), bp.data_ptr(), bp.stride(0), bp.stride(1), i32.data_ptr(),
                      big.data_ptr(), 1, 4, P, S, None)
        with pytest.raises(ValueError):
            _lib.call("fs2_align_loop_backtrack", bp.data_ptr(), bp.stride(0), bp.stride(1), i32.data_ptr(), i32.data_ptr(), i32.data_ptr(),
                      i32.data_ptr(), 8, i32.data_ptr(), 1, 4, P, S, None)
    with pytest.raises(ValueError):                                        # a bad stride, a null pointer
        _lib.call("fs2_align_loop_viterbi", wide.data_ptr(), wide.stride(0), 5, i32.data_ptr(), big.data_ptr(), big.data_ptr(), big.data_ptr(),
                  400, big.data_ptr(), big.data_ptr(), bp.data_ptr(), bp.stride(0), bp.stride(1), i32.data_ptr(), big.data_ptr(), 1, 4, 3, 2, None)
    with pytest.raises(ValueError):
        _lib.call("fs2_align_loop_viterbi", wide.data_ptr(), wide.stride(0), wide.stride(1), i32.data_ptr(), big.data_ptr(), big.data_ptr(),
                  None, 400, big.data_ptr(), big.data_ptr(), bp.data_ptr(), bp.stride(0), bp.stride(1), i32.data_ptr(), big.data_ptr(), 1, 4, 3,
                  2, None)
    with pytest.raises(ValueError):
        RC.loop_viterbi(E.cpu(), [4], z(6), z(6), z(3, 3), z(3), z(3), 3, 2)


# ------------------------------------------------------------------------------------------------ model files
SEED, N_MODEL = 1234, 30
FRONT = dict(lda=8, splice=1, lda_iters=1, fmllr=1, fmllr_rounds=1, fmllr_iters=1, fmllr_sweeps=5, fmllr_min_frames=100)
MODELS = {"defaults": {}, "mixtures_lda_transitions": dict(mixtures=2, mix_iters=2, lda=20, lda_iters=2, transitions=1),
          "triphones_fmllr": dict(triphones=40, tri_iters=1, tri_min_occ=10, **FRONT)}
FEATURES = {"sampling_rate": 22050, "filter_length": 1024, "hop_length": 256, "win_length": 1024, "n_mel": 80, "fmin": 0, "fmax": 8000}


def corpus_batches(dev, utts, graphs, budget=12 << 20, **kw):
    frames = [u["mel"].shape[1] for u in utts]
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, budget, **kw):
        mel = padded([utts[i]["mel"].T for i in batch], 0.0, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        batches.append((A.features(mel, lens), lens, [graphs[i] for i in batch], batch))
    return batches


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope="module")
def trained(dev):
    """name -> (Aligner, batches, speaker lists, phone names) for the three models of MODELS"""
    lex, utts = C.corpus(SEED, N_MODEL)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    batches = corpus_batches(dev, utts, graphs, splice_dim=240, fmllr_dim=8, mixtures=2, transitions=1)
    speakers = [[i % 2 for i in b[3]] for b in batches]
    out = {}
    for name, kw in MODELS.items():
        al = A.Aligner(len(ids) * C.STATES, 2 * C.N_MEL, C.STATES, dev, phone_ids=ids if kw.get("triphones") else None, **kw)
        al.fit([b[:3] for b in batches], 4, speakers if kw.get("fmllr") else None)
        out[name] = (al, batches, speakers, sorted(ids, key=ids.get))
    return out


@pytest.mark.parametrize("name", list(MODELS))
def test_save_and_load_give_the_same_bits(trained, tmp_path, name):
    al, batches, speakers, names = trained[name]
    path = str(tmp_path / "model.npz")
    counts = np.arange((len(names) + 1) ** 2, dtype=np.float64).reshape(len(names) + 1, -1)
    al.save(path, names, FEATURES, ["a", "b"] if al.fmllr else None, counts)
    with np.load(path, allow_pickle=False) as f:                           # one npz without pickled objects
        assert int(f["version"]) == A.MODEL_VERSION and {"options", "features", "phones", "floor", "loop", "opt", "bigram"} <= set(f.files)
    back = A.Aligner.load(path, al.device)
    assert back.phone_names == names and back.feature_config == FEATURES and np.array_equal(back.bigram, counts)
    assert back.speaker_names == (["a", "b"] if al.fmllr else None) and back.options() == al.options() and back.n_classes == al.n_classes
    for (feats, lens, gs, _), sp in zip(batches, speakers):
        sp = sp if al.fmllr else None
        assert same(al.align(feats, lens, gs, sp), back.align(feats, lens, gs, sp))
        seg = name == "mixtures_lda_transitions"
        assert same(al.score(feats, lens, gs, sp, segmental=seg), back.score(feats, lens, gs, sp, segmental=seg))
    if al.fmllr:
        with pytest.raises(ValueError, match="speaker names"):
            al.save(path, names, FEATURES, ["a"])
    with pytest.raises(ValueError, match="phone names"):
        al.save(path, names[:-1], FEATURES, ["a", "b"])


def test_recognizer_refuses_context_dependent_and_adapted_models(trained):
    al, _, _, names = trained["triphones_fmllr"]
    with pytest.raises(ValueError, match="triphones"):
        RC.Recognizer(al, names, lm="none")
    plain, _, _, names = trained["defaults"]
    with pytest.raises(ValueError, match="bigram"):
        RC.Recognizer(plain, names)                                        # lm = "bigram" without counts
    with pytest.raises(ValueError, match="classes"):
        RC.Recognizer(plain, names[:-1], lm="none")


def textgrids(root):
    out = {}
    for d, _, files in os.walk(os.path.join(root, "pre", "TextGrid")):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


@pytest.fixture(scope="module")
def wav_model(dev, tmp_path_factory):
    """`build(save_model=...)` on eight utterances of tone sequences -> (root, config, model file, truth, the TextGrids' bytes)"""
    root = str(tmp_path_factory.mktemp("loop_wav"))
    lexicon_path, truth = C.wav_corpus(root, 99, 8)
    cfg = config(root, lexicon_path)
    model = os.path.join(root, "model.npz")
    written, skipped, history = A.build(cfg, device=dev, iters=6, save_model=model)
    assert written == 8 and not skipped and len(history) == 6
    return root, cfg, model, truth, textgrids(root)


def test_build_with_a_model_file_writes_the_same_textgrids(dev, wav_model):
    root, cfg, model, truth, before = wav_model
    assert len(before) == 8
    with pytest.raises(FileExistsError):
        A.build(cfg, device=dev, model=model)
    written, skipped, history = A.build(cfg, device=dev, model=model, overwrite=True)
    assert written == 8 and not skipped and history == []
    assert textgrids(root) == before
    al = A.Aligner.load(model, dev)
    assert al.feature_config == RC.feature_config(cfg) and al.bigram.shape == (len(al.phone_names) + 1,) * 2
    assert al.bigram[-1].sum() == 8 and al.bigram[:, -1].sum() == 8      # eight sequences start and end


def test_build_refuses_a_model_that_does_not_fit(dev, wav_model, tmp_path):
    root, cfg, model, _, before = wav_model
    with pytest.raises(ValueError, match="training options .*mixtures"):
        A.build(cfg, device=dev, model=model, overwrite=True, mixtures=2)
    other = json.loads(json.dumps(cfg))
    other["preprocessing"]["stft"]["hop_length"] = 128
    with pytest.raises(ValueError, match="hop_length 128"):
        A.build(other, device=dev, model=model, overwrite=True)
    lex2 = str(tmp_path / "lexicon.txt")
    with open(cfg["path"]["lexicon_path"]) as f, open(lex2, "w") as g:
        g.write(f.read() + "EXTRA\tAA ZH\n")
    other = json.loads(json.dumps(cfg))
    other["path"]["lexicon_path"] = lex2
    with pytest.raises(ValueError, match="ZH"):
        A.build(other, device=dev, model=model, overwrite=True)
    assert textgrids(root) == before                                       # a refusal comes before any work


def test_build_with_fmllr_refuses_an_unknown_speaker(dev, tmp_path):
    root = str(tmp_path)
    lexicon_path, _ = C.wav_corpus(root, 99, 6, speaker="anna")
    C.wav_corpus(root, 99, 6, speaker="bert")                              # the same seed: the same lexicon file
    cfg = config(root, lexicon_path)
    model = os.path.join(root, "sat.npz")
    written, _, history = A.build(cfg, device=dev, iters=4, save_model=model, **FRONT)
    assert written == 12 and len(history) == 4 + 1 + 1 + 2
    before = textgrids(root)
    assert A.build(cfg, device=dev, model=model, overwrite=True)[0] == 12 and textgrids(root) == before
    assert A.Aligner.load(model, dev).speaker_names == ["anna", "bert"]
    shutil.move(os.path.join(root, "raw", "bert"), os.path.join(root, "raw", "carl"))
    with pytest.raises(ValueError, match="carl"):
        A.build(cfg, device=dev, model=model, overwrite=True)
    with pytest.raises(ValueError, match="fmllr"):
        RC.Recognizer(A.Aligner.load(model, dev), A.Aligner.load(model, dev).phone_names, lm="none")


# ------------------------------------------------------------------------------------------------ end to end
def word_spans(utt, lex):
    """[(first frame, end frame, first index among the non-silent phones, end index)] per word, from the true segments"""
    spans, segs, t, k, i = [], utt["segments"], 0, 0, 0
    for word in utt["words"]:
        while segs[i][0] in MB.SILENT:
            t, i = t + segs[i][1], i + 1
        n = len(lex[word])
        assert [p for p, _ in segs[i:i + n]] == lex[word]
        d = sum(f for _, f in segs[i:i + n])
        spans.append((t, t + d, k, k + n))
        t, k, i = t + d, k + n, i + n
    return spans


@pytest.fixture(scope="module")
def end_to_end(dev):
    """The recipe of tests/golden/make_align_loop_bars.py on the GPU, first seed: (lexicon, utterances, phone ids, names, aligner,
    bigram counts)."""
    seed = MB.SEEDS[0]
    lex, utts = C.corpus(seed, MB.N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    batches = corpus_batches(dev, utts[:MB.N_TRAIN], graphs[:MB.N_TRAIN])
    al = A.Aligner(len(ids) * C.STATES, 2 * C.N_MEL, C.STATES, dev)
    al.fit([b[:3] for b in batches], MB.ITERS)
    seqs = []
    for feats, lens, gs, _ in batches:
        seqs += [MB.heard(g, fr, ids) for g, fr in zip(gs, al.align(feats, lens, gs))]
    return lex, utts, ids, sorted(ids, key=ids.get), al, RC.phone_bigram(seqs, len(ids), MB.SMOOTHING)[0]


def features_of(dev, mels):
    lens = [m.shape[1] for m in mels]
    mel = padded([m.T for m in mels], 0.0, np.float32, dev).transpose(1, 2).contiguous()
    return A.features(mel, lens), lens


@pytest.mark.parametrize("lm", ["none", "bigram"])
def test_per_on_the_synthetic_corpus(dev, end_to_end, lm):
    """The GPU hypotheses equal the oracle's from the same emissions and costs, and the PER against the true segments (silences
    dropped) stays under the recorded bar: the worst oracle PER over three seeds + 0.02 (recorded: none 0.0 / 0.0 / 0.0060, bigram
    0.0070 / 0.0124 / 0.0119).  On this corpus the bigram at scale 8 does not help: the classes are well separated and the loop
    without a language model is already nearly exact."""
    lex, utts, ids, names, al, counts = end_to_end
    with open(MB.PATH) as f:
        bars = json.load(f)
    assert bars["seeds"] == list(MB.SEEDS) and bars["margin"] == MB.MARGIN
    assert abs(bars["bar"][lm] - (max(v[lm] for v in bars["per"].values()) + MB.MARGIN)) <= 1e-15
    rec = RC.Recognizer(al, names, counts, lm=lm, lm_scale=MB.LM_SCALE, penalty=MB.PENALTY, smoothing=MB.SMOOTHING)
    test = utts[MB.N_TRAIN:]
    feats, lens = features_of(dev, [u["mel"] for u in test])
    segs, scores = rec.decode(feats, lens)
    E = rec.emissions(feats, lens)[0].cpu().numpy()
    for b, T in enumerate(lens):
        want, wscore = LR.decode(E[b, :T], rec.self_, rec.next_, rec.link, rec.init, rec.final_, rec.P, rec.S)
        assert segs[b] == want and scores[b] == wscore, b
        assert sum(n for _, _, n in segs[b]) == T
    per, _ = MB.score([[names[p] for p, _, _ in s] for s in segs], test)
    print("PER", lm, per, "bar", bars["bar"][lm], "oracle", bars["per"][str(MB.SEEDS[0])][lm])
    assert per <= bars["bar"][lm], (per, bars["bar"][lm])


def test_an_overwritten_word_shows_as_substitutions_in_its_span(dev, end_to_end):
    lex, utts, ids, names, al, counts = end_to_end
    rec = RC.Recognizer(al, names, counts, lm="bigram", lm_scale=MB.LM_SCALE)
    test = utts[MB.N_TRAIN:]
    def fits(u, w, other):
        """`other` has as many phones as word w of u, every one another phone, and does not run into u's neighbouring phones (a loop
        cannot tell one long phone from the same phone twice)"""
        ref = [p for p, _ in u["segments"] if p not in MB.SILENT]
        _, _, k0, k1 = word_spans(u, lex)[w]
        own, new = lex[u["words"][w]], lex[other]
        return (len(own) == len(new) and all(x != y for x, y in zip(own, new)) and (k0 == 0 or ref[k0 - 1] != new[0])
                and (k1 == len(ref) or ref[k1] != new[-1]))
    pick = None
    for u in test:                                                         # a word, and another of as many and other phones, said somewhere
        for w in range(len(u["words"])):
            for v in utts:
                for w2, other in enumerate(v["words"]):
                    if pick is None and fits(u, w, other):
                        pick = (u, w, v, w2)
    assert pick is not None
    u, w, v, w2 = pick
    a0, a1, k0, k1 = word_spans(u, lex)[w]
    b0, b1, _, _ = word_spans(v, lex)[w2]
    changed = np.concatenate([u["mel"][:, :a0], v["mel"][:, b0:b1], u["mel"][:, a1:]], axis=1)
    feats, lens = features_of(dev, [u["mel"], changed])
    segs, _ = rec.decode(feats, lens)
    (per0, per1), rows = zip(*[MB.score([[names[p] for p, _, _ in s]], [u]) for s in segs])
    subs = [[a for kind, a, _ in r[0][1] if kind == "sub"] for r in rows]
    print("PER", per0, "->", per1, "substitutions at", subs, "span", (k0, k1))
    new = set(subs[1]) - set(subs[0])
    assert new and new <= set(range(k0, k1)), (subs, k0, k1)
    assert per1 > per0


# ------------------------------------------------------------------------------------------------ command line
def test_command_line(dev, wav_model, tmp_path):
    root, cfg, model, truth, _ = wav_model
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    source, out = str(tmp_path / "val.txt"), str(tmp_path / "per.jsonl")
    with open(source, "w") as f:
        for name, segs in truth.items():
            f.write(f"{name}|spk|{{{' '.join(p for p, _ in segs)}}}|text\n")
        f.write("nowav|spk|{AA B}|text\n")
    cmd = [sys.executable, os.path.join(ROOT, "recognize.py"), model, "-p", os.path.join(root, "preprocess.yaml"), "--source", source,
           "--wav_dir", os.path.join(root, "raw", "spk"), "--out", out]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rows = [json.loads(ln) for ln in open(out)]
    assert [r["basename"] for r in rows] == list(truth)
    for r in rows:
        assert set(r) == {"basename", "n_ref", "hits", "sub", "del", "ins", "per", "score_per_frame", "hyp"}
        ref = [p for p, _ in truth[r["basename"]] if p not in MB.SILENT]
        assert r["n_ref"] == len(ref) == r["hits"] + r["sub"] + r["del"] and r["per"] == (r["sub"] + r["del"] + r["ins"]) / r["n_ref"]
        assert r["hyp"][0][1] == 0.0 and all(a[2] == b[1] for a, b in zip(r["hyp"], r["hyp"][1:]))
        assert round(r["hyp"][-1][2] * C.SR / C.HOP) == sum(d for _, d in truth[r["basename"]]) + 1
        hyp = [p for p, _, _ in r["hyp"] if p not in MB.SILENT]
        assert LR.edit_counts(ref, hyp)[0] == (r["hits"], r["sub"], r["del"], r["ins"])
    assert "skipped nowav: missing " in run.stdout
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["utterances"] == 8 and summary["missing"] == 1 and summary["lm"] == "bigram"
    err, n = sum(r["sub"] + r["del"] + r["ins"] for r in rows), sum(r["n_ref"] for r in rows)
    assert summary["n_ref"] == n and summary["per"] == err / n
    assert sum(c for _, _, c in summary["substitutions"]) <= summary["sub"] and len(summary["substitutions"]) <= 10
    print("PER of the recorded tones under their own model", summary["per"])
