"""GPU: the grapheme-to-phoneme kernels (csrc/fs2_g2p.hip) and the trained model against the float64 reference tests/g2p_ref.py.
fp64 values to the project's RTOL; decisions (backpointers, kept candidates, phones) exactly, except for a word whose deciding gap, as
the reference reports it, is above 0 and below 1e-9 |score| (at most 2 % of the words).  A gap of exactly 0 is a tie, which the
specification decides (the lower code, slot or candidate number): there the two sides must agree like anywhere else.  All padding is
-1 ids or NaN."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib, g2p
from tests import g2p_corpus, g2p_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-6                                                                # tests/test_align_gpu.py
NEAR = 1e-9
A, P = 6, 8
DEV = "cuda"
BARS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2p_bars.json")


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(got[~fin], want[~fin])
    assert np.all(np.abs(got[fin] - want[fin]) <= RTOL * np.abs(want[fin])), np.abs(got[fin] - want[fin]).max()


# ------------------------------------------------------------------------------------------------ the lattice
def _lattice_words():
    rng = np.random.RandomState(3)
    w = lambda lg, lp: (rng.randint(0, A, lg).tolist(), rng.randint(0, P, lp).tolist())      # noqa: E731
    words = [w(1, 0), w(1, 1), w(1, 2), w(2, 1), w(3, 6), w(3, 0), w(1, 3), w(32, 48), w(5, 4)]    # 9: not a multiple of 4
    words[3] = ([0, 1], [2])
    return words


@pytest.fixture(scope="module")
def lattice():
    words = _lattice_words()
    _, cnt = g2p_ref.counts_of(words, np.zeros(g2p_ref.table_size(A, P)), A, P)            # the reference's flat-start estimate
    table = g2p_ref.m_step(cnt, A, P)
    ref = [g2p_ref.expect(L, Ph, table, A, P) for L, Ph in words]
    vit = [g2p_ref.viterbi(L, Ph, table, A, P) for L, Ph in words]
    return words, table, ref, vit


def _device_words(words):
    L, g = g2p.pack_ids([w[0] for w in words], 32)
    Ph, p = g2p.pack_ids([w[1] for w in words], 48)
    t = lambda a: torch.as_tensor(a).to(DEV)                                                # noqa: E731
    return L, Ph, g, p, t(L), t(Ph), t(g), t(p)


@pytest.mark.parametrize("which", ["batch", "one"])
def test_m2m_expect_and_viterbi_match_the_reference(lattice, which):
    words, table, ref, vit = lattice
    pick = list(range(len(words))) if which == "batch" else [4]
    ws = [words[k] for k in pick]
    _, _, g, p, dL, dPh, dg, dp = _device_words(ws)
    tab = torch.as_tensor(table).to(DEV)
    post = torch.full((len(ws), 32, 49, 4), float("nan"), dtype=torch.float64, device=DEV)
    ll, post = g2p.m2m_expect(dL, dPh, dg, dp, tab, A, P, 32, 48, post=post)
    bp = torch.full((len(ws), 33, 49), 77, dtype=torch.uint8, device=DEV)
    score, bp = g2p.m2m_viterbi(dL, dPh, dg, dp, tab, A, P, 32, 48, bp=bp)
    ll, post, score, bp = ll.cpu().numpy(), post.cpu().numpy(), score.cpu().numpy(), bp.cpu().numpy()
    for r, k in enumerate(pick):
        Lg, Lp = int(g[r]), int(p[r])
        want_ll, want_post = ref[k]
        inside = post[r, :Lg, :Lp + 1]
        assert not np.isnan(inside).any()
        assert np.isnan(post[r, Lg:]).all() and np.isnan(post[r, :Lg, Lp + 1:]).all()      # nothing outside the word's cells
        _close([ll[r]], [want_ll])
        assert np.array_equal(inside == 0.0, want_post == 0.0)                              # absent arcs are exactly 0
        _close(inside, want_post)
        if want_ll == -math.inf:
            assert ll[r] == -math.inf and not inside.any()
        else:
            consumed = sum(inside[..., c].sum() * g2p.ARCS[c][0] for c in range(4))
            assert abs(consumed - Lg) <= 1e-9 * Lg
        want_score, want_bp, _, gap = vit[k]
        _close([score[r]], [want_score])
        assert np.all(bp[r, Lg + 1:] == 77) and np.all(bp[r, :Lg + 1, Lp + 1:] == 77)
        if not 0.0 < gap < NEAR * abs(want_score):
            assert np.array_equal(bp[r, :Lg + 1, :Lp + 1], want_bp), k
    assert ll[pick.index(4)] > -math.inf
    if which == "batch":
        assert ll[6] == -math.inf and score[6] == -math.inf


def test_count_reduction_matches_the_reference_and_repeats_bit_for_bit(lattice):
    words, table, _, _ = lattice
    L, Ph, g, p, dL, dPh, dg, dp = _device_words(words)
    tab = torch.as_tensor(table).to(DEV)
    _, post = g2p.m2m_expect(dL, dPh, dg, dp, tab, A, P, 32, 48)
    flat = g2p.arc_types(L, Ph, g, p, A, P).ravel()
    assert flat.size == post.numel()
    at = np.nonzero(flat >= 0)[0]
    types = np.unique(flat[at])
    comp = np.searchsorted(types, flat[at])
    o = np.argsort(comp, kind="stable")
    items = torch.as_tensor(at[o].astype(np.int32)).to(DEV)
    offs = torch.as_tensor(np.searchsorted(comp[o], np.arange(len(types) + 1)).astype(np.int32)).to(DEV)
    runs = []
    for _ in range(2):
        counts = torch.full((len(types),), float("nan"), dtype=torch.float64, device=DEV)
        _lib.call("fs2_align_reduce", post.data_ptr(), 1, post.numel(), offs.data_ptr(), items.data_ptr(), len(types), 1, counts.data_ptr(),
                  0, torch.cuda.current_stream().cuda_stream)
        runs.append(counts.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()
    _, cnt = g2p_ref.counts_of(words, table, A, P)
    assert sorted(cnt) == types.tolist()
    _close(runs[0], [cnt[t] for t in types.tolist()])


# ------------------------------------------------------------------------------------------------ the n-gram and the search
@pytest.fixture(scope="module")
def small():
    """a reference model of 120 words after two E-steps; the n-gram of orders 1, 2 and 4 over its alignments"""
    lex = g2p_corpus.lexicon(1, 140)
    entries, letters, phones = g2p_corpus.ids(lex)
    train, held = entries[:120], entries[120:]
    m = g2p_ref.train_model(train, A, P, order=4, iters=2)
    T = len(m["tokens"])
    out = {"m": m, "T": T, "held": held, "lms": {}}
    for N in (1, 2, 4):
        lm = g2p.kneser_ney(m["seqs"], T, N)
        model = g2p.G2P(letters + ["z"], phones, m["type_letters"], m["type_phones"], lm, N, 64, {}, DEV)     # z: a letter nothing spells
        out["lms"][N] = (lm, g2p_ref.model_from_arrays(lm, N), model)
    return out


@pytest.mark.parametrize("N", [1, 4])
def test_ngram_score_takes_every_branch(small, N):
    T = small["T"]
    lm, md, model = small["lms"][N]
    rng = np.random.RandomState(5)
    hists = [(T, T, T)]
    for s in small["m"]["seqs"][:40]:
        padded = [T, T, T] + list(s)
        hists += [tuple(padded[k:k + 3]) for k in range(len(padded) - 2)]
    hists += [tuple(rng.randint(0, T, 3).tolist()) for _ in range(40)]                     # mostly unseen histories
    hists = sorted(set(hists))
    pairs = [(h, w) for h in hists for w in list(range(T)) + [T + 1]]
    level = {n: 0 for n in range(1, N + 1)}
    unseen_hist = 0
    for h, w in pairs:
        ctx = h[3 - (N - 1):] if N > 1 else ()
        for n in range(N, 0, -1):
            c = ctx[len(ctx) - (n - 1):] if n > 1 else ()
            if c + (w,) in md[n]:
                level[n] += 1
                break
            unseen_hist += n > 1 and c not in md[n - 1]
    assert all(v > 0 for v in level.values()), level                      # a hit at every order: back-off by 0 .. N - 1 levels
    assert N == 1 or unseen_hist > 0
    hist = torch.as_tensor(np.array([h[3 - (N - 1):] if N > 1 else () for h, _ in pairs], np.int32).reshape(len(pairs), N - 1))
    hist = torch.cat([hist, torch.full((len(pairs), 1), -1, dtype=torch.int32)], 1).to(DEV)   # a padded row stride
    tok = torch.as_tensor(np.array([w for _, w in pairs], np.int32)).to(DEV)
    _, ngram = model._tables()
    got = g2p.ngram_score(hist, tok, ngram).cpu().numpy()
    want = np.array([g2p_ref.lookup(md, N, h, w) for h, w in pairs])
    assert np.array_equal(got, want)                                       # the same additions in the same order
    assert np.isfinite(want).all()


def _decode_words(small):
    return g2p_corpus.decode_words(small["held"], A)


@pytest.mark.parametrize("N", [1, 2, 4])
@pytest.mark.parametrize("K", [1, 4, 256])
def test_decode_matches_the_reference_beam_search(small, N, K):
    assert g2p.limits()["beam"] == 256
    T, m = small["T"], small["m"]
    lm, md, model = small["lms"][N]
    words = _decode_words(small)
    L, g = g2p.pack_ids(words, 33)
    speller, ngram = model._tables()
    ph, n, score, beams = g2p.decode(torch.as_tensor(L).to(DEV), torch.as_tensor(g).to(DEV), speller, ngram, K, 32, full=True)
    ph, n, score = ph.cpu().numpy(), n.cpu().numpy(), score.cpu().numpy()
    beams = {k: v.cpu().numpy() for k, v in beams.items()}
    left_out = 0
    for r, word in enumerate(words):
        want, want_score, want_beams, gap = g2p_ref.beam_search(word, m["spelling"], md, N, K, T, m["type_phones"])
        if want is None:
            assert n[r] == -1 and score[r] == -math.inf, word
            continue
        if 0.0 < gap < NEAR * abs(want_score):
            left_out += 1
            continue
        assert n[r] == len(want) and ph[r, :n[r]].tolist() == want, word
        assert score[r] == want_score
        for i in range(1, len(word) + 1):
            assert beams["n"][r, i] == len(want_beams[i])
            for k, (sc, hist, ppos, pslot) in enumerate(want_beams[i]):
                h = int(beams["hist"][r, i, k])
                assert beams["score"][r, i, k] == sc
                assert ((h >> 32) & 0xffff, (h >> 16) & 0xffff, h & 0xffff) == tuple(hist)
                assert beams["bp"][r, i, k] == 2 * pslot + (i - ppos - 1)
        if K == 256 and len(word) <= 3:
            brute, brute_score, n_paths = g2p_ref.brute_force(word, m["spelling"], md, N, T, m["type_phones"])
            assert n_paths <= K and brute == want and brute_score == want_score
    assert left_out <= 0.02 * len(words)
    assert n[words.index([0, -1, 3])] == -1 and n[words.index([1, 6])] == -1 and n[words.index([6])] == -1


# ------------------------------------------------------------------------------------------------ end to end
def test_training_end_to_end_matches_the_reference():
    bars = json.load(open(BARS))
    lex = g2p_corpus.lexicon(bars["corpus_seed"])
    model = g2p.G2P.train(lex, order=bars["order"], beam=bars["beam"], device=DEV, holdout=bars["holdout"], seed=bars["split_seed"])
    hist = model.summary["loglik"]
    print("loglik", hist, "reference", bars["loglik"], "wer", model.summary["holdout_wer"])
    assert all(b >= a for a, b in zip(hist, hist[1:]))
    assert len(hist) == len(bars["loglik"])
    _close(hist, bars["loglik"])
    rows = bars["held_out"]
    assert [w for w, _ in model.held_out] == [r["word"] for r in rows]
    got = model.pronounce([r["word"] for r in rows])
    left_out = [r for r in rows if r["gap"] is not None and 0.0 < r["gap"] < NEAR]
    assert len(left_out) <= 0.02 * len(rows)
    for r, ph in zip(rows, got):
        if r not in left_out:
            assert ph == r["phones"], r["word"]
    right = sum(1 for (_, truth), ph in zip(model.held_out, got) if ph == truth)
    assert right >= round(bars["word_accuracy"] * len(rows)) - 1
    assert model.summary["graphone_types"] == bars["graphone_types"]


def test_limits_are_refused_before_any_launch():
    t = torch.zeros(4, dtype=torch.int32, device=DEV).reshape(1, 4)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    tab = torch.zeros(g2p.table_size(A, P), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        g2p.m2m_expect(t, t, one, one, tab, A, P, 33, 4)
    with pytest.raises(ValueError):
        g2p.m2m_expect(t, t, one, one, tab[:-1], A, P, 4, 4)
    with pytest.raises(ValueError):
        g2p.m2m_viterbi(t, t, one, one, tab, A, P, 4, 49)


# ------------------------------------------------------------------------------------------------ the aligner and the synthesizer
def test_align_gives_an_out_of_lexicon_word_the_models_phones(tmp_path):
    """align.build(..., g2p=) on the aligner tests' tone corpus: with every word in the lexicon the TextGrids are byte-identical with
    and without the model; with one word taken out of the lexicon (after the model was trained on it) that word's phones in the
    TextGrid are the model's, not spn."""
    from fastspeech2_amd import align as AL
    from fastspeech2_amd import preprocess as PP
    from tests import align_corpus
    from tests.test_align_cpu import config
    root = str(tmp_path)
    lexicon_path, truth = align_corpus.wav_corpus(root, 99, 6)
    lex = AL.read_lexicon(lexicon_path)
    model = g2p.G2P.train(lex, order=2, iters=3, device=DEV)
    cfg = config(root, lexicon_path)
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")          # noqa: E731

    def run(g, capsys=None):
        written, skipped, _ = AL.build(cfg, device=DEV, iters=2, overwrite=True, g2p=g)
        assert written == len(truth) and not skipped
        return {name: open(tg(name), "rb").read() for name in truth}

    assert run(None) == run(model)                                        # no OOV word: nothing changes
    words = {name: open(os.path.join(root, "raw", "spk", name + ".lab")).read().split() for name in truth}
    spoken = sorted({w for ws in words.values() for w in ws})
    said = dict(zip(spoken, model.pronounce(spoken)))
    gone = None
    for w in spoken:
        rest = AL.phone_table({k: v for k, v in lex.items() if k != w})
        if said[w] and all(p in rest for p in said[w]):
            gone = w
            break
    assert gone is not None
    with open(lexicon_path, "w") as f:
        for w in sorted(lex):
            if w != gone:
                f.write(w.upper() + "\t" + " ".join(lex[w]) + "\n")
    path = os.path.join(root, "model.npz")
    model.save(path)
    run(path)                                                              # the command line's way: a file
    hit = 0
    for name, ws in words.items():
        labels = [p for _, _, p in PP.read_textgrid(tg(name))["phones"] if p not in PP.SIL_PHONES]
        assert labels == [p for w in ws for p in (said[w] if w == gone else lex[w])], name
        assert "spn" not in labels
        hit += gone in ws
    assert hit > 0
    without = run(None)
    assert any(b"spn" in without[name] for name, ws in words.items() if gone in ws)


LEXICON = """HELLO HH AH0 L OW1\nWORLD W ER1 L D\nHAT HH AE1 T\nCOT K AA1 T\nCALL K AO1 L\nTALL T AO1 L\nHOT HH AA1 T\nCOAT K OW1 T
LOW L OW1\nDOT D AA1 T\nCOLD K OW1 L D\nTOLD T OW1 L D\nAT AE1 T\nACT AE1 K T\n"""


def test_synthesize_single_takes_free_text_with_a_model(tmp_path, capsys):
    import copy
    import yaml
    import synthesize as synth_cli
    from fastspeech2_amd.align import read_lexicon
    from fastspeech2_amd.model import FastSpeech2
    from tests.golden import configs
    from tests.helpers import make_preprocessed_dir
    root = str(tmp_path)
    lexicon_path = os.path.join(root, "lexicon.txt")
    open(lexicon_path, "w").write(LEXICON)
    model = g2p.G2P.train(lexicon_path, order=2, iters=3, device=DEV)
    model.save(os.path.join(root, "g2p.npz"))
    pcfg, mcfg = configs.make(dec_layers=1, enc_layers=1)
    pcfg["path"]["preprocessed_path"] = make_preprocessed_dir(os.path.join(root, "data"), seed=31, n_train=8, n_val=2, lo=6, hi=12)
    pcfg["path"]["lexicon_path"] = lexicon_path
    pcfg["preprocessing"]["text"]["language"] = "en"
    tcfg = copy.deepcopy(configs.TRAIN)
    tcfg["path"] = {k: os.path.join(root, "out", k.split("_")[0]) for k in ("ckpt_path", "log_path", "result_path")}
    paths = []
    for name, cfg in (("preprocess.yaml", pcfg), ("model.yaml", mcfg), ("train.yaml", tcfg)):
        paths.append(os.path.join(root, name))
        with open(paths[-1], "w") as f:
            yaml.safe_dump(cfg, f)
    os.makedirs(tcfg["path"]["ckpt_path"])
    torch.manual_seed(11)
    msd = FastSpeech2(pcfg, mcfg).state_dict()
    key = "variance_adaptor.duration_predictor.linear_layer.bias"         # an untrained duration predictor says no frames at all
    msd[key] = torch.full_like(msd[key], 1.5)
    torch.save({"model": msd}, os.path.join(tcfg["path"]["ckpt_path"], "1.pth.tar"))
    text = "Hello, WORLD cat 42!"
    cat = model.pronounce(["cat"])[0]
    assert cat is not None and model.pronounce(["42"]) == [None]
    lex = read_lexicon(lexicon_path)
    want = "{" + " ".join(lex["hello"] + ["sp"] + lex["world"] + cat) + "}"
    capsys.readouterr()
    synth_cli.main(synth_cli.parse_args(["--restore_step", "1", "--mode", "single", "--text", text, "--g2p_model", os.path.join(root, "g2p.npz"),
                                         "-p", paths[0], "-m", paths[1], "-t", paths[2], "--random_vocoder"]))
    out = capsys.readouterr().out
    assert "Raw Text Sequence: " + text in out and "Phoneme Sequence: " + want in out
    assert "no pronunciation for 42" in out
    assert os.path.exists(os.path.join(tcfg["path"]["result_path"], "Hello,_WORLD_cat_42!.wav"))
