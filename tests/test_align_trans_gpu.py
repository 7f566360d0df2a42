"""GPU: the forced aligner's trained transition and optional-silence probabilities (fastspeech2_amd.align forward_arcs / backward_arcs /
viterbi_arcs / Aligner(transitions=1), csrc/fs2_align.hip) against the numpy oracle tests/align_trans_ref.py: the three scans with
arc costs on ragged batches whose padding is NaN, one batch per instantiation of the kernels; the bits of the scans without costs
when every cost is 0; the argument checks; training and decoding on the synthetic corpus of tests/align_corpus.py, alone, under
mixtures and on tied triphones; determinism; the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import _lib, align as A
from fastspeech2_amd import preprocess as P
from tests import align_corpus as C
from tests import align_ref as R
from tests import align_trans_ref as T
from tests.test_align_cpu import ITERS, N_UTT, SEED, config
from tests.test_align_gpu import NAN, ROOT, RTOL, padded, rel_close, single_block_graph
from tests.test_align_trans_cpu import without_final_sil

pytestmark = pytest.mark.gpu
LEX = {"a": ["X"], "bc": ["Y", "Z"]}


@functools.lru_cache(maxsize=None)
def cases():
    """Three batches, one per instantiation of the scans (the widest graph of a batch chooses it): up to 256 states (two utterances of
    the corpus with the oracle's flat-start emissions, a single block with T = 9, T equal to the mandatory states, one state and
    three states per phone, a last block that is mandatory), 257 .. 512 states, 1024 states.  -> [(graphs, Es, lens, w, edge)] with
    random finite negative costs."""
    lex, utts = C.corpus(SEED, 12)
    ids = A.phone_table(lex)
    S = C.STATES
    graphs = [A.utterance_graph(u["words"], lex, ids, S) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    mu, var, _ = R.fit(xs, graphs, len(ids) * S, 0)
    rng = np.random.RandomState(17)
    rand = lambda T_, g: 3.0 * rng.randn(T_, len(g["sid"]))               # noqa: E731
    small = [(g, R.emissions(x, g["sid"], mu, var)) for g, x in zip(graphs[:2], xs[:2])]
    g = single_block_graph(3, S)
    small.append((g, rand(9, g)))
    g = A.utterance_graph(sorted(lex)[:5], lex, ids, S)
    small.append((g, rand(g["mandatory"], g)))                             # exactly one path
    ids3 = A.phone_table(LEX)
    for S_, words, T_ in ((1, ["bc", "a", "a"], 13), (3, ["a", "bc"], 31)):
        g = A.utterance_graph(words, LEX, ids3, S_)
        small.append((g, rand(T_, g)))
    g = without_final_sil(A.utterance_graph(["bc", "a"], LEX, ids3, 2), 2)
    small.append((g, rand(17, g)))
    one = [w for w in sorted(lex) if len(lex[w]) == 2][0]
    g = A.utterance_graph([one] * 60, lex, ids, S)                         # 2 + 120 + 59 blocks: 362 states
    mid = [(g, rand(g["mandatory"] + 25, g)), small[4]]
    g = A.utterance_graph([one] * 170, lex, ids, S)                        # 2 + 340 + 169 = 511 blocks, 1022 states
    spn = ids["spn"] * S
    g = {"sid": np.concatenate([g["sid"], np.array([spn, spn + 1], np.int32)]),
         "skip": np.concatenate([g["skip"], np.array([509 * S + S - 1, -1], np.int32)]),
         "block": np.concatenate([g["block"], np.array([511, 511], np.int32)]), "alt": (g["alt"][0], -1),
         "blocks": g["blocks"] + [("spn", 170, False)], "mandatory": g["mandatory"] + S}      # one more word after an inner sil
    assert len(g["sid"]) == A.max_states() == 1024
    big = [(g, rand(g["mandatory"] + 30, g)), small[5]]
    out = []
    for batch, lo, hi in ((small, 1, 256), (mid, 257, 512), (big, 1024, 1024)):
        gs, Es = [b[0] for b in batch], [b[1] for b in batch]
        assert lo <= max(len(g["sid"]) for g in gs) <= hi
        w = [-rng.uniform(0.05, 3.0, (3, len(g["sid"]))) for g in gs]
        edge = -rng.uniform(0.05, 3.0, (len(gs), 4))
        out.append((gs, Es, [len(E) for E in Es], w, edge))
    return out


@functools.lru_cache(maxsize=None)
def references():
    return [[T.posteriors(E, g, wb, eb) + T.viterbi(E, g, wb, eb) for g, E, wb, eb in zip(gs, Es, w, edge)] for gs, Es, _, w, edge in cases()]


def upload(case, dev, zero=False):
    gs, Es, lens, w, edge = case
    G = A.Graphs(gs, dev)
    E = padded(Es, NAN, np.float64, dev)
    wbuf = torch.full((len(gs), 3, G.Jmax + 3), NAN, dtype=torch.float64, device=dev)    # a strided view, NaN beyond every utterance's states
    for b, wb in enumerate(w):
        wbuf[b, :, :wb.shape[1]] = 0.0 if zero else torch.from_numpy(wb).to(dev)
    ed = torch.zeros(len(gs), 4, dtype=torch.float64, device=dev) if zero else torch.from_numpy(edge).to(dev)
    return G, E, wbuf[:, :, :G.Jmax], ed


@pytest.mark.parametrize("k", [0, 1, 2])
def test_zero_costs_give_the_bits_of_the_scans_without_costs(dev, k):
    case = cases()[k]
    G, E, w, edge = upload(case, dev, zero=True)
    lens = case[2]
    nn = lambda t: torch.nan_to_num(t, nan=-1.0)                          # noqa: E731
    a0, l0 = A.forward(E, lens, G, out=torch.full_like(E, NAN))
    a1, l1 = A.forward_arcs(E, lens, G, w, edge, out=torch.full_like(E, NAN))
    assert torch.equal(nn(a0), nn(a1)) and torch.equal(l0, l1)
    g0 = A.backward(E, lens, G, a0, l0, out=torch.full_like(E, NAN))
    g1, _ = A.backward_arcs(E, lens, G, w, edge, a1, l1, out=torch.full_like(E, NAN))
    assert torch.equal(nn(g0), nn(g1)) and not torch.isnan(g1[0, :lens[0], :G.jl[0]]).any()
    b0, e0, s0 = A.viterbi(E, lens, G, out=torch.full(E.shape, 77, dtype=torch.uint8, device=dev))
    b1, e1, s1 = A.viterbi_arcs(E, lens, G, w, edge, out=torch.full(E.shape, 77, dtype=torch.uint8, device=dev))
    assert torch.equal(b0, b1) and torch.equal(e0, e1) and torch.equal(s0, s1)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_scans_with_costs_against_the_oracle(dev, k):
    case, want = cases()[k], references()[k]
    gs, Es, lens, _, _ = case
    G, E, w, edge = upload(case, dev)
    alpha = torch.full_like(E, NAN)
    _, loglik = A.forward_arcs(E, lens, G, w, edge, out=alpha)
    rel_close(loglik.cpu().numpy(), [r[3] for r in want])
    a = alpha.cpu().numpy()
    for b, r in enumerate(want):
        fin, got = np.isfinite(r[2]), a[b, :lens[b], :G.jl[b]]
        assert np.array_equal(np.isneginf(got), np.isneginf(r[2])), b
        rel_close(got[fin], r[2][fin])
        assert np.isnan(a[b, lens[b]:]).all() and np.isnan(a[b, :, G.jl[b]:]).all()               # padding is never written
    xbuf = torch.full((len(gs), G.Jmax + 2, 7), NAN, dtype=torch.float64, device=dev)
    own, xi_own = A.backward_arcs(E, lens, G, w, edge, alpha, loglik, out=torch.full_like(E, NAN), xi=xbuf[:, :, :5])
    gamma, xi = A.backward_arcs(E, lens, G, w, edge, alpha, loglik)        # written over alpha
    assert gamma.data_ptr() == alpha.data_ptr() and xi_own.data_ptr() == xbuf.data_ptr()
    nn = lambda t: torch.nan_to_num(t, nan=-1.0)                          # noqa: E731
    assert torch.equal(nn(own), nn(gamma))
    gm, x, xo = gamma.cpu().numpy(), xi.cpu().numpy(), xbuf.cpu().numpy()
    for b, r in enumerate(want):
        J = G.jl[b]
        assert np.abs(gm[b, :lens[b], :J] - r[0]).max() <= 1e-6, b
        assert np.abs(x[b, :J] - r[1]).max() <= 1e-6, b
        assert np.array_equal(xo[b, :J, :5], x[b, :J])                     # its own strided buffer: the same bits
        assert np.isnan(gm[b, lens[b]:]).all() and np.isnan(gm[b, :, J:]).all()
        assert np.isnan(xo[b, J:]).all() and np.isnan(xo[b, :, 5:]).all()
        if lens[b] == gs[b]["mandatory"]:                                  # one path: every arc posterior is 0 or 1
            assert np.abs(x[b, :J] - np.round(x[b, :J])).max() <= 1e-9 and x[b, :J, 1].sum() > 1
    bp, end, score = A.viterbi_arcs(E, lens, G, w, edge, out=torch.full(E.shape, 77, dtype=torch.uint8, device=dev))
    frames = A.backtrack(bp, lens, G, end).cpu().numpy()
    bp, end = bp.cpu().numpy(), end.cpu().numpy()
    rel_close(score.cpu().numpy(), [r[7] for r in want])
    for b, (r, g) in enumerate(zip(want, gs)):
        assert np.array_equal(bp[b, :lens[b], :G.jl[b]], r[4]), b
        assert (bp[b, lens[b]:] == 77).all() and (bp[b, :, G.jl[b]:] == 77).all()
        assert end[b] == r[5] and np.array_equal(frames[b, :len(g["blocks"])], r[6]) and r[6].sum() == lens[b], b


def test_bad_arguments(dev):
    case = cases()[0]
    G, E, w, edge = upload(case, dev)
    lens = case[2]
    wc = w.contiguous()
    with pytest.raises(ValueError):
        A.forward_arcs(E, lens, G, wc[:, :, :G.Jmax - 1], edge)            # fewer columns than states
    with pytest.raises(ValueError):
        A.forward_arcs(E, lens, G, wc[:, :2], edge)
    with pytest.raises(ValueError):
        A.viterbi_arcs(E, lens, G, wc, edge[:, :3])
    with pytest.raises(ValueError):
        A.forward_arcs(E, lens, G, torch.stack([wc, wc], 1)[:, 0], edge)   # the three rows of an utterance are not ldw apart
    with pytest.raises(ValueError, match="on the GPU"):
        A.forward_arcs(E, lens, G, wc.cpu(), edge)
    alpha, loglik = A.forward_arcs(E, lens, G, w, edge)
    with pytest.raises(ValueError):
        A.backward_arcs(E, lens, G, w, edge, alpha, loglik, xi=torch.zeros(len(lens), G.Jmax, 4, dtype=torch.float64, device=dev))
    # the ABI itself: FS2_EINVAL before any launch, the outputs stay as they were
    B, Tmax, J = E.shape[0], E.shape[1], G.Jmax
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full_like(E, NAN)
    ll = torch.full((B,), NAN, dtype=torch.float64, device=dev)
    xi = torch.full((B, J, 5), NAN, dtype=torch.float64, device=dev)
    bp = torch.full(E.shape, 77, dtype=torch.uint8, device=dev)
    end = torch.full((B,), -7, dtype=torch.int32, device=dev)

    def fwd(wp, ldw, ep):
        _lib.call("fs2_align_forward_arcs", E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), G.skip.data_ptr(),
                  G.ldg, G.alt.data_ptr(), wp, ldw, ep, out.data_ptr(), out.stride(0), out.stride(1), ll.data_ptr(), B, Tmax, J, None)

    def bwd(wp, ldw, ep, ldx_b, ldx_j):
        _lib.call("fs2_align_backward_arcs", E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), G.skip.data_ptr(),
                  G.ldg, G.alt.data_ptr(), wp, ldw, ep, alpha.data_ptr(), alpha.stride(0), alpha.stride(1), loglik.data_ptr(), out.data_ptr(),
                  out.stride(0), out.stride(1), xi.data_ptr(), ldx_b, ldx_j, B, Tmax, J, None)

    def vit(wp, ldw, ep):
        _lib.call("fs2_align_viterbi_arcs", E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(), G.skip.data_ptr(),
                  G.ldg, G.alt.data_ptr(), wp, ldw, ep, bp.data_ptr(), bp.stride(0), bp.stride(1), end.data_ptr(), ll.data_ptr(), B, Tmax, J,
                  None)
    for call in (fwd, vit):
        for args in ((None, wc.stride(1), edge.data_ptr()), (wc.data_ptr(), wc.stride(1), None), (wc.data_ptr(), J - 1, edge.data_ptr())):
            with pytest.raises(ValueError, match="arc cost"):
                call(*args)
    for args in ((None, wc.stride(1), edge.data_ptr(), 5 * J, 5), (wc.data_ptr(), J - 1, edge.data_ptr(), 5 * J, 5)):
        with pytest.raises(ValueError, match="arc cost"):
            bwd(*args)
    for ldx in ((5 * J, 4), (5 * J - 1, 5)):
        with pytest.raises(ValueError, match="xi strides"):
            bwd(wc.data_ptr(), wc.stride(1), edge.data_ptr(), *ldx)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ll).all() and torch.isnan(xi).all() and (bp == 77).all() and (end == -7).all()
    with pytest.raises(ValueError, match="transitions"):
        A.Aligner(6, 4, 2, dev, transitions=2)


# ------------------------------------------------------------------------------------------------ the schedule
@functools.lru_cache(maxsize=None)
def oracle_mono():
    lex, utts = C.corpus(SEED, N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    return utts, ids, graphs, xs, T.fit_mono(xs, graphs, len(ids) * C.STATES, ITERS)


@pytest.fixture(scope="module")
def corpus_run(dev):
    utts, ids, graphs, xs, _ = oracle_mono()
    n_classes, frames = len(ids) * C.STATES, [len(x) for x in xs]
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, 12 << 20, mixtures=2, transitions=1):
        mel = padded([utts[i]["mel"].T for i in batch], NAN, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        feats = A.features(mel, lens)
        for r, n in enumerate(lens):
            feats[r, n:] = NAN                                             # rows beyond an utterance must never be read
        batches.append((feats, lens, [graphs[i] for i in batch], batch))
    assert len(batches) >= 3

    def run(**kw):
        al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev, phone_ids=ids if kw.get("triphones") else None, **kw)
        hist = al.fit([b[:3] for b in batches], ITERS)
        got = [None] * len(utts)
        for feats, lens, gs, batch in batches:
            for i, fr in zip(batch, al.align(feats, lens, gs)):
                got[i] = fr
        return al, hist, got
    return run


def max_close(got, want):
    assert got.shape == want.shape and np.abs(got - want).max() <= RTOL * np.abs(want).max()


def compare(al, hist, got, want, xs):
    print("loglik per frame", hist, want["history"], "opt", al.opt, want["opt"])
    assert len(hist) == len(want["history"])
    rel_close(hist, want["history"])
    rel_close(al.loop, want["loop"])
    rel_close(al.opt, want["opt"])
    max_close(al.mu.cpu().numpy(), want["mu"])
    rel_close(al.var.cpu().numpy(), want["var"])
    frames = [T.align(x, g, want) for x, g in zip(xs, want["graphs"])]
    differ = [i for i, (a, b) in enumerate(zip(got, frames)) if not np.array_equal(a, b)]
    assert not differ, differ


def test_fit_and_align_against_the_oracle(corpus_run):
    utts, ids, graphs, xs, mono = oracle_mono()
    al, hist, got = corpus_run(transitions=1)
    compare(al, hist, got, dict(mono, graphs=graphs), xs)
    assert al.loop.shape == (len(ids) * C.STATES,) and al.opt.shape == (3,) and not np.all(al.loop == 0.5) and not np.all(al.opt == 0.5)
    assert al.opt[1] < 0.5                                                 # a pause follows 3 words in 10 in this corpus
    al2, hist2, got2 = corpus_run(transitions=1)                           # two runs: the same bits
    assert hist == hist2 and np.array_equal(al.loop, al2.loop) and np.array_equal(al.opt, al2.opt)
    assert torch.equal(al.mu, al2.mu) and torch.equal(al.var, al2.var) and all(np.array_equal(a, b) for a, b in zip(got, got2))
    old, hist_old, got_old = corpus_run()                                  # the default: no table moves, nothing else does
    new, hist_new, got_new = corpus_run(transitions=0)
    assert hist_old == hist_new and torch.equal(old.mu, new.mu) and all(np.array_equal(a, b) for a, b in zip(got_old, got_new))
    assert np.all(new.loop == 0.5) and np.all(new.opt == 0.5) and hist_new != hist


def test_under_mixtures(corpus_run):
    utts, ids, graphs, xs, mono = oracle_mono()
    want = T.fit(xs, graphs, len(ids) * C.STATES, ITERS, mixtures=2, mix_iters=2, front=mono)
    al, hist, got = corpus_run(transitions=1, mixtures=2, mix_iters=2)
    assert len(hist) == ITERS + 2
    compare(al, hist, got, want, xs)
    assert np.array_equal(al.ncomp, want["ncomp"]) and al.ncomp.max() == 2
    max_close(al.gmu.cpu().numpy(), want["gmu"])
    max_close(al.gw.cpu().numpy(), want["w"])
    assert not np.array_equal(want["loop"], mono["loop"])                  # the mixture passes moved the tables


LEAVES, TRI_ITERS, TRI_MIN_OCC = 40, 2, 20.0                               # the smallest leaf budget of tests/test_align_tri_gpu.py


def test_on_tied_triphones(corpus_run):
    utts, ids, graphs, xs, mono = oracle_mono()
    want = T.fit(xs, graphs, len(ids) * C.STATES, ITERS, leaves=LEAVES, tri_iters=TRI_ITERS, min_occ=TRI_MIN_OCC, phone_ids=ids,
                 states=C.STATES, front=mono)
    al, hist, got = corpus_run(transitions=1, triphones=LEAVES, tri_iters=TRI_ITERS, tri_min_occ=TRI_MIN_OCC)
    assert len(hist) == ITERS + 1 + TRI_ITERS
    for key, ref in zip(("question", "yes", "no", "leaf"), want["tree"]):
        assert np.array_equal(al.tree[key], ref), key
    assert al.n_classes == want["n_leaves"] > len(ids) * C.STATES and al.loop.shape == (want["n_leaves"],)
    compare(al, hist, got, want, xs)


def test_command_line_transitions(dev, tmp_path):
    """`align.py cfg --transitions 1` writes a TextGrid per utterance that the preprocessor's reader takes; a second run writes the
    same bytes."""
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 99, 8)
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(config(root, lexicon_path), f)
    cmd = [sys.executable, os.path.join(ROOT, "align.py"), os.path.join(root, "preprocess.yaml"), "--transitions", "1"]
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    files = []
    for extra in ((), ("--overwrite",)):
        run = subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "8 TextGrids written, 0 utterances skipped" in run.stdout, run.stdout
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("transitions: ")]
        assert len(line) == 1 and " opt " in line[0] and "frames per state" in line[0], run.stdout
        assert len(run.stdout.split("log-likelihood per frame: ")[1].splitlines()[0].split()) == 12
        files.append({name: open(tg(name), "rb").read() for name in truth})
        for name, segs in truth.items():
            iv = P.read_textgrid(tg(name))["phones"]
            assert iv[0][0] == 0.0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
            assert int(round(iv[-1][1] * C.SR / C.HOP)) == sum(d for _, d in segs) + 1
            assert [p for _, _, p in iv if p not in P.SIL_PHONES] == [p for p, _ in segs if p not in P.SIL_PHONES]
    assert files[0] == files[1]
