"""GPU: the forced aligner's Gaussian-mixture emissions (fastspeech2_amd.align emit_gmm / stats_gmm / Aligner(mixtures=M),
csrc/fs2_align.hip) against the numpy oracle tests/align_gmm_ref.py: both kernels on ragged batches at the tile edges with NaN
padding, equality with the single-Gaussian kernel at M = 1, training and decoding on the bimodal corpus of tests/align_gmm_corpus.py,
run-to-run determinism and the command line."""
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
from tests import align_gmm_corpus as GC
from tests import align_gmm_ref as GR
from tests import align_ref as R
from tests.test_align_cpu import config
from tests.test_align_gpu import NAN, ROOT, RTOL, padded, rel_close, single_block_graph

pytestmark = pytest.mark.gpu
S = 2
LEX = {"a": ["X"], "abc": ["X", "Y", "Z"], "cab": ["Z", "X", "Y"]}
IDS = A.phone_table(LEX)
N_CLASSES = len(IDS) * S
# oracle accuracies (+-1 frame) on GC.corpus(SEED, N_UTT) with SEP 0.5, VSEP 3.0, SIGMA 1.0, measured on the host with the two numpy
# oracles before any GPU run: one Gaussian after ITERS passes, two components after 4 more passes
SEED, N_UTT, ITERS, MIX_ITERS = 1234, 40, 8, 4
A_REF_1, A_REF_2 = 0.8111, 0.9008


def tile_edge_batch(D, rng):
    """(T, J) of (1, 2), (31, 6), (33, 34), (70, 66), a single block and an utterance of exactly its mandatory states"""
    graphs = [single_block_graph(1, S), A.utterance_graph(["a"], LEX, IDS, S), A.utterance_graph(["abc", "cab"] * 2, LEX, IDS, S),
              A.utterance_graph(["abc", "cab"] * 4, LEX, IDS, S), single_block_graph(3, S),
              A.utterance_graph(["abc", "a", "cab"], LEX, IDS, S)]
    lens = [1, 31, 33, 70, 9, graphs[-1]["mandatory"]]
    assert [len(g["sid"]) for g in graphs[:4]] == [2, 6, 34, 66]
    return graphs, [rng.randn(T, D) for T in lens], lens


def tables(rng, M, D):
    """mixed K_c: class 0 has one active component, class 1 an active component of weight exactly 0 (when M > 1), the rest 1..M"""
    ncomp = rng.randint(1, M + 1, N_CLASSES)
    ncomp[0], ncomp[1] = 1, M
    w, mu, var = np.zeros((N_CLASSES, M)), np.zeros((N_CLASSES, M, D)), np.ones((N_CLASSES, M, D))
    for c, K in enumerate(ncomp):
        w[c, :K] = rng.dirichlet(np.ones(K))
        mu[c, :K] = 0.2 * rng.randn(1, D) + 0.1 * rng.randn(K, D)          # close components: responsibilities are soft
        var[c, :K] = 0.8 + 0.4 * rng.rand(K, D)
    if M > 1:
        w[1, 0], w[1, 1] = w[1, 0] + w[1, 1], 0.0
    return ncomp, w, mu, var


def dev_tables(dev, *t):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in t]


@pytest.fixture(scope="module")
def cases():
    """(D, M) -> batch, tables and the oracle's E and r, computed once"""
    out = {}
    for D in (160, 6):
        for M in (1, 2, 3, 8):
            rng = np.random.RandomState(100 * D + M)
            graphs, xs, lens = tile_edge_batch(D, rng)
            ncomp, w, mu, var = tables(rng, M, D)
            out[D, M] = (graphs, xs, lens, ncomp, w, mu, var, [GR.emissions(x, g["sid"], w, mu, var) for x, g in zip(xs, graphs)])
    return out


@pytest.mark.parametrize("D", [160, 6])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_emit_gmm_against_oracle(dev, cases, D, M):
    graphs, xs, lens, ncomp, w, mu, var, want = cases[D, M]
    G = A.Graphs(graphs, dev)
    x = padded(xs, NAN, np.float64, dev)
    wd, mud, vard = dev_tables(dev, w, mu, var)
    Tm = max(lens)
    out = torch.full((len(xs), Tm + 3, G.Jmax + 2), NAN, dtype=torch.float64, device=dev)[:, :Tm, :G.Jmax]          # strided views
    resp = torch.full((len(xs), Tm + 1, G.Jmax + 1, M), NAN, dtype=torch.float64, device=dev)[:, :Tm, :G.Jmax]
    E = A.emit_gmm(x, lens, G, wd, mud, vard, out=out, resp=resp)
    assert E.data_ptr() == out.data_ptr()
    E, r = E.cpu().numpy(), resp.cpu().numpy()
    soft = 0
    for b, (we, wr) in enumerate(want):
        T, J = lens[b], G.jl[b]
        rel_close(E[b, :T, :J], we)
        print("D", D, "M", M, "b", b, "max |r - oracle|", np.abs(r[b, :T, :J] - wr).max())
        assert np.abs(r[b, :T, :J] - wr).max() <= 1e-6
        assert np.isnan(E[b, T:]).all() and np.isnan(E[b, :, J:]).all()                      # padding is never written
        assert np.isnan(r[b, T:]).all() and np.isnan(r[b, :, J:]).all()
        for j, c in enumerate(graphs[b]["sid"]):
            assert (r[b, :T, j][:, w[c] == 0.0] == 0.0).all()                                # w = 0: exactly 0
        soft += int(((wr > 0.05) & (wr < 0.95)).sum())
    assert M == 1 or soft > 0
    plain = A.emit_gmm(x, lens, G, wd, mud, vard)                                             # decoding: no responsibilities
    for b in range(len(xs)):
        assert np.array_equal(plain[b, :lens[b], :G.jl[b]].cpu().numpy(), E[b, :lens[b], :G.jl[b]])       # the same bits


def test_one_component_of_weight_one_is_the_single_gaussian_kernel(dev, cases):
    graphs, xs, lens, ncomp, w, mu, var, _ = cases[160, 1]
    G = A.Graphs(graphs, dev)
    x = padded(xs, NAN, np.float64, dev)
    wd, mud, vard = dev_tables(dev, np.ones_like(w), mu, var)
    old = torch.zeros(len(xs), max(lens), G.Jmax, dtype=torch.float64, device=dev)
    new = torch.zeros_like(old)
    A.emit(x, lens, G, mud[:, 0], vard[:, 0], out=old)
    A.emit_gmm(x, lens, G, wd, mud, vard, out=new)
    assert torch.equal(old, new) and bool(old.abs().sum() > 0)
    bad = graphs[1]["sid"].copy()
    graphs = list(graphs)
    graphs[1] = dict(graphs[1], sid=np.where(np.arange(len(bad)) == 2, N_CLASSES + 5, bad).astype(np.int32))
    G = A.Graphs(graphs, dev)                                              # a class outside the table: NaN there, nothing else moves
    got = A.emit_gmm(x, lens, G, wd, mud, vard)
    assert bool(torch.isnan(got[1, :lens[1], 2]).all()) and torch.equal(got[1, :lens[1], :2], new[1, :lens[1], :2])


@pytest.mark.parametrize("D,M", [(160, 3), (6, 8), (160, 8)])
def test_stats_gmm_and_reduce_against_oracle(dev, cases, D, M):
    graphs, xs, lens, ncomp, w, mu, var, want = cases[D, M]
    G = A.Graphs(graphs, dev)
    x = padded(xs, NAN, np.float64, dev)
    cols = 1 + 2 * D
    bound = lambda ref: 1e-6 * max(1.0, np.abs(ref).max())                # noqa: E731  (the bar of the single-Gaussian stats test)

    def check(parts, ref, rows):
        p = parts.cpu().numpy()
        for b in rows:
            err = np.abs(p[b, :G.jl[b]] - ref[b]).max()
            print("D", D, "M", M, "b", b, "partials err", err, "bound", bound(ref[b]))
            assert err <= bound(ref[b])
            assert np.isnan(p[b, G.jl[b]:]).all()                                            # rows beyond J M stay unwritten

    # the oracle's gamma and r
    gammas = [R.posteriors(e, g)[0] for (e, _), g in zip(want, graphs)]
    pw = [GR.partials(gm, r, xx) for gm, (_, r), xx in zip(gammas, want, xs)]
    gd = padded(gammas, NAN, np.float64, dev)
    rd = torch.full((len(xs), max(lens), G.Jmax, M), NAN, dtype=torch.float64, device=dev)
    for b, (_, r) in enumerate(want):
        rd[b, :lens[b], :G.jl[b]] = torch.from_numpy(r).to(dev)
    parts = torch.full((len(xs), G.Jmax, M, cols), NAN, dtype=torch.float64, device=dev)
    assert A.stats_gmm(gd, rd, x, lens, G, out=parts).data_ptr() == parts.data_ptr()
    check(parts, pw, range(len(xs)))
    # the chain's own: utterances that have a path (the first has one frame for two states)
    sub = list(range(1, len(xs)))
    G1 = A.Graphs([graphs[b] for b in sub], dev)
    lens1, x1 = [lens[b] for b in sub], x[1:]
    wd, mud, vard = dev_tables(dev, w, mu, var)
    r1 = torch.full((len(sub), max(lens1), G1.Jmax, M), NAN, dtype=torch.float64, device=dev)
    E1 = A.emit_gmm(x1, lens1, G1, wd, mud, vard, resp=r1)
    alpha, loglik = A.forward(E1, lens1, G1)
    gamma = A.backward(E1, lens1, G1, alpha, loglik)
    own = torch.full((len(sub), G1.Jmax, M, cols), NAN, dtype=torch.float64, device=dev)
    A.stats_gmm(gamma, r1, x1, lens1, G1, out=own)
    p = own.cpu().numpy()
    for i, b in enumerate(sub):
        assert np.abs(p[i, :G1.jl[i]] - pw[b]).max() <= bound(pw[b])
        assert np.isnan(p[i, G1.jl[i]:]).all()
    # class sums with the component index: fp64 adds of a few dozen rows, held to the same bar
    ref = GR.class_sums(pw, graphs, N_CLASSES)
    pd = torch.full((len(xs), G.Jmax, M, cols), NAN, dtype=torch.float64, device=dev)
    for b, a in enumerate(pw):
        pd[b, :G.jl[b]] = torch.from_numpy(a).to(dev)
    sums = A.reduce(pd, G, N_CLASSES).cpu().numpy()
    assert sums.shape == (N_CLASSES * M, cols)
    assert np.abs(sums.reshape(N_CLASSES, M, cols) - ref).max() <= bound(ref)
    chain = A.reduce(parts, G, N_CLASSES, sums=A.reduce(parts, G, N_CLASSES)).cpu().numpy()
    assert np.abs(chain.reshape(N_CLASSES, M, cols) - 2 * ref).max() <= 2 * bound(ref)


@pytest.fixture(scope="module")
def corpus_run(dev):
    lex, utts = GC.corpus(SEED, N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    n_classes = len(ids) * C.STATES
    frames = [len(x) for x in xs]
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, 12 << 20, mixtures=2):
        mel = padded([utts[i]["mel"].T for i in batch], NAN, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        feats = A.features(mel, lens)
        for r, n in enumerate(lens):
            feats[r, n:] = NAN                                             # rows beyond an utterance must never be read
        batches.append((feats, lens, [graphs[i] for i in batch], batch))
    assert len(batches) >= 3

    def run():
        al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev, mixtures=2, mix_iters=MIX_ITERS)
        hist = al.fit([b[:3] for b in batches], ITERS)
        got = [None] * len(utts)
        for feats, lens, gs, batch in batches:
            for i, fr in zip(batch, al.align(feats, lens, gs)):
                got[i] = fr
        return [t.cpu().numpy().copy() for t in (al.gw, al.gmu, al.gvar)] + [al.ncomp.copy()], hist, got
    oracle = GR.fit(xs, graphs, n_classes, ITERS, mixtures=2, mix_iters=MIX_ITERS)
    return utts, graphs, xs, n_classes, run(), run, oracle


def test_fit_and_align_on_the_bimodal_corpus(corpus_run):
    """Oracle accuracies within +-1 frame measured on the host (40 utterances, seed 1234, SEP 0.5, VSEP 3.0, SIGMA 1.0, 8 passes with one
    Gaussian, then one split and 4 passes): A_REF_1 with one Gaussian, A_REF_2 with two components."""
    utts, graphs, xs, n_classes, ((gw, gmu, gvar, ncomp), hist, got), _, (w, mu, var, oncomp, ohist, _, (smu, svar)) = corpus_run
    print("loglik per frame", hist, ohist)
    assert len(hist) == ITERS + MIX_ITERS
    rel_close(hist, ohist)
    assert np.array_equal(ncomp, oncomp) and ncomp.max() == 2
    for a, b in ((gw, w), (gmu, mu), (gvar, var)):                          # the tables, to the bar of the statistics they come from
        print("table err", np.abs(a - b).max())
        assert np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(b).max())
    true = [[d for _, d in u["segments"]] for u in utts]
    want = [GR.align(x, g, w, mu, var) for x, g in zip(xs, graphs)]
    a_1 = C.accuracy(true, [R.align(x, g, smu, svar) for x, g in zip(xs, graphs)], 1)
    a_2, a_gpu = C.accuracy(true, want, 1), C.accuracy(true, got, 1)
    differ = sum(1 for a, b in zip(got, want) if not np.array_equal(a, b))
    print("utterances that differ", differ, "of", len(utts), "A_1", a_1, "A_2", a_2, "A_gpu", a_gpu)
    assert differ <= 0.02 * len(utts), differ
    assert A_REF_2 - A_REF_1 >= 0.05
    assert a_2 >= a_1 + 0.5 * (A_REF_2 - A_REF_1), (a_1, a_2)              # the corpus still shows what mixtures are for
    assert a_gpu >= a_2 - 0.01, (a_2, a_gpu)


def test_two_runs_are_bitwise_equal(corpus_run):
    _, _, _, _, (tabs, hist, got), run, _ = corpus_run
    tabs2, hist2, got2 = run()
    assert all(np.array_equal(a, b) for a, b in zip(tabs, tabs2)) and hist == hist2
    assert all(np.array_equal(a, b) for a, b in zip(got, got2))


def test_command_line_mixtures(dev, tmp_path):
    """`align.py cfg --mixtures 2` writes a TextGrid per utterance that the preprocessor's reader takes; `--mixtures 1` writes the
    bytes no flag writes."""
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 99, 8)
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(config(root, lexicon_path), f)
    cmd = [sys.executable, os.path.join(ROOT, "align.py"), os.path.join(root, "preprocess.yaml"), "--overwrite"]
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    files = {}
    for flags in ((), ("--mixtures", "1"), ("--mixtures", "2")):
        run = subprocess.run(cmd + list(flags), capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "8 TextGrids written, 0 utterances skipped" in run.stdout, run.stdout
        files[flags] = {name: open(tg(name), "rb").read() for name in truth}
        n_pass = len(run.stdout.split("log-likelihood per frame: ")[1].splitlines()[0].split())
        assert n_pass == (12 + 4 if flags == ("--mixtures", "2") else 12)
        assert ("mixtures: stage 2" in run.stdout) == (flags == ("--mixtures", "2"))
    assert files[()] == files[("--mixtures", "1")]
    for name, segs in truth.items():
        iv = P.read_textgrid(tg(name))["phones"]
        assert iv[0][0] == 0.0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
        assert int(round(iv[-1][1] * C.SR / C.HOP)) == sum(d for _, d in segs) + 1
        assert [p for _, _, p in iv if p not in P.SIL_PHONES] == [p for p, _ in segs if p not in P.SIL_PHONES]


def test_bad_arguments(dev):
    g = A.utterance_graph(["a"], LEX, IDS, S)
    G = A.Graphs([g], dev)
    D, T = 4, 8
    x = torch.zeros(1, T, D, dtype=torch.float64, device=dev)
    tab = lambda M, d=D, c=N_CLASSES: (torch.ones(c, M, dtype=torch.float64, device=dev) / max(M, 1),                 # noqa: E731
                                       torch.zeros(c, M, d, dtype=torch.float64, device=dev), torch.ones(c, M, d, dtype=torch.float64, device=dev))
    assert A.max_mixtures() == 8 == _lib.load().fs2_align_max_mixtures()
    for M in (0, 9):
        with pytest.raises(ValueError, match="mixture components"):
            A.emit_gmm(x, [T], G, *tab(M))
        with pytest.raises(ValueError):
            A.Aligner(N_CLASSES, D, S, dev, mixtures=M)
    E = torch.zeros(1, T, G.Jmax, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="supported are 1..8"):           # the ABI itself refuses before any launch
        w, mu, var = tab(8)
        _lib.call("fs2_align_emit_gmm", x.data_ptr(), x.stride(0), x.stride(1), G.jlens.data_ptr(), G.jlens.data_ptr(), G.sid.data_ptr(),
                  G.ldg, w.data_ptr(), mu.data_ptr(), var.data_ptr(), N_CLASSES, 9, D, E.data_ptr(), E.stride(0), E.stride(1), None, 0, 0, 0,
                  1, T, G.Jmax, None)
    w, mu, var = tab(2)
    with pytest.raises(ValueError, match="fit together"):
        A.emit_gmm(x, [T], G, w, mu[:, :1], var)                           # tables of different M
    with pytest.raises(ValueError, match="fit together"):
        A.emit_gmm(x, [T], G, w, *tab(2, D + 1)[1:])                       # another D
    with pytest.raises(ValueError, match="fit together"):
        A.emit_gmm(x, [T], G, w[:-1], mu, var)                             # another number of classes
    with pytest.raises(ValueError):
        A.emit_gmm(x, [T], G, w[:, 0], mu, var)                            # w is not (C, M)
    with pytest.raises(ValueError, match="on the GPU"):
        A.emit_gmm(x.cpu(), [T], G, w, mu, var)
    with pytest.raises(ValueError, match="on the GPU"):
        A.emit_gmm(x, [T], G, w.cpu(), mu, var)
    for shape in ((1, T, G.Jmax, 3), (1, T - 1, G.Jmax, 2), (1, T, G.Jmax - 1, 2), (2, T, G.Jmax, 2), (1, T, G.Jmax * 2)):
        with pytest.raises(ValueError):
            A.emit_gmm(x, [T], G, w, mu, var, resp=torch.zeros(shape, dtype=torch.float64, device=dev))
    resp = torch.zeros(1, T, G.Jmax, 2, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="on the GPU"):
        A.stats_gmm(E.cpu(), resp, x, [T], G)
    with pytest.raises(ValueError):
        A.stats_gmm(E, resp[:, :, :-1], x, [T], G)                         # fewer states than gamma
    with pytest.raises(ValueError):
        A.stats_gmm(E, resp, x, [T], G, out=torch.zeros(1, G.Jmax, 3, 1 + 2 * D, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        A.stats_gmm(E, torch.zeros(1, T, G.Jmax, 9, dtype=torch.float64, device=dev), x, [T], G)
