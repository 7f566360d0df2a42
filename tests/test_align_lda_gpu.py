"""GPU: the forced aligner's LDA stage (fastspeech2_amd.align splice / scatter / project / Aligner(lda=k),
csrc/fs2_align_lda.hip) against the numpy oracle tests/align_lda_ref.py: the three kernels elementwise on ragged batches with NaN
padding, at D_s under one 16-tile, at a ragged tile edge, at the customary 560 and at the limit of 720; the whole schedule and
decoding on the correlated-channel corpus of tests/align_lda_corpus.py; the untouched default; the command line."""
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
from tests import align_lda_corpus as LC
from tests import align_lda_ref as LR
from tests import align_ref as R
from tests.test_align_cpu import config
from tests.test_align_gpu import NAN, ROOT, padded
from tests.test_align_lda_cpu import E2E_ITERS, E2E_K, E2E_LDA_ITERS, E2E_N_UTT, E2E_SEED, E2E_SPLICE

pytestmark = pytest.mark.gpu
# (n_mel, c, lens, k): D_s = 15 under one 16-tile (k = D_s), 35 a ragged tile edge, 560 the customary size with B = 3, 720 the limit
# (k = 70: two tiles of outputs).  173 (170) frames in 650 (390) padded rows: off every multiple of 4 and off the chunks of 32 (16)
# padded rows the scatter kernel cuts them into, so chunks begin and end inside utterances and inside padding.
SHAPES = {15: (5, 1, (1, 2, 3, 37, 130), 15), 35: (7, 2, (1, 2, 3, 37, 130), 20), 560: (80, 3, (3, 37, 130), 40),
          720: (80, 4, (1, 2, 3, 37, 130), 70)}


@pytest.fixture(scope="module")
def cases():
    """D_s -> (n_mel, c, lens, xs, ys, P, o, the oracle's (N, s, S), its bounds), computed once"""
    out = {}
    for Ds, (n_mel, c, lens, k) in SHAPES.items():
        rng = np.random.RandomState(Ds)
        scale, shift = 0.5 + rng.rand(2 * n_mel), rng.randn(2 * n_mel)    # no symmetry between channels, sums that do not cancel
        xs = [rng.randn(T, 2 * n_mel) * scale + shift for T in lens]
        ys = [LR.splice(x, n_mel, c) for x in xs]
        assert ys[0].shape[1] == Ds
        out[Ds] = (n_mel, c, list(lens), xs, ys, rng.randn(k, Ds) / np.sqrt(Ds), rng.randn(k), LR.scatter(ys), LR.scatter_bounds(ys))
    return out


@pytest.mark.parametrize("Ds", sorted(SHAPES))
def test_splice_is_bit_equal(dev, cases, Ds):
    n_mel, c, lens, xs, ys, *_ = cases[Ds]
    x = padded(xs, NAN, np.float64, dev)
    Tm = max(lens)
    out = torch.full((len(xs), Tm + 2, Ds + 3), NAN, dtype=torch.float64, device=dev)[:, :Tm, :Ds]      # a strided view
    y = A.splice(x, lens, n_mel, c, out=out)
    assert y.data_ptr() == out.data_ptr()
    y = y.cpu().numpy()
    for b, want in enumerate(ys):
        assert np.array_equal(y[b, :lens[b]], want)
        assert np.isnan(y[b, lens[b]:]).all()                              # padding is never written (and NaN was never read)
    assert torch.equal(A.splice(x[:, :, :n_mel].contiguous(), lens, n_mel, c)[0, :1], out[0, :1])       # the statics alone do


@pytest.mark.parametrize("Ds", sorted(SHAPES))
def test_scatter_against_oracle(dev, cases, Ds):
    n_mel, c, lens, xs, ys, _, _, (N, s_ref, S_ref), (s_bound, S_bound) = cases[Ds]
    assert N == sum(lens) and N % 4 != 0
    y = padded(ys, NAN, np.float64, dev)
    s, S = A.scatter(y, lens)
    sn, Sn = s.cpu().numpy(), S.cpu().numpy()
    print("Ds", Ds, "S err / bound", (np.abs(Sn - S_ref) / S_bound).max(), "s err / bound", (np.abs(sn - s_ref) / s_bound).max())
    assert (np.abs(Sn - S_ref) <= S_bound).all() and (np.abs(sn - s_ref) <= s_bound).all()
    assert np.array_equal(Sn, Sn.T)                                        # exactly symmetric
    s2, S2 = A.scatter(y, lens)
    assert torch.equal(s, s2) and torch.equal(S, S2)                       # two runs: the same bits
    s0, S0 = A.scatter(padded(ys, 0.0, np.float64, dev), lens)
    assert torch.equal(s, s0) and torch.equal(S, S0)                       # what the padding holds changes nothing
    # two batches into one pair of tables against one batch of both, to the same bound
    cut = len(ys) // 2
    sa, Sa = A.scatter(padded(ys[:cut], NAN, np.float64, dev), lens[:cut])
    sb, Sb = A.scatter(padded(ys[cut:], NAN, np.float64, dev), lens[cut:], sa, Sa)
    assert sb.data_ptr() == sa.data_ptr() and Sb.data_ptr() == Sa.data_ptr()
    assert (np.abs(Sb.cpu().numpy() - S_ref) <= S_bound).all() and (np.abs(sb.cpu().numpy() - s_ref) <= s_bound).all()
    assert torch.equal(Sb, Sb.T)


@pytest.mark.parametrize("Ds", sorted(SHAPES))
def test_project_against_oracle(dev, cases, Ds):
    n_mel, c, lens, xs, ys, Pm, o, *_ = cases[Ds]
    k, Tm = Pm.shape[0], max(lens)
    y = padded(ys, NAN, np.float64, dev)
    Pd, od = torch.from_numpy(Pm).to(dev), torch.from_numpy(o).to(dev)
    out = torch.full((len(ys), Tm + 1, k + 2), NAN, dtype=torch.float64, device=dev)[:, :Tm, :k]
    z = A.project(y, lens, Pd, od, out=out)
    assert z.data_ptr() == out.data_ptr()
    zn = z.cpu().numpy()
    for b, yy in enumerate(ys):
        err, bound = np.abs(zn[b, :lens[b]] - LR.project(yy, Pm, o)), LR.project_bound(yy, Pm)
        print("Ds", Ds, "b", b, "z err / bound", (err / bound).max())
        assert (err <= bound).all()
        assert np.isnan(zn[b, lens[b]:]).all()
    z0 = A.project(padded(ys, 0.0, np.float64, dev), lens, Pd, od)
    z1 = A.project(y, lens, Pd, od)
    for b, T in enumerate(lens):
        assert torch.equal(z1[b, :T], out[b, :T]) and torch.equal(z0[b, :T], out[b, :T])                # runs and padding: the same bits


def test_bad_arguments(dev):
    assert A.max_splice_dim() == 720 == _lib.load().fs2_align_max_splice_dim()
    x = torch.zeros(2, 6, 160, dtype=torch.float64, device=dev)
    lens = torch.tensor([6, 4], dtype=torch.int32, device=dev)
    y = torch.zeros(2, 6, 800, dtype=torch.float64, device=dev)
    call = lambda n_mel, c: _lib.call("fs2_align_splice", x.data_ptr(), x.stride(0), x.stride(1), lens.data_ptr(), n_mel, c,    # noqa: E731
                                      y.data_ptr(), y.stride(0), y.stride(1), 2, 6, None)
    for n_mel, c in ((80, 5), (80, -1), (81, 4)):                          # c = 5, D_s = 729: the ABI itself refuses before any launch
        with pytest.raises(ValueError, match="supported"):
            call(n_mel, c)
        with pytest.raises(ValueError):
            A.splice(x, [6, 4], n_mel, c)
    Pm, o = torch.zeros(9, 8, dtype=torch.float64, device=dev), torch.zeros(9, dtype=torch.float64, device=dev)
    z = torch.zeros(2, 6, 9, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="k <= D_s"):                      # k > D_s
        _lib.call("fs2_align_project", y.data_ptr(), y.stride(0), y.stride(1), lens.data_ptr(), Pm.data_ptr(), o.data_ptr(), 9, 8,
                  z.data_ptr(), z.stride(0), z.stride(1), 2, 6, None)
    with pytest.raises(ValueError):
        A.project(y[:, :, :8].contiguous(), [6, 4], Pm, o)
    with pytest.raises(ValueError, match="dimensions"):                    # D_s > 720
        _lib.call("fs2_align_scatter", y.data_ptr(), y.stride(0), y.stride(1), lens.data_ptr(), 721, o.data_ptr(), z.data_ptr(), 721,
                  z.data_ptr(), 1 << 30, 2, 6, None)
    with pytest.raises(ValueError, match="workspace"):                     # a workspace smaller than the query asks for
        S = torch.zeros(8, 8, dtype=torch.float64, device=dev)
        _lib.call("fs2_align_scatter", y.data_ptr(), y.stride(0), y.stride(1), lens.data_ptr(), 8, o.data_ptr(), S.data_ptr(), 8,
                  z.data_ptr(), _lib.load().fs2_align_scatter_ws(2, 6, 8) - 1, 2, 6, None)
    with pytest.raises(ValueError):
        A.scatter(y, [6, 4])                                               # 800 dimensions
    with pytest.raises(ValueError, match="on the GPU"):
        A.scatter(y[:, :, :8].contiguous().cpu(), [6, 4])
    with pytest.raises(ValueError, match="together"):
        A.scatter(y[:, :, :8].contiguous(), [6, 4], s=torch.zeros(8, dtype=torch.float64, device=dev))
    for kw in ({"lda": 241, "splice": 1}, {"lda": 8, "splice": 5}, {"lda": -1}):
        with pytest.raises(ValueError):
            A.Aligner(28, 160, 2, dev, **kw)
    with pytest.raises(ValueError):
        A.Aligner(28, 162, 2, dev, lda=8, splice=4)                        # 81 channels x 9 frames


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.fixture(scope="module")
def corpus_run(dev):
    lex, utts = LC.corpus(E2E_SEED, E2E_N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    n_classes = len(ids) * C.STATES
    frames = [len(x) for x in xs]
    Ds = A.splice_dim(C.N_MEL, E2E_SPLICE, E2E_K)
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, 16 << 20, splice_dim=Ds):
        mel = padded([utts[i]["mel"].T for i in batch], NAN, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        feats = A.features(mel, lens)
        for r, n in enumerate(lens):
            feats[r, n:] = NAN                                             # rows beyond an utterance must never be read
        batches.append((feats, lens, [graphs[i] for i in batch], batch))
    assert len(batches) >= 3

    def run(**kw):
        al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev, **kw)
        hist = al.fit([b[:3] for b in batches], E2E_ITERS)
        got = [None] * len(utts)
        for feats, lens, gs, batch in batches:
            for i, fr in zip(batch, al.align(feats, lens, gs)):
                got[i] = fr
        return al, hist, got
    return utts, graphs, xs, n_classes, run


def test_fit_and_align_against_the_oracle_schedule(corpus_run):
    """tests/test_align_lda_cpu.py shows that, for this seed, the oracle's alignment does not move when P is perturbed by 1e-12
    relative noise (and its log-likelihoods move by far less than 1e-9), so frames can be compared exactly."""
    utts, graphs, xs, n_classes, run = corpus_run
    kw = dict(lda=E2E_K, splice=E2E_SPLICE, lda_iters=E2E_LDA_ITERS)
    al, hist, got = run(**kw)
    want = LR.fit(xs, graphs, n_classes, E2E_ITERS, C.N_MEL, E2E_K, E2E_SPLICE, E2E_LDA_ITERS)
    print("loglik per frame", hist, want["history"])
    assert len(hist) == E2E_ITERS + 1 + E2E_LDA_ITERS == len(want["history"])
    rel = np.abs(np.array(hist) - np.array(want["history"])) / np.abs(np.array(want["history"]))
    print("relative difference per pass", rel, "eigenvalues", want["eig"])
    assert (rel <= 1e-9).all()
    assert al.mu.shape == (n_classes, E2E_K) and tuple(al.P.shape) == (E2E_K, C.N_MEL * (2 * E2E_SPLICE + 1))
    frames = [LR.align(x, g, want) for x, g in zip(xs, graphs)]
    differ = [i for i, (a, b) in enumerate(zip(got, frames)) if not np.array_equal(a, b)]
    assert not differ, differ
    true = [[d for _, d in u["segments"]] for u in utts]
    print("accuracy within one frame", C.accuracy(true, got, 1))
    al2, hist2, got2 = run(**kw)                                           # two runs: the same bits
    assert hist == hist2 and all(np.array_equal(a, b) for a, b in zip(got, got2))
    assert torch.equal(al.P, al2.P) and torch.equal(al.o, al2.o) and torch.equal(al.mu, al2.mu) and torch.equal(al.var, al2.var)


def test_lda_zero_is_the_aligner_without_the_new_arguments(corpus_run):
    _, _, _, _, run = corpus_run
    old, hist_old, got_old = run()
    new, hist_new, got_new = run(lda=0, splice=2, lda_iters=7)
    assert hist_old == hist_new and len(hist_old) == E2E_ITERS
    assert torch.equal(old.mu, new.mu) and torch.equal(old.var, new.var) and new.P is None
    assert all(np.array_equal(a, b) for a, b in zip(got_old, got_new))


def test_command_line_lda(dev, tmp_path):
    """`align.py cfg --lda 8 --splice 1` writes a TextGrid per utterance that the preprocessor's reader takes; a second run writes
    the same bytes."""
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 99, 8)
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(config(root, lexicon_path), f)
    cmd = [sys.executable, os.path.join(ROOT, "align.py"), os.path.join(root, "preprocess.yaml"), "--overwrite", "--lda", "8", "--splice", "1"]
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    files = []
    for _ in range(2):
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "8 TextGrids written, 0 utterances skipped" in run.stdout, run.stdout
        assert "lda: eigenvalues" in run.stdout and len(run.stdout.split("lda: eigenvalues ")[1].splitlines()[0].split()) == 8
        assert len(run.stdout.split("log-likelihood per frame: ")[1].splitlines()[0].split()) == 12 + 1 + 4
        files.append({name: open(tg(name), "rb").read() for name in truth})
    assert files[0] == files[1]
    for name, segs in truth.items():
        iv = P.read_textgrid(tg(name))["phones"]
        assert iv[0][0] == 0.0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
        assert int(round(iv[-1][1] * C.SR / C.HOP)) == sum(d for _, d in segs) + 1
        assert [p for _, _, p in iv if p not in P.SIL_PHONES] == [p for p, _ in segs if p not in P.SIL_PHONES]
