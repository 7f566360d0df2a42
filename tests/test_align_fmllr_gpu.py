"""GPU: the forced aligner's fMLLR stage (fastspeech2_amd.align fmllr_weights / fmllr_accumulate / fmllr_apply / Aligner(fmllr=1),
csrc/fs2_align_fmllr.hip) against the numpy oracle tests/align_fmllr_ref.py: the three kernels elementwise on ragged batches with
NaN padding, at D + 1 under one 16-tile, exactly a tile, one past, at the customary 40 and at the limit of 64; the whole schedule
and decoding on the multi-speaker corpus of tests/align_fmllr_corpus.py; the untouched default; the command line."""
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
from tests import align_fmllr_ref as FR
from tests.test_align_cpu import config
from tests.test_align_fmllr_cpu import (E2E_FMLLR_ITERS, E2E_ITERS, E2E_K, E2E_LDA_ITERS, E2E_MIN_FRAMES, E2E_ROUNDS, E2E_SPLICE,
                                        E2E_SWEEPS, e2e)
from tests.test_align_gpu import NAN, ROOT, padded

pytestmark = pytest.mark.gpu
# 173 frames in 650 padded rows: the accumulation cuts a speaker's padded rows into chunks of 32.  Speaker 0 owns the rows 0, 2 and 4
# (not adjacent, one of a single frame, chunk boundaries inside the last one), speakers 1 and 2 one row each, speaker 3 none.
LENS, SPEAKERS, N_SPK, N_CLASSES = (1, 2, 3, 37, 130), (0, 1, 0, 2, 0), 4, 7
DIMS, JS = (3, 15, 16, 40, 64), (5, 37)


def fake_graph(sid):
    """what `Graphs` and the weights kernel read of a graph: the emission classes of J states"""
    J = len(sid)
    return {"sid": np.asarray(sid, np.int32), "skip": np.full(J, -1, np.int32), "block": np.zeros(J, np.int32), "alt": (-1, -1),
            "blocks": [("X", 0, False)], "mandatory": J}


@pytest.fixture(scope="module")
def cases():
    """(D, J) -> dict of the inputs, the oracle's outputs and their bounds, computed once"""
    out = {}
    for D in DIMS:
        for J in JS:
            rng = np.random.RandomState(1000 * D + J)
            jl = [J, max(J - 3, 1), J, 2, max(J - 1, 1)]                    # ragged in j as well
            graphs = [fake_graph(rng.randint(0, N_CLASSES, n)) for n in jl]
            mu, var = rng.randn(N_CLASSES, D), 0.5 + rng.rand(N_CLASSES, D)
            scale, shift = 0.5 + rng.rand(D), rng.randn(D)                 # no symmetry between dimensions, sums that do not cancel
            fs = [rng.randn(T, D) * scale + shift for T in LENS]
            gammas = []
            for T, n in zip(LENS, jl):
                g = rng.dirichlet(0.5 * np.ones(n), T)
                g[rng.rand(T, n) < 0.2] = 0.0                              # exact zeros, as the backward pass leaves them
                gammas.append(g)
            ch = [FR.weights(g, gr["sid"], mu, var) for g, gr in zip(gammas, graphs)]
            chb = [FR.weights_bounds(g, gr["sid"], mu, var) for g, gr in zip(gammas, graphs)]
            cs, hs, cbs, hbs = [v[0] for v in ch], [v[1] for v in ch], [v[0] for v in chb], [v[1] for v in chb]
            W = np.eye(D, D + 1)[None] + 0.3 * rng.randn(N_SPK, D, D + 1)
            out[(D, J)] = dict(graphs=graphs, jl=jl, mu=mu, var=var, fs=fs, gammas=gammas, cs=cs, hs=hs, cbs=cbs, hbs=hbs, W=W,
                               stats=FR.accumulate(fs, cs, hs, SPEAKERS, N_SPK),
                               bounds=FR.accumulate_bounds(fs, cs, hs, SPEAKERS, N_SPK, cbs, hbs))
    return out


def weights_on_device(case, dev, fill):
    G = A.Graphs(case["graphs"], dev)
    gamma = padded(case["gammas"], fill, np.float64, dev)
    D, Tm = case["mu"].shape[1], max(LENS)
    c = torch.full((len(LENS), Tm + 2, D + 3), NAN, dtype=torch.float64, device=dev)[:, :Tm, :D]       # strided views
    h = torch.full((len(LENS), Tm + 2, D + 3), NAN, dtype=torch.float64, device=dev)[:, :Tm, :D]
    got = A.fmllr_weights(gamma, list(LENS), G, torch.from_numpy(case["mu"]).to(dev), torch.from_numpy(case["var"]).to(dev), out=(c, h))
    assert got[0].data_ptr() == c.data_ptr() and got[1].data_ptr() == h.data_ptr()
    return c, h


@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("D", DIMS)
def test_weights_against_oracle(dev, cases, D, J):
    case = cases[(D, J)]
    c, h = weights_on_device(case, dev, NAN)
    cn, hn = c.cpu().numpy(), h.cpu().numpy()
    for b, T in enumerate(LENS):
        for got, want, bound, name in ((cn, case["cs"], case["cbs"], "c"), (hn, case["hs"], case["hbs"], "h")):
            err = np.abs(got[b, :T] - want[b])
            print("D", D, "J", J, "b", b, name, "err / bound", (err[bound[b] > 0] / bound[b][bound[b] > 0]).max(initial=0.0))
            assert (err <= bound[b]).all()
            assert np.isnan(got[b, T:]).all()                              # padding is never written (and NaN was never read)
    c2, h2 = weights_on_device(case, dev, NAN)
    c0, h0 = weights_on_device(case, dev, 0.0)
    for b, T in enumerate(LENS):                                           # runs and padding: the same bits
        assert torch.equal(c[b, :T], c2[b, :T]) and torch.equal(h[b, :T], h2[b, :T])
        assert torch.equal(c[b, :T], c0[b, :T]) and torch.equal(h[b, :T], h0[b, :T])


@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("D", DIMS)
def test_accumulate_against_oracle(dev, cases, D, J):
    """The kernel's own c and h go in, the oracle's statistics come from the oracle's c and h: the bound carries the bounds of c
    and h through the sums."""
    case = cases[(D, J)]
    lens = list(LENS)
    c, h = weights_on_device(case, dev, NAN)                               # their padding is NaN
    f = padded(case["fs"], NAN, np.float64, dev)
    beta, G, k = A.fmllr_accumulate(f, c, h, lens, SPEAKERS, N_SPK)
    (beta_ref, G_ref, k_ref), (G_bound, k_bound) = case["stats"], case["bounds"]
    bn, Gn, kn = beta.cpu().numpy(), G.cpu().numpy(), k.cpu().numpy()
    assert np.array_equal(bn, beta_ref) and list(bn) == [134.0, 2.0, 37.0, 0.0]                         # the frame counts, exactly
    present = [0, 1, 2]
    print("D", D, "J", J, "G err / bound", (np.abs(Gn - G_ref)[present] / G_bound[present]).max(), "k err / bound",
          (np.abs(kn - k_ref)[present] / k_bound[present]).max())
    assert (np.abs(Gn - G_ref) <= G_bound).all() and (np.abs(kn - k_ref) <= k_bound).all()
    assert np.array_equal(Gn, Gn.transpose(0, 1, 3, 2))                    # exactly symmetric
    assert not Gn[3].any() and not kn[3].any()
    beta2, G2, k2 = A.fmllr_accumulate(f, c, h, lens, SPEAKERS, N_SPK)
    assert torch.equal(beta, beta2) and torch.equal(G, G2) and torch.equal(k, k2)                       # two runs: the same bits
    zero = lambda t: torch.where(torch.isnan(t), torch.zeros_like(t), t)   # noqa: E731
    beta0, G0, k0 = A.fmllr_accumulate(zero(f), zero(c), zero(h), lens, SPEAKERS, N_SPK)
    assert torch.equal(beta, beta0) and torch.equal(G, G0) and torch.equal(k, k0)                       # what the padding holds changes nothing
    # pre-filled tables: the absent speaker's are bit-unchanged, the others have moved
    rng = np.random.RandomState(3)
    pre = [torch.from_numpy(rng.randn(*t.shape)).to(dev) for t in (beta, G, k)]
    got = A.fmllr_accumulate(f, c, h, lens, SPEAKERS, N_SPK, *[t.clone() for t in pre])
    for t, p in zip(got, pre):
        assert torch.equal(t[3], p[3]) and not torch.equal(t[0], p[0]) and not torch.equal(t[2], p[2])
    # two half-batches into one set of tables against one batch of both, to the same bound
    cut = 2
    half = lambda a, b: (padded(case["fs"][a:b], NAN, np.float64, dev), c[a:b, :max(LENS[a:b])].contiguous(),    # noqa: E731
                         h[a:b, :max(LENS[a:b])].contiguous(), lens[a:b], SPEAKERS[a:b], N_SPK)
    ta = A.fmllr_accumulate(*half(0, cut))
    tb = A.fmllr_accumulate(*half(cut, len(lens)), *ta)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(ta, tb))
    assert np.array_equal(tb[0].cpu().numpy(), beta_ref)
    assert (np.abs(tb[1].cpu().numpy() - G_ref) <= G_bound).all() and (np.abs(tb[2].cpu().numpy() - k_ref) <= k_bound).all()
    assert torch.equal(tb[1], tb[1].transpose(2, 3))


@pytest.mark.parametrize("D", DIMS)
def test_apply_against_oracle(dev, cases, D):
    case = cases[(D, JS[0])]
    lens, Tm, W = list(LENS), max(LENS), case["W"]
    f = padded(case["fs"], NAN, np.float64, dev)
    Wd = torch.from_numpy(W).to(dev)
    out = torch.full((len(lens), Tm + 1, D + 2), NAN, dtype=torch.float64, device=dev)[:, :Tm, :D]
    fh = A.fmllr_apply(f, lens, Wd, SPEAKERS, out=out)
    assert fh.data_ptr() == out.data_ptr()
    fn = fh.cpu().numpy()
    for b, (ff, s) in enumerate(zip(case["fs"], SPEAKERS)):
        err, bound = np.abs(fn[b, :lens[b]] - FR.apply(ff, W[s])), FR.apply_bound(ff, W[s])
        print("D", D, "b", b, "fh err / bound", (err / bound).max())
        assert (err <= bound).all()
        assert np.isnan(fn[b, lens[b]:]).all()
    f1 = A.fmllr_apply(f, lens, Wd, SPEAKERS)
    f0 = A.fmllr_apply(padded(case["fs"], 0.0, np.float64, dev), lens, Wd, SPEAKERS)
    for b, T in enumerate(lens):
        assert torch.equal(f1[b, :T], out[b, :T]) and torch.equal(f0[b, :T], out[b, :T])                # runs and padding: the same bits
    eye = torch.from_numpy(np.tile(np.eye(D, D + 1), (N_SPK, 1, 1))).to(dev)
    same = A.fmllr_apply(f, lens, eye, SPEAKERS)
    for b, T in enumerate(lens):
        assert torch.equal(same[b, :T], f[b, :T])                          # [I | 0] changes nothing


def test_bad_arguments(dev):
    assert A.max_fmllr_dim() == 64 == _lib.load().fs2_align_max_fmllr_dim()
    lens = [6, 4]
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)            # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)                     # noqa: E731
    graphs = [fake_graph([0, 1, 2]), fake_graph([1, 2])]
    G = A.Graphs(graphs, dev)

    offs, rows, beta, Gt, kt, ws = i32([0, 1, 2]), i32([0, 1]), z(2), z(2, 8, 9, 9), z(2, 8, 9), z(1 << 16)

    def accum(D, ws_doubles):
        f, c = z(2, 6, max(D, 1)), z(2, 6, max(D, 1))
        _lib.call("fs2_align_fmllr_accum", f.data_ptr(), f.stride(0), f.stride(1), c.data_ptr(), c.data_ptr(), c.stride(0), c.stride(1),
                  lens_d.data_ptr(), offs.data_ptr(), rows.data_ptr(), 2, D, beta.data_ptr(), Gt.data_ptr(), kt.data_ptr(), ws.data_ptr(),
                  ws_doubles, 2, 6, None)
        torch.cuda.synchronize()
    for D in (0, 65):                                                      # the ABI itself refuses before any launch
        with pytest.raises(ValueError, match="supported"):
            accum(D, 1 << 16)
        f, spk = z(2, 6, max(D, 1)), i32([0, 1])
        with pytest.raises(ValueError, match="supported"):
            _lib.call("fs2_align_fmllr_apply", f.data_ptr(), f.stride(0), f.stride(1), lens_d.data_ptr(), f.data_ptr(), spk.data_ptr(), 2, D,
                      f.data_ptr(), f.stride(0), f.stride(1), 2, 6, None)
        with pytest.raises(ValueError, match="supported"):
            _lib.call("fs2_align_fmllr_weights", f.data_ptr(), f.stride(0), f.stride(1), lens_d.data_ptr(), G.jlens.data_ptr(),
                      G.sid.data_ptr(), G.ldg, f.data_ptr(), f.data_ptr(), 3, D, f.data_ptr(), f.data_ptr(), f.stride(0), f.stride(1), 2, 6,
                      0, None)
        assert _lib.load().fs2_align_fmllr_accum_ws(2, 6, D) == 0
    need = _lib.load().fs2_align_fmllr_accum_ws(2, 6, 8)
    assert 0 < need <= 1 << 16
    with pytest.raises(ValueError, match="workspace"):                     # a workspace smaller than the query asks for
        accum(8, need - 1)
    accum(8, need)
    assert beta.tolist() == [6.0, 4.0]
    f65, f8 = z(2, 6, 65), z(2, 6, 8)
    with pytest.raises(ValueError):
        A.fmllr_apply(f65, lens, z(2, 65, 66), [0, 1])
    with pytest.raises(ValueError):
        A.fmllr_accumulate(f65, f65, f65, lens, [0, 1], 2)
    with pytest.raises(ValueError):
        A.fmllr_weights(z(2, 6, 3), lens, G, z(3, 65), z(3, 65) + 1)
    with pytest.raises(ValueError, match="on the GPU"):                    # host tensors
        A.fmllr_accumulate(f8.cpu(), f8, f8, lens, [0, 1], 2)
    with pytest.raises(ValueError, match="on the GPU"):
        A.fmllr_apply(f8, lens, z(2, 8, 9).cpu(), [0, 1])
    with pytest.raises(ValueError, match="on the GPU"):
        A.fmllr_weights(z(2, 6, 3).cpu(), lens, G, z(3, 8), z(3, 8) + 1)
    for spk in ([0, 2], [-1, 0], [0], None):                               # a speaker index out of range, a list of the wrong length
        with pytest.raises(ValueError, match="speaker"):
            A.fmllr_accumulate(f8, f8, f8, lens, spk, 2)
        with pytest.raises(ValueError, match="speaker"):
            A.fmllr_apply(f8, lens, z(2, 8, 9), spk)
    with pytest.raises(ValueError, match="together"):
        A.fmllr_accumulate(f8, f8, f8, lens, [0, 1], 2, beta=z(2))
    with pytest.raises(ValueError, match="--lda k with k <= 64"):
        A.Aligner(28, 160, 2, dev, fmllr=1)                                # D = 160 without lda
    with pytest.raises(ValueError):
        A.Aligner(28, 160, 2, dev, lda=65, splice=1, fmllr=1)
    with pytest.raises(ValueError):
        A.Aligner(28, 160, 2, dev, lda=8, splice=1, fmllr=1, fmllr_rounds=0)
    al = A.Aligner(28, 160, 2, dev, lda=8, splice=1, fmllr=1)
    with pytest.raises(ValueError, match="speakers"):
        al.fit([(z(2, 6, 160), lens, graphs)], 1)                          # fit without speakers
    with pytest.raises(ValueError, match="speaker"):
        al.fit([(z(2, 6, 160), lens, graphs)], 1, speakers=[[0, -1]])
    with pytest.raises(ValueError, match="fit"):
        al.align(z(2, 6, 160), lens, graphs, [0, 1])                       # no transforms yet


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.fixture(scope="module")
def corpus_run(dev):
    utts, graphs, xs, spk, n_classes, model = e2e()
    frames = [len(x) for x in xs]
    Ds = A.splice_dim(C.N_MEL, E2E_SPLICE, E2E_K)
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, 16 << 20, splice_dim=Ds, fmllr_dim=E2E_K):
        mel = padded([utts[i]["mel"].T for i in batch], NAN, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        feats = A.features(mel, lens)
        for r, n in enumerate(lens):
            feats[r, n:] = NAN                                             # rows beyond an utterance must never be read
        batches.append((feats, lens, [graphs[i] for i in batch], batch))
    assert len(batches) >= 3
    speakers = [[spk[i] for i in b[3]] for b in batches]

    def run(**kw):
        al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev, **kw)
        hist = al.fit([b[:3] for b in batches], E2E_ITERS, speakers if kw.get("fmllr") else None)
        got = [None] * len(utts)
        for (feats, lens, gs, batch), sp in zip(batches, speakers):
            for i, fr in zip(batch, al.align(feats, lens, gs, sp if kw.get("fmllr") else None)):
                got[i] = fr
        return al, hist, got
    return utts, graphs, xs, spk, n_classes, model, run


KW = dict(lda=E2E_K, splice=E2E_SPLICE, lda_iters=E2E_LDA_ITERS, fmllr=1, fmllr_rounds=E2E_ROUNDS, fmllr_iters=E2E_FMLLR_ITERS,
          fmllr_sweeps=E2E_SWEEPS, fmllr_min_frames=E2E_MIN_FRAMES)


def compare(al, hist, got, want, xs, graphs, spk, n_passes):
    print("loglik per frame", hist, want["history"])
    assert len(hist) == n_passes == len(want["history"])
    rel = np.abs(np.array(hist) - np.array(want["history"])) / np.abs(np.array(want["history"]))
    print("relative difference per pass", rel)
    assert (rel <= 1e-9).all()
    W = al.W.cpu().numpy()
    relW = [np.abs(W[s] - want["W"][s]).max() / np.abs(want["W"][s]).max() for s in range(len(W))]
    print("relative difference of W per speaker", relW)
    assert W.shape == want["W"].shape and max(relW) <= 1e-9
    frames = [FR.align(x, g, want, s) for x, g, s in zip(xs, graphs, spk)]
    differ = [i for i, (a, b) in enumerate(zip(got, frames)) if not np.array_equal(a, b)]
    assert not differ, differ


def test_fit_and_align_against_the_oracle_schedule(corpus_run):
    """tests/test_align_fmllr_cpu.py shows that, for this seed, the oracle's alignment does not move when every W is perturbed by
    1e-12 relative noise (and its log-likelihoods move by far less than 1e-9), so frames can be compared exactly."""
    utts, graphs, xs, spk, n_classes, want, run = corpus_run
    al, hist, got = run(**KW)
    compare(al, hist, got, want, xs, graphs, spk, E2E_ITERS + 1 + E2E_LDA_ITERS + E2E_ROUNDS * (1 + E2E_FMLLR_ITERS))
    assert np.array_equal(al.W[4].cpu().numpy(), np.eye(E2E_K, E2E_K + 1))                              # the short speaker keeps [I | 0]
    for p in want["stat_passes"]:
        assert hist[p + 1] >= hist[p]                                      # no drop from a statistics pass to the pass after its update
    true = [[d for _, d in u["segments"]] for u in utts]
    print("accuracy within one frame", C.accuracy(true, got, 1))
    al2, hist2, got2 = run(**KW)                                           # two runs: the same bits
    assert hist == hist2 and all(np.array_equal(a, b) for a, b in zip(got, got2))
    assert torch.equal(al.W, al2.W) and torch.equal(al.mu, al2.mu) and torch.equal(al.var, al2.var)
    one = torch.zeros(1, len(xs[0]), 2 * C.N_MEL, dtype=torch.float64, device=al.device)
    for bad in (None, [5], [-1]):                                          # no speakers, a speaker `fit` has not seen
        with pytest.raises(ValueError, match="speaker"):
            al.align(one, [len(xs[0])], graphs[:1], bad)


def test_mixtures_on_top_of_the_adapted_features(corpus_run):
    utts, graphs, xs, spk, n_classes, base, run = corpus_run
    want = FR.fit(xs, graphs, spk, n_classes, E2E_ITERS, C.N_MEL, E2E_K, E2E_SPLICE, E2E_LDA_ITERS, E2E_ROUNDS, E2E_FMLLR_ITERS,
                  E2E_SWEEPS, E2E_MIN_FRAMES, mixtures=2, mix_iters=2, start=base)
    al, hist, got = run(mixtures=2, mix_iters=2, **KW)
    compare(al, hist, got, want, xs, graphs, spk, E2E_ITERS + 1 + E2E_LDA_ITERS + E2E_ROUNDS * (1 + E2E_FMLLR_ITERS) + 2)
    assert np.array_equal(al.ncomp, want["ncomp"]) and al.ncomp.max() == 2
    al2, hist2, got2 = run(mixtures=2, mix_iters=2, **KW)
    assert hist == hist2 and all(np.array_equal(a, b) for a, b in zip(got, got2)) and torch.equal(al.gmu, al2.gmu)


def test_fmllr_zero_is_the_aligner_without_the_new_arguments(corpus_run):
    *_, run = corpus_run
    kw = dict(lda=E2E_K, splice=E2E_SPLICE, lda_iters=E2E_LDA_ITERS)
    old, hist_old, got_old = run(**kw)
    new, hist_new, got_new = run(fmllr=0, fmllr_rounds=7, fmllr_iters=5, fmllr_sweeps=3, fmllr_min_frames=11, **kw)
    assert hist_old == hist_new and len(hist_old) == E2E_ITERS + 1 + E2E_LDA_ITERS
    assert torch.equal(old.mu, new.mu) and torch.equal(old.var, new.var) and new.W is None
    assert all(np.array_equal(a, b) for a, b in zip(got_old, got_new))


def test_command_line_fmllr(dev, tmp_path):
    """`align.py cfg --lda 8 --splice 1 --fmllr 1` over two speaker directories writes a TextGrid per utterance that the
    preprocessor's reader takes; a second run writes the same bytes."""
    root = str(tmp_path)
    lexicon_path, truth_a = C.wav_corpus(root, 99, 8, speaker="spka")
    _, truth_b = C.wav_corpus(root, 99, 6, speaker="spkb")                 # the same seed: the same lexicon file
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(config(root, lexicon_path), f)
    cmd = [sys.executable, os.path.join(ROOT, "align.py"), os.path.join(root, "preprocess.yaml"), "--overwrite", "--lda", "8", "--splice", "1",
           "--fmllr", "1", "--fmllr_min_frames", "100"]
    tg = lambda spk, name: os.path.join(root, "pre", "TextGrid", spk, name + ".TextGrid")          # noqa: E731
    names = [("spka", n) for n in truth_a] + [("spkb", n) for n in truth_b]
    files = []
    for _ in range(2):
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "14 TextGrids written, 0 utterances skipped" in run.stdout, run.stdout
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("fmllr: round")]
        assert len(lines) == 2 and all("2 speakers adapted, 0 kept (too few frames), 0 kept (not positive definite)" in ln for ln in lines), lines
        assert len(run.stdout.split("log-likelihood per frame: ")[1].splitlines()[0].split()) == 12 + 1 + 4 + 2 * (1 + 2)
        files.append({n: open(tg(*n), "rb").read() for n in names})
    assert files[0] == files[1]
    for spk, truth in (("spka", truth_a), ("spkb", truth_b)):
        for name, segs in truth.items():
            iv = P.read_textgrid(tg(spk, name))["phones"]
            assert iv[0][0] == 0.0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
            assert int(round(iv[-1][1] * C.SR / C.HOP)) == sum(d for _, d in segs) + 1
            assert [p for _, _, p in iv if p not in P.SIL_PHONES] == [p for p, _ in segs if p not in P.SIL_PHONES]
