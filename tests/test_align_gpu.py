"""GPU forced aligner (fastspeech2_amd.align, csrc/fs2_align.hip) against the numpy oracle tests/align_ref.py: every kernel on ragged
batches whose padding is NaN, the recursions fed the oracle's own emissions, training and decoding on the synthetic corpus of
tests/align_corpus.py, run-to-run determinism, and align.py -> preprocess end to end on a corpus of tone sequences."""
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
from tests.test_align_cpu import ITERS, N_UTT, SEED, config

pytestmark = pytest.mark.gpu
RTOL = 1e-6                                                                # the project's bar for fp64 kernels (tests/test_f0_gpu.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def single_block_graph(cls, states):
    """one mandatory block and nothing else: the smallest graph the kernels can be given"""
    return {"sid": np.arange(cls * states, (cls + 1) * states, dtype=np.int32), "skip": np.full(states, -1, np.int32),
            "block": np.zeros(states, np.int32), "alt": (-1, -1), "blocks": [("X", 0, False)], "mandatory": states}


def rel_close(got, want, rtol=RTOL):
    got, want = np.asarray(got), np.asarray(want)
    bad = ~(np.abs(got - want) <= rtol * np.abs(want))
    assert not bad.any(), (np.nonzero(bad), got[bad][:4], want[bad][:4])


def padded(arrays, fill, dtype, dev, width=None):
    """[(T_b, W_b)] -> (B, Tmax, Wmax) device tensor, everything outside the arrays = fill"""
    T = max(a.shape[0] for a in arrays)
    W = width or max(a.shape[1] for a in arrays)
    out = np.full((len(arrays), T, W), fill, dtype)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(out).to(dev)


@pytest.fixture(scope="module")
def ragged():
    """Seven utterances: four of the synthetic corpus, a single block, T equal to the mandatory states, J at the supported maximum.
    Class tables: the oracle's flat-start estimate (soft posteriors: many paths matter)."""
    lex, utts = C.corpus(SEED, 12)
    ids = A.phone_table(lex)
    S = C.STATES
    n_classes = len(ids) * S
    graphs = [A.utterance_graph(u["words"], lex, ids, S) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    mu, var, _ = R.fit(xs, graphs, n_classes, 0)
    rng = np.random.RandomState(7)
    graphs, xs = graphs[:4], xs[:4]
    graphs.append(single_block_graph(3, S))
    xs.append(rng.randn(9, 2 * C.N_MEL))
    words = sorted(lex)[:5]
    graphs.append(A.utterance_graph(words, lex, ids, S))
    xs.append(rng.randn(graphs[-1]["mandatory"], 2 * C.N_MEL))             # exactly one path
    one = [w for w in sorted(lex) if len(lex[w]) == 2][0]
    g = A.utterance_graph([one] * 170, lex, ids, S)                        # 2 + 340 + 169 = 511 blocks
    extra = {"sid": np.array([ids["spn"] * S, ids["spn"] * S + 1], np.int32), "skip": np.array([509 * S + S - 1, -1], np.int32),
             "block": np.array([511, 511], np.int32)}
    g = {"sid": np.concatenate([g["sid"], extra["sid"]]), "skip": np.concatenate([g["skip"], extra["skip"]]),
         "block": np.concatenate([g["block"], extra["block"]]), "alt": (g["alt"][0], -1), "blocks": g["blocks"] + [("spn", 170, False)],
         "mandatory": g["mandatory"] + S}                                  # one more word after an inner sil: 1024 states
    assert len(g["sid"]) == A.max_states() == 1024
    graphs.append(g)
    xs.append(rng.randn(g["mandatory"] + 40, 2 * C.N_MEL))
    lens = [len(x) for x in xs]
    Es = [R.emissions(x, g["sid"], mu, var) for x, g in zip(xs, graphs)]
    return graphs, xs, lens, mu, var, Es, n_classes


def test_emit_against_oracle(dev, ragged):
    graphs, xs, lens, mu, var, Es, _ = ragged
    G = A.Graphs(graphs, dev)
    x = padded(xs, NAN, np.float64, dev)
    out = torch.full((len(xs), max(lens) + 3, G.Jmax), NAN, dtype=torch.float64, device=dev)[:, :max(lens)]   # a strided view
    E = A.emit(x, lens, G, torch.from_numpy(mu).to(dev), torch.from_numpy(var).to(dev), out=out).cpu().numpy()
    for b, want in enumerate(Es):
        rel_close(E[b, :lens[b], :G.jl[b]], want)
        assert np.isnan(E[b, lens[b]:]).all() and np.isnan(E[b, :, G.jl[b]:]).all()          # padding is never written


def test_features_against_oracle(dev):
    rng = np.random.RandomState(2)
    mels = [rng.randn(C.N_MEL, T).astype(np.float32) * 2 - 5 for T in (57, 1, 300, 2)]
    lens = [m.shape[1] for m in mels]
    mel = padded([m.T for m in mels], NAN, np.float32, dev).transpose(1, 2).contiguous()
    x = A.features(mel, lens).cpu().numpy()
    for b, m in enumerate(mels):
        assert np.abs(x[b, :lens[b]] - R.features(m)).max() <= 1e-12


def test_forward_backward_stats_reduce_on_the_oracles_emissions(dev, ragged):
    graphs, xs, lens, mu, var, Es, n_classes = ragged
    G = A.Graphs(graphs, dev)
    E = padded(Es, NAN, np.float64, dev)
    x = padded(xs, NAN, np.float64, dev)
    alpha = torch.full_like(E, NAN)
    _, loglik = A.forward(E, lens, G, out=alpha)
    want = [R.posteriors(e, g) for e, g in zip(Es, graphs)]
    rel_close(loglik.cpu().numpy(), [w[2] for w in want])
    a = alpha.cpu().numpy()
    for b, (_, wa, _) in enumerate(want):
        fin = np.isfinite(wa)
        got = a[b, :lens[b], :G.jl[b]]
        assert np.array_equal(np.isneginf(got), np.isneginf(wa))
        rel_close(got[fin], wa[fin])
    gamma = A.backward(E, lens, G, alpha, loglik)                          # written over alpha
    assert gamma.data_ptr() == alpha.data_ptr()
    gm = gamma.cpu().numpy()
    for b, (wg, _, _) in enumerate(want):
        assert np.abs(gm[b, :lens[b], :G.jl[b]] - wg).max() <= 1e-6
        assert np.isnan(gm[b, lens[b]:]).all() and np.isnan(gm[b, :, G.jl[b]:]).all()
    own = A.backward(E, lens, G, A.forward(E, lens, G)[0], loglik, out=torch.full_like(E, NAN))
    assert torch.equal(torch.nan_to_num(own, nan=-1.0), torch.nan_to_num(gamma, nan=-1.0))   # its own buffer: the same values

    parts = torch.full((len(xs), G.Jmax, 1 + 2 * x.shape[2]), NAN, dtype=torch.float64, device=dev)
    A.stats(gamma, x, lens, G, out=parts)
    pw = [R.partials(w[0], xx) for w, xx in zip(want, xs)]
    p = parts.cpu().numpy()
    for b in range(len(xs)):
        assert np.abs(p[b, :G.jl[b]] - pw[b]).max() <= 1e-6 * max(1.0, np.abs(pw[b]).max())
        assert np.isnan(p[b, G.jl[b]:]).all()
    # the reduction alone, on the oracle's partial sums, then the chain
    sums = A.reduce(padded(pw, NAN, np.float64, dev), G, n_classes).cpu().numpy()
    rel_close(sums, R.class_sums(pw, graphs, n_classes))
    twice = A.reduce(parts, G, n_classes, sums=A.reduce(parts, G, n_classes)).cpu().numpy()
    once = A.reduce(parts, G, n_classes).cpu().numpy()
    assert np.abs(twice - 2 * once).max() <= 1e-12 * np.abs(once).max()      # accumulation onto given sums (another order of adds)
    rel_close(once, R.class_sums(pw, graphs, n_classes))


def test_viterbi_and_backtrack_are_exact(dev, ragged):
    graphs, xs, lens, mu, var, Es, _ = ragged
    graphs, Es, lens = list(graphs), list(Es), list(lens)
    lex = {"a": ["X"], "bc": ["Y", "Z"]}
    rng = np.random.RandomState(5)
    for words, T in ((["a", "a"], 7), (["bc", "a", "bc"], 19), (["a"], 4)):   # small-integer emissions: exact ties everywhere
        graphs.append(A.utterance_graph(words, lex, A.phone_table(lex), 1))
        Es.append(rng.randint(-2, 1, (T, len(graphs[-1]["sid"]))).astype(np.float64))
        lens.append(T)
    graphs.append(A.utterance_graph(["a", "a"], lex, A.phone_table(lex), 2))
    Es.append(np.zeros((12, len(graphs[-1]["sid"]))))                      # every path ties: the rule alone decides
    lens.append(12)
    G = A.Graphs(graphs, dev)
    E = padded(Es, NAN, np.float64, dev)
    bp, end, score = A.viterbi(E, lens, G, out=torch.full(E.shape, 77, dtype=torch.uint8, device=dev))
    frames = A.backtrack(bp, lens, G, end).cpu().numpy()
    bp, end = bp.cpu().numpy(), end.cpu().numpy()
    ties = 0
    for b, (e, g) in enumerate(zip(Es, graphs)):
        wbp, wend, wframes = R.viterbi(e, g)
        assert np.array_equal(bp[b, :lens[b], :G.jl[b]], wbp), b
        assert (bp[b, lens[b]:] == 77).all() and (bp[b, :, G.jl[b]:] == 77).all()
        assert end[b] == wend, b
        assert np.array_equal(frames[b, :len(g["blocks"])], wframes) and not frames[b, len(g["blocks"]):].any(), b
        assert wframes.sum() == lens[b]
        ties += b >= len(graphs) - 4
    assert ties == 4


@pytest.fixture(scope="module")
def corpus_run(dev):
    lex, utts = C.corpus(SEED, N_UTT)
    ids = A.phone_table(lex)
    graphs = [A.utterance_graph(u["words"], lex, ids, C.STATES) for u in utts]
    xs = [R.features(u["mel"]) for u in utts]
    n_classes = len(ids) * C.STATES
    frames = [len(x) for x in xs]
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, 12 << 20):
        mel = padded([utts[i]["mel"].T for i in batch], NAN, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        feats = A.features(mel, lens)
        for r, n in enumerate(lens):
            feats[r, n:] = NAN                                             # rows beyond an utterance must never be read
        batches.append((feats, lens, [graphs[i] for i in batch], batch))
    assert len(batches) >= 3

    def run():
        al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev)
        hist = al.fit([b[:3] for b in batches], ITERS)
        got = [None] * len(utts)
        for feats, lens, gs, batch in batches:
            for i, fr in zip(batch, al.align(feats, lens, gs)):
                got[i] = fr
        return al.mu.cpu().numpy().copy(), al.var.cpu().numpy().copy(), hist, got
    return utts, graphs, xs, n_classes, run(), run


def test_fit_and_align_against_oracle_em(corpus_run):
    utts, graphs, xs, n_classes, (mu, var, hist, got), _ = corpus_run
    omu, ovar, ohist = R.fit(xs, graphs, n_classes, ITERS)
    print("loglik per frame", hist, ohist)
    rel_close(hist, ohist)
    want = [R.align(x, g, omu, ovar) for x, g in zip(xs, graphs)]
    differ = sum(1 for a, b in zip(got, want) if not np.array_equal(a, b))
    true = [[d for _, d in u["segments"]] for u in utts]
    a_ref, a_gpu = C.accuracy(true, want, 1), C.accuracy(true, got, 1)
    print("utterances that differ", differ, "of", len(utts), "A_ref", a_ref, "A_gpu", a_gpu)
    assert differ <= 0.02 * len(utts), differ
    assert a_ref >= 0.95 and a_gpu >= a_ref - 0.01, (a_ref, a_gpu)


def test_two_runs_are_bitwise_equal(corpus_run):
    _, _, _, _, (mu, var, hist, got), run = corpus_run
    mu2, var2, hist2, got2 = run()
    assert np.array_equal(mu, mu2) and np.array_equal(var, var2) and hist == hist2
    assert all(np.array_equal(a, b) for a, b in zip(got, got2))


def test_command_line_to_preprocessor(dev, tmp_path):
    """align.py writes the TextGrids, refuses to overwrite them, and the preprocessor consumes them; on stationary tones with abrupt
    changes (1024 window, 256 hop) at least 90 % of the true boundaries are found within +-2 frames."""
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 99, 24)
    cfg = config(root, lexicon_path)
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    cmd = [sys.executable, os.path.join(ROOT, "align.py"), os.path.join(root, "preprocess.yaml")]
    first = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert first.returncode == 0, first.stdout[-2000:] + first.stderr[-2000:]
    assert "24 TextGrids written, 0 utterances skipped" in first.stdout, first.stdout
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    before = {name: open(tg(name), "rb").read() for name in truth}
    second = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert second.returncode != 0 and "--overwrite" in second.stderr, second.stderr[-2000:]
    third = subprocess.run(cmd + ["--overwrite"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert third.returncode == 0, third.stderr[-2000:]
    assert before == {name: open(tg(name), "rb").read() for name in truth}                   # byte-identical on a second run

    true, got = [], []
    for name, segs in truth.items():
        iv = P.read_textgrid(tg(name))["phones"]
        edges = [int(round(e * C.SR / C.HOP)) for _, e, _ in iv]
        assert iv[0][0] == 0.0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
        assert edges[-1] == sum(d for _, d in segs) + 1                    # samples // hop + 1 frames
        assert [p for _, _, p in iv if p not in P.SIL_PHONES] == [p for p, _ in segs if p not in P.SIL_PHONES]
        true.append([d for _, d in segs])
        got.append(np.diff([0] + edges))
    acc = C.accuracy(true, got, 2)
    print("boundaries within 2 frames", acc)
    assert acc >= 0.90, acc

    out = P.Preprocessor(cfg, device=dev, pitch="gpu", seed=0).build_from_path()
    assert len(out) >= 12                                                  # an utterance DIO finds unvoiced is dropped, as always
    for line in out:
        name = line.split("|")[0]
        dur = np.load(os.path.join(root, "pre", "duration", f"spk-duration-{name}.npy"))
        mel = np.load(os.path.join(root, "pre", "mel", f"spk-mel-{name}.npy"))
        assert dur.sum() == mel.shape[0] and len(dur) == len(line.split("|")[2].strip("{}").split())


def test_bad_arguments(dev):
    lex = {"a": ["X"]}
    ids = A.phone_table(lex)
    g = A.utterance_graph(["a"], lex, ids, 2)
    G = A.Graphs([g], dev)
    E = torch.zeros(1, 8, G.Jmax, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.forward(E.cpu(), [8], G)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.viterbi(E.cpu(), [8], G)
    with pytest.raises(ValueError):
        A.forward(E, [8, 8], G)                                            # lens does not match the batch
    with pytest.raises(ValueError):
        A.forward(E, [9], G)                                               # longer than the buffer
    with pytest.raises(ValueError):
        A.viterbi(E[:, :, :3], [8], G)                                     # fewer columns than states
    big = A.utterance_graph(["a"] * 300, lex, ids, 2)
    assert len(big["sid"]) > A.max_states()
    with pytest.raises(ValueError, match="supported maximum"):
        A.Graphs([big], dev)
    wide = torch.zeros(1, 2, 1025, dtype=torch.float64, device=dev)
    i32 = torch.zeros(1025, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="supported maximum"):             # the ABI itself refuses before any launch
        _lib.call("fs2_align_forward", wide.data_ptr(), wide.stride(0), wide.stride(1), i32.data_ptr(), i32.data_ptr(), i32.data_ptr(),
                  1025, i32.data_ptr(), wide.data_ptr(), wide.stride(0), wide.stride(1), wide.data_ptr(), 1, 2, 1025, None)
    al = A.Aligner(len(ids) * 2, 4, 2, dev)
    with pytest.raises(ValueError, match="mandatory"):
        al.align(torch.zeros(1, 1, 4, dtype=torch.float64, device=dev), [1], [g])
