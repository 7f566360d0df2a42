"""GPU STOI / ESTOI (fastspeech2_amd/stoi.py, csrc/fs2_stoi.hip) against the fp64 restatement tests/stoi_ref.py: every kernel alone
on the restatement's own input for that stage, then `measure`, score.py --aligned and copysynth.py end to end.  Integer outputs
must be equal; floating outputs are held to the bars of tests/golden/stoi_bars.json: 16 times the distance between the fp64 and the
longdouble restatement on these inputs (tests/golden/make_stoi_bars.py), never anything a kernel gave.  Every batch's padding is NaN."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import yaml
from scipy.io import wavfile

from fastspeech2_amd import _lib, ops
from fastspeech2_amd import resample as R
from fastspeech2_amd import stoi as S
from tests import stoi_ref as ref
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "stoi_bars.json")))
LONG = len(ref.LENGTHS) - 1                                                 # the row with the planted silences
SR, HOP = 22050, 256


def bar(stage):
    return BARS["factor"] * BARS["distance"][stage]


@functools.lru_cache(maxsize=None)
def _case():
    """the test pairs at 10 kHz and the restatement's chain of each, computed once"""
    assert BARS["seed"] == ref.SEED and tuple(BARS["lengths"]) == ref.LENGTHS and tuple(BARS["lengths_22k"]) == ref.LENGTHS_22K
    pairs = ref.pairs()
    return pairs, [ref.chain(x, y) for x, y in pairs]


def _batch(rows, dev, dtype=np.float32, width=None):
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(max(lens), 1) if width is None else width), np.nan, dtype=dtype)
    for b, r in enumerate(rows):
        x[b, :lens[b]] = r
    return torch.from_numpy(x).to(dev), lens


def _worst(got, want, what):
    """largest elementwise distance over the rows' valid parts"""
    w = 0.0
    for b, (g, r) in enumerate(zip(got, want)):
        assert g.shape == r.shape, (what, b, g.shape, r.shape)
        if r.size:
            assert np.isfinite(g).all(), (what, b)
            w = max(w, float(np.abs(g - r).max()))
    return w


def test_the_inputs_are_what_the_cases_need():
    """on the reference alone: the frame and segment counts at the edges, silences that drop frames, and no frame whose energy is
    within a factor 1 +- 1e-6 of the threshold, so that a flipped keep decision is a bug and not rounding"""
    pairs, chains = _case()
    assert [c["frames"] for c in chains] == [0, 1, 29, 30, 31, S.n_frames(15000)]
    assert [c["X"].shape[1] for c in chains[:5]] == [0, 0, 28, 29, 30] and [c["segments"] for c in chains[:5]] == [0, 0, 0, 0, 1]
    c = chains[LONG]
    assert 30 < c["frames_kept"] < c["frames"] - 20 and not c["mask"][0] and not c["mask"][-1] and not c["mask"][len(c["mask"]) // 2 + 2]
    for c in chains:
        assert ref.threshold_margin(c) > 1e-6


def test_frame_energies(dev):
    pairs, chains = _case()
    x, lens = _batch([p[0] for p in pairs], dev)
    e = S.frame_energy(x, lens)
    assert e.dtype == torch.float64 and e.shape == (len(pairs), S.n_frames(max(lens)))
    e = e.cpu().numpy()
    worst = _worst([e[b, :c["frames"]] for b, c in enumerate(chains)], [c["e"] for c in chains], "e")
    print(f"frame energies: largest distance {worst:.2e}, bar {bar('energy'):.2e}")
    assert worst <= bar("energy")
    xa, la = _batch([pairs[LONG][0]], dev)                                  # B = 1: the same bytes as the row in the batch
    assert S.frame_energy(xa, la).cpu().numpy()[0].tobytes() == e[LONG, :chains[LONG]["frames"]].tobytes()
    with pytest.raises(ValueError):
        S.frame_energy(x.double(), lens)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.frame_energy(x.cpu(), lens)


def test_keep_mask_and_compaction_map_are_exact(dev):
    pairs, chains = _case()
    lens = [len(p[0]) for p in pairs]
    for rows in (list(range(len(pairs))), [LONG]):
        e, _ = _batch([chains[b]["e"] for b in rows], dev, np.float64, width=max(S.n_frames(max(lens[b] for b in rows)), 1))
        mask, cmap, n_kept = S.keep(e, [lens[b] for b in rows])
        assert mask.dtype == cmap.dtype == n_kept.dtype == torch.int32
        mask, cmap, n_kept = mask.cpu().numpy(), cmap.cpu().numpy(), n_kept.cpu().numpy()
        for r, b in enumerate(rows):
            c = chains[b]
            assert n_kept[r] == c["frames_kept"], b
            assert np.array_equal(mask[r, :c["frames"]], c["mask"].astype(np.int32)), b
            assert np.array_equal(cmap[r, :n_kept[r]], c["map"]), b
    # all-zero energies keep nothing (e_max > 0 is part of the rule)
    z = torch.zeros(1, S.n_frames(3000), dtype=torch.float64, device=dev)
    assert S.keep(z, [3000])[2].tolist() == [0]


def test_overlap_add_is_a_gather_of_the_kept_frames(dev):
    pairs, chains = _case()
    x, lens = _batch([p[0] for p in pairs], dev)
    y, _ = _batch([p[1] for p in pairs], dev)
    F = S.n_frames(max(lens))
    cmap = np.full((len(pairs), F), -7, np.int32)
    for b, c in enumerate(chains):
        cmap[b, :c["frames_kept"]] = c["map"]
    n_kept = torch.tensor([c["frames_kept"] for c in chains], dtype=torch.int32, device=dev)
    xo, yo = S.overlap_add(x, y, lens, torch.from_numpy(cmap).to(dev), n_kept)
    assert xo.dtype == torch.float64 and xo.shape == yo.shape == (len(pairs), (F - 1) * 128 + 256)
    xo, yo = xo.cpu().numpy(), yo.cpu().numpy()
    worst = max(_worst([xo[b, :len(c["xo"])] for b, c in enumerate(chains)], [c["xo"] for c in chains], "xo"),
                _worst([yo[b, :len(c["yo"])] for b, c in enumerate(chains)], [c["yo"] for c in chains], "yo"))
    print(f"overlap-add: largest distance {worst:.2e}, bar {bar('overlap_add'):.2e}")
    assert worst <= bar("overlap_add")
    assert [len(c["xo"]) for c in chains[:3]] == [0, 256, 28 * 128 + 256]


def test_band_magnitudes(dev):
    pairs, chains = _case()
    worst = 0.0
    for key, out in (("xo", "X"), ("yo", "Y")):
        F = S.n_frames(max(len(p[0]) for p in pairs))
        sig, _ = _batch([c[key] for c in chains], dev, np.float64, width=(F - 1) * 128 + 256)
        n_kept = torch.tensor([c["frames_kept"] for c in chains], dtype=torch.int32, device=dev)
        X = S.band_magnitudes(sig, n_kept)
        assert X.dtype == torch.float64 and X.shape == (len(pairs), 15, F - 1)
        X = X.cpu().numpy()
        worst = max(worst, _worst([X[b, :, :c[out].shape[1]] for b, c in enumerate(chains)], [c[out] for c in chains], out))
        if key == "xo":                                                     # B = 1
            one, _ = _batch([chains[LONG]["xo"]], dev, np.float64)
            Xa = S.band_magnitudes(one, n_kept[LONG:LONG + 1]).cpu().numpy()
            M = chains[LONG]["X"].shape[1]
            assert Xa.shape[2] == M and Xa[0].tobytes() == np.ascontiguousarray(X[LONG, :, :M]).tobytes()
    print(f"band magnitudes: largest distance {worst:.2e}, bar {bar('bands'):.2e}")
    assert worst <= bar("bands")


def _bands_batch(chains, key, dev):
    M = max(c[key].shape[1] for c in chains)
    X = np.full((len(chains), 15, M), np.nan)
    for b, c in enumerate(chains):
        X[b, :, :c[key].shape[1]] = c[key]
    return torch.from_numpy(X).to(dev)


def test_segment_scores_and_row_means(dev):
    pairs, chains = _case()
    lens = [len(p[0]) for p in pairs]
    n_kept = torch.tensor([c["frames_kept"] for c in chains], dtype=torch.int32, device=dev)
    seg = S.segment_scores(_bands_batch(chains, "X", dev), _bands_batch(chains, "Y", dev), n_kept)
    Smax = max(c["segments"] for c in chains)
    assert seg.dtype == torch.float64 and seg.shape == (len(pairs), 2, Smax)
    segh = seg.cpu().numpy()
    worst = _worst([segh[b, :, :c["segments"]] for b, c in enumerate(chains)], [c["seg"] for c in chains], "seg")
    print(f"segment scores: largest distance {worst:.2e}, bar {bar('segments'):.2e}")
    assert worst <= bar("segments")
    # the ordered mean, on the restatement's own segment scores
    want = np.full((len(pairs), 2, S.n_frames(max(lens)) - 30), np.nan)     # as wide as the longest row could need
    for b, c in enumerate(chains):
        want[b, :, :c["segments"]] = c["seg"]
    out = S.row_scores(torch.from_numpy(want).to(dev), lens, n_kept).cpu().numpy()
    worst = 0.0
    for b, c in enumerate(chains):
        assert out[b, 2:].tolist() == [c["frames"], c["frames_kept"], c["segments"], float(c["too_short"])], b
        if c["too_short"]:
            assert np.isnan(out[b, 0]) and np.isnan(out[b, 1]), b
        else:
            worst = max(worst, abs(out[b, 0] - c["stoi"]), abs(out[b, 1] - c["estoi"]))
    print(f"row means: largest distance {worst:.2e}, bar {bar('final'):.2e}")
    assert worst <= bar("final")
    one = S.segment_scores(_bands_batch([chains[LONG]], "X", dev), _bands_batch([chains[LONG]], "Y", dev), n_kept[LONG:LONG + 1])
    assert one.cpu().numpy()[0].tobytes() == np.ascontiguousarray(segh[LONG, :, :chains[LONG]["segments"]]).tobytes()


def test_bad_arguments_are_refused_before_launch(dev):
    pairs, _ = _case()
    x, lens = _batch([p[0] for p in pairs], dev)
    e = S.frame_energy(x, lens)
    with pytest.raises(ValueError):
        S.keep(e[:, :3].contiguous(), lens)                                 # too few frames for these lengths
    mask, cmap, n_kept = S.keep(e, lens)
    with pytest.raises(ValueError):
        S.overlap_add(x, x[:, :-1], lens, cmap, n_kept)
    with pytest.raises(ValueError):
        S.overlap_add(x, x, lens, cmap, n_kept.long())
    with pytest.raises(ValueError):
        S.segment_scores(torch.zeros(2, 14, 40, dtype=torch.float64, device=dev), torch.zeros(2, 14, 40, dtype=torch.float64, device=dev),
                         n_kept[:2])
    w, tw, edges = S._device_tables(dev)
    X = torch.empty(1, 15, 40, dtype=torch.float64, device=dev)
    sig = torch.zeros(1, 40 * 128 + 256, dtype=torch.float64, device=dev)
    bad = edges.copy()
    bad[3] = bad[4] + 1                                                     # not ascending
    with pytest.raises(ValueError, match="band edges"):
        _lib.call("fs2_stoi_bands", sig.data_ptr(), sig.shape[1], n_kept.data_ptr(), w.data_ptr(), tw.data_ptr(), bad.ctypes.data,
                  X.data_ptr(), 15 * 40, 40, 1, 41, ops._stream())
    with pytest.raises(ValueError):                                         # X too narrow for Fmax - 1 frames
        _lib.call("fs2_stoi_bands", sig.data_ptr(), sig.shape[1], n_kept.data_ptr(), w.data_ptr(), tw.data_ptr(), edges.ctypes.data,
                  X.data_ptr(), 15 * 39, 39, 1, 41, ops._stream())
    with pytest.raises(ValueError):
        _lib.call("fs2_stoi_segments", X.data_ptr(), X.data_ptr(), 15 * 40, 40, n_kept.data_ptr(), 0.5, X.data_ptr(), 80, 40, 1, 41,
                  ops._stream())


# ------------------------------------------------------------------------------------------------ end to end
def _measure_twice(dev, pairs, sr):
    x, xl = _batch([p[0] for p in pairs], dev)
    y, yl = _batch([p[1] for p in pairs], dev)
    a, b = S.measure(x, xl, y, yl, sr), S.measure(x, xl, y, yl, sr)
    assert set(a) == {"stoi", "estoi", "frames", "frames_kept", "segments", "too_short"}
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    return {k: v.cpu().numpy() for k, v in a.items()}


def test_measure_at_10k_against_the_restatement(dev):
    pairs, chains = _case()
    cut = [(x, y[:len(y) - 5 * (b % 2)]) for b, (x, y) in enumerate(pairs)]  # odd rows: the processed side 5 samples short
    want = [c if b % 2 == 0 else ref.chain(*cut[b]) for b, c in enumerate(chains)]
    got = _measure_twice(dev, cut, 10000)
    worst = 0.0
    for b, c in enumerate(want):
        assert (got["frames"][b], got["frames_kept"][b], got["segments"][b], bool(got["too_short"][b])) == \
            (c["frames"], c["frames_kept"], c["segments"], c["too_short"]), b
        if c["too_short"]:
            assert np.isnan(got["stoi"][b]) and np.isnan(got["estoi"][b])
        else:
            worst = max(worst, abs(got["stoi"][b] - c["stoi"]), abs(got["estoi"][b] - c["estoi"]))
    print(f"measure at 10 kHz: largest distance {worst:.2e}, bar {bar('final'):.2e}")
    assert worst <= bar("final") and not got["too_short"][LONG]


def test_measure_at_22050_against_the_restatement_on_the_resamplers_output(dev):
    """the restatement is fed what the GPU resampler gave (it has its own tests): only STOI is under test here"""
    pairs = ref.pairs_22k()
    x, xl = _batch([p[0] for p in pairs], dev)
    y, yl = _batch([p[1] for p in pairs], dev)
    x10, l10 = R.resample_poly(x, xl, SR, 10000)
    y10, _ = R.resample_poly(y, yl, SR, 10000)
    x10, y10 = x10.cpu().numpy(), y10.cpu().numpy()
    want = [ref.chain(x10[b, :n], y10[b, :n]) for b, n in enumerate(l10.tolist())]
    assert [c["segments"] > 0 for c in want] == [True, True, False] and all(ref.threshold_margin(c) > 1e-6 for c in want)
    got = _measure_twice(dev, pairs, SR)
    worst = 0.0
    for b, c in enumerate(want):
        assert (got["frames"][b], got["frames_kept"][b], got["segments"][b]) == (c["frames"], c["frames_kept"], c["segments"]), b
        if not c["too_short"]:
            worst = max(worst, abs(got["stoi"][b] - c["stoi"]), abs(got["estoi"][b] - c["estoi"]))
    print(f"measure at 22 050 Hz: largest distance {worst:.2e}, bar {bar('final'):.2e}")
    assert worst <= bar("final") and bool(got["too_short"][2]) and 0 < got["stoi"][1] < 1


def _write(path, x):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, SR, (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _configs(root):
    docs = {"preprocess.yaml": config(root), "model.yaml": {"vocoder": {"model": "HiFi-GAN", "speaker": "universal"}},
            "train.yaml": {"path": {"result_path": os.path.join(root, "result")}}}
    for name, doc in docs.items():
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    return [a for flag, name in (("-p", "preprocess.yaml"), ("-t", "train.yaml")) for a in (flag, os.path.join(root, name))]


def test_score_aligned_on_a_tiny_corpus(dev, tmp_path):
    import score
    root = str(tmp_path)
    sigs = ref.pairs_22k((12000, 14000, 13000), seed=5)
    for k, (x, y) in enumerate(sigs):
        _write(os.path.join(root, "raw", "spk", f"u{k}.wav"), 3 * x)
        _write(os.path.join(root, "result", f"u{k}.wav"), 3 * (y if k < 2 else y[3 * HOP + 1:]))     # u2: offset by three hops
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"u{k}|spk|{{AA B}}|text {k}\n" for k in range(3)))
    argv = _configs(root) + ["--source", os.path.join(root, "val.txt"), "--no_f0", "--out", os.path.join(root, "s.jsonl")]
    plain, skipped0, summary0 = score.main(argv)
    rows, skipped, summary = score.main(argv + ["--aligned"])
    assert len(plain) == 3 and not skipped0 and "stoi_mean" not in summary0 and "stoi" not in plain[0]
    assert [r["basename"] for r in rows] == ["u0", "u1"] and [s[0] for s in skipped] == ["u2"] and "not time-aligned" in skipped[0][1]
    new = {"stoi", "estoi", "stoi_frames_kept", "stoi_segments", "aligned_samples"}
    for r, p in zip(rows, plain):
        assert new <= set(r) and {k: v for k, v in r.items() if k not in new} == p       # the default run's rows are unchanged
        assert r["aligned_samples"] == 12000 + 2000 * int(r["basename"][1]) and r["stoi_segments"] > 0
        assert 0.3 < r["stoi"] < 1 and -0.2 < r["estoi"] < r["stoi"]
    # against the restatement on the resampler's output of what the files hold
    rate, a = wavfile.read(os.path.join(root, "raw", "spk", "u0.wav"))
    _, b = wavfile.read(os.path.join(root, "result", "u0.wav"))
    pair = [torch.from_numpy((v / 32768.0).astype(np.float32)[None]).to(dev) for v in (a, b)]
    a10, b10 = (R.resample_poly(v, [12000], SR, 10000)[0].cpu().numpy()[0] for v in pair)
    c = ref.chain(a10, b10)
    assert abs(rows[0]["stoi"] - c["stoi"]) <= bar("final") and abs(rows[0]["estoi"] - c["estoi"]) <= bar("final")
    assert rows[0]["stoi_frames_kept"] == c["frames_kept"] and rows[0]["stoi_segments"] == c["segments"]
    assert summary["stoi_mean"] == pytest.approx(np.mean([r["stoi"] for r in rows]), abs=1e-15) and summary["stoi_too_short_utterances"] == 0


def test_copysynth_with_griffin_lim_and_score_aligned(dev, tmp_path):
    """two short mels (<= 40 frames) of two signals -> copysynth.py --griffin_iters 2 -> wavs of T hop samples that score.py
    --aligned takes against the signals the mels came from; no vocoder checkpoint is involved"""
    import copysynth
    import score
    from fastspeech2_amd.audio import TacotronSTFT
    root = str(tmp_path)
    cfg = config(root)
    stft = TacotronSTFT(1024, HOP, 1024, 80, SR, 0, 8000).to(dev)
    sigs = [3 * p[0] for p in ref.pairs_22k((39 * HOP + 17, 36 * HOP), seed=9)]
    x, lens = _batch(sigs, dev)
    mel, _, frames = stft.mel_spectrogram_ragged(torch.nan_to_num(x), lens)
    os.makedirs(os.path.join(root, "pre", "mel"))
    for k, s in enumerate(sigs):
        T = int(frames[k])
        assert T <= 40
        np.save(os.path.join(root, "pre", "mel", f"spk-mel-g{k}.npy"), mel[k, :, :T].T.cpu().numpy())
        _write(os.path.join(root, "raw", "spk", f"g{k}.wav"), s)
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("g0|spk|{AA}|x\ng1|spk|{AA}|x\ngone|spk|{AA}|x\n")
    args = _configs(root)
    written, missing = copysynth.main(args + ["-m", os.path.join(root, "model.yaml"), "--source", os.path.join(root, "val.txt"),
                                              "--griffin_iters", "2"])
    assert [m[0] for m in missing] == ["gone"]
    for k, (name, n) in enumerate(written):
        rate, w = wavfile.read(os.path.join(root, "result", "copy", name + ".wav"))
        T = int(frames[k])
        assert rate == SR and len(w) == n == T * HOP and np.isfinite(w).all() and np.abs(w[:(T - 2) * HOP]).max() > 0
    rows, skipped, summary = score.main(args + ["--source", os.path.join(root, "val.txt"), "--syn_dir", os.path.join(root, "result", "copy"),
                                                "--no_f0", "--aligned", "--out", os.path.join(root, "s.jsonl")])
    assert [r["basename"] for r in rows] == ["g0", "g1"] and [s[0] for s in skipped] == ["gone"]
    for r, s in zip(rows, sigs):
        assert r["aligned_samples"] == len(s) and r["stoi_segments"] >= 1 and np.isfinite(r["stoi"]) and np.isfinite(r["estoi"])
    assert np.isfinite(summary["stoi_mean"]) and summary["stoi_too_short_utterances"] == 0
