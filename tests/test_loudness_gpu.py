"""GPU programme loudness (fastspeech2_amd/loudness.py, csrc/fs2_loudness.hip) against the fp64 restatement tests/loudness_ref.py;
prepare_align(normalize="loudness") and the root loudness.py end to end.  Every batch's padding is NaN."""
import functools
import json
import os
import runpy
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from fastspeech2_amd import _lib, ops
from fastspeech2_amd import loudness as L
from fastspeech2_amd import prepare_align as PA
from fastspeech2_amd import resample as R
from tests import loudness_ref as ref
from tests import resample_corpus as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [22050, 16000, 11025]
SILENT = 8                                                                  # row of zeros in `_rows`


@functools.lru_cache(maxsize=None)
def _rows(fs):
    """seeded noise under a slow envelope at the lengths where the block count or the chunking changes, a row of length 0, a pure
    997 Hz sine, a silent row; with the reference's block energies, computed once per rate"""
    n, h = ref.sizes(fs)
    chunk = _lib.load().fs2_kweight_chunk()
    rng = np.random.default_rng(fs)
    rows = []
    for length in (n - 1, n, n + h - 1, n + h, chunk + 1, 67693, 0):
        t = np.arange(length) / fs
        rows.append((0.3 * rng.standard_normal(length) * (0.02 + 0.98 * np.sin(2 * np.pi * 0.25 * t + 0.3) ** 2)).astype(np.float32))
    rows.append(np.sin(2 * np.pi * 997.0 * np.arange(3 * n) / fs).astype(np.float32))
    rows.append(np.zeros(n + h, np.float32))
    assert len(rows) == SILENT + 1
    return rows, [ref.block_energies(x, fs) for x in rows]


def _batch(rows, dev):
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(max(lens), 1)), np.nan, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :lens[b]] = r
    return torch.from_numpy(x).to(dev), lens


@pytest.mark.parametrize("fs", RATES)
def test_block_energies_match_the_reference(dev, fs):
    """1e-9 relative on every z[b, i]: both sides are fp64 on float32 inputs, the recursion grows rounding errors by about
    1 / (1 - r)^2 = 4e4 units of 1e-16; any fp32 state or wrong chunk seam is orders of magnitude beyond it."""
    rows, zs = _rows(fs)
    x, lens = _batch(rows, dev)
    z, nb = L.block_energy(x, lens, fs)
    assert z.dtype == torch.float64 and nb.dtype == torch.int32
    z, nb = z.cpu().numpy(), nb.cpu().numpy()
    assert nb.tolist() == [len(zr) for zr in zs] and nb[:7].tolist() == [0, 1, 1, 2, 0, L.n_blocks(67693, fs), 0]
    worst = 0.0
    for b, zr in enumerate(zs):
        if len(zr) and zr.max() > 0:
            worst = max(worst, float((np.abs(z[b, :len(zr)] - zr) / zr).max()))
        else:
            assert not z[b, :len(zr)].any()
    print(f"fs {fs}: largest relative error of a block energy {worst:.2e}")
    assert worst <= 1e-9
    # the same bytes on a second run; a row alone (B = 1) equals its row in the batch
    z2, nb2 = L.block_energy(x, lens, fs)
    assert np.array_equal(nb2.cpu().numpy(), nb)
    z2 = z2.cpu().numpy()
    for b in range(len(rows)):
        assert z2[b, :nb[b]].tobytes() == z[b, :nb[b]].tobytes(), b
    xa, la = _batch([rows[5]], dev)
    za, nba = L.block_energy(xa, la, fs)
    assert nba.tolist() == [nb[5]] and za.cpu().numpy()[0].tobytes() == z[5, :nb[5]].tobytes()


def test_rows_without_a_block_touch_nothing(dev):
    """the C entry point with z pre-filled: a row of no block leaves its z row alone, the others write [0, n_blocks) only"""
    fs = 22050
    rows, zs = _rows(fs)
    x, lens = _batch(rows, dev)
    coef, pw, chunk, n, h = L._device_tables(dev, fs)
    B, N = x.shape
    M = (N - n) // h + 1
    z = torch.full((B, M + 3), 777.0, dtype=torch.float64, device=dev)
    nb = torch.full((B,), -5, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().fs2_kweight_energy_ws(B, N, h), dtype=torch.float64, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    _lib.call("fs2_kweight_energy", x.data_ptr(), N, lens_d.data_ptr(), coef.ctypes.data, pw.data_ptr(), chunk, n, h, z.data_ptr(),
              M + 3, nb.data_ptr(), ws.data_ptr(), ws.numel(), B, N, ops._stream())
    zh, nbh = z.cpu().numpy(), nb.cpu().numpy()
    for b, zr in enumerate(zs):
        assert nbh[b] == len(zr) and np.all(zh[b, len(zr):] == 777.0) and not np.any(zh[b, :len(zr)] == 777.0), b
    with pytest.raises(ValueError):
        _lib.call("fs2_kweight_energy", x.data_ptr(), N, lens_d.data_ptr(), coef.ctypes.data, pw.data_ptr(), chunk + 1, n, h,
                  z.data_ptr(), M + 3, nb.data_ptr(), ws.data_ptr(), ws.numel(), B, N, ops._stream())
    with pytest.raises(ValueError):
        _lib.call("fs2_kweight_energy", x.data_ptr(), N, lens_d.data_ptr(), coef.ctypes.data, pw.data_ptr(), chunk, n, h,
                  z.data_ptr(), M + 3, nb.data_ptr(), ws.data_ptr(), ws.numel() - 1, B, N, ops._stream())
    with pytest.raises(ValueError):
        L.block_energy(x.double(), lens, fs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.block_energy(x.cpu(), lens, fs)


@pytest.mark.parametrize("fs", RATES)
def test_integrated_loudness_and_gate_counts(dev, fs):
    rows, zs = _rows(fs)
    want = [ref.gated(zr) for zr in zs]
    for zr, (loud, _, n_abs, n_rel, thr) in zip(zs, want):                  # on the reference alone: no block near a threshold
        if n_abs:
            l = ref.block_loudness(zr)
            assert np.abs(l - (-70.0)).min() > 1e-6 and np.abs(l - thr).min() > 1e-6
    assert any(0 < w[3] < w[2] for w in want)                               # the relative gate drops blocks somewhere
    x, lens = _batch(rows, dev)
    out = L.integrated(*L.block_energy(x, lens, fs)).cpu().numpy()
    assert out.shape == (len(rows), 5)
    worst = 0.0
    for b, (loud, mmax, n_abs, n_rel, _) in enumerate(want):
        assert out[b, 2:].tolist() == [len(zs[b]), n_abs, n_rel], b
        if len(zs[b]) == 0:
            assert np.isnan(out[b, 0]) and np.isnan(out[b, 1])
        elif b == SILENT:
            assert out[b, 0] == -np.inf and out[b, 1] == -np.inf and loud == -np.inf
        else:
            worst = max(worst, abs(out[b, 0] - loud), abs(out[b, 1] - mmax))
    print(f"fs {fs}: largest loudness error {worst:.2e} LU")
    assert worst <= 1e-7
    m = L.measure(x, lens, fs, true_peak=True)
    assert [d["n_blocks"] for d in m] == [len(zr) for zr in zs] and m[7]["lufs"] == out[7, 0]
    # the full-scale sine; its abrupt end may overshoot in the interpolator, so the oversampled peak is only bracketed
    assert abs(m[7]["sample_peak_dbfs"]) < 1e-3 and -0.01 < m[7]["true_peak_dbtp"] < 1.5
    assert set(m[0]) == {"lufs", "momentary_max", "sample_peak_dbfs", "n_blocks", "gated_abs", "gated_rel", "true_peak_dbtp"}


def test_cast_is_bit_exact(dev):
    rows, _ = _rows(22050)
    x, lens = _batch(rows, dev)
    g = np.array([1.0, 0.37, 2.5, 1e-3, 7.0, 3.0, 1.0, 1.0 - 2.0 ** -17, 1.0], dtype=np.float64)
    pcm, sat = L.gain_pcm(x, lens, torch.from_numpy(g).to(dev))
    assert pcm.dtype == torch.int16 and sat.dtype == torch.int32
    pcm, sat = pcm.cpu().numpy(), sat.cpu().numpy()
    for b, r in enumerate(rows):
        want, n_sat = ref.cast(r, g[b])
        assert np.array_equal(pcm[b, :len(r)], want) and sat[b] == n_sat and not pcm[b, len(r):].any(), b
    assert sat[5] > 100 and sat[0] == 0                                     # 3 x noise of sigma up to 0.3 saturates
    ties = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32767.5, -32768.5, 32767.4, 40000.0]], dtype=np.float32) / 32768.0
    pcm, sat = L.gain_pcm(torch.from_numpy(ties).to(dev), [10], torch.ones(1, dtype=torch.float64, device=dev))
    assert pcm.cpu().numpy()[0].tolist() == [0, 2, 2, 0, -2, -2, 32767, -32768, 32767, 32767] and sat.tolist() == [2]
    with pytest.raises(ValueError):
        L.gain_pcm(x, lens, torch.ones(len(rows), dtype=torch.float32, device=dev))


def test_through_the_device_gain(dev):
    """peak_abs -> block_energy -> integrated -> gain -> gain_pcm against the reference end to end: g differs by about 1e-12
    relative, so only exact rounding ties can flip.  MI355X run: 0 differing samples of 144 931 (share 0); the test prints the share."""
    fs = 22050
    rows, zs = _rows(fs)
    x, lens = _batch(rows, dev)
    peak = R.peak_abs(x, lens)
    loud = L.integrated(*L.block_energy(x, lens, fs))
    g, flags = L.gain(loud, peak, -10.0, -1.0)
    pcm, sat = L.gain_pcm(x, lens, g)
    g, flags, pcm, sat = g.cpu().numpy(), flags.cpu().numpy(), pcm.cpu().numpy(), sat.cpu().numpy()
    differ = total = 0
    seen = set()
    for b, r in enumerate(rows):
        pk = float(np.abs(r).max()) if len(r) else 0.0
        rg, limited, fallback = ref.gain(ref.gated(zs[b])[0], pk, -10.0, -1.0)
        assert flags[b] == (1 if limited else 0) | (2 if fallback else 0), b
        assert abs(g[b] - rg) <= 1e-10 * rg, (b, g[b], rg)
        seen.add(int(flags[b]))
        want, n_sat = ref.cast(r, rg)
        d = np.abs(pcm[b, :len(r)].astype(np.int32) - want.astype(np.int32))
        assert d.max(initial=0) <= 1 and sat[b] == n_sat == 0, b
        differ += int(np.count_nonzero(d))
        total += d.size
    print(f"device gain: share of differing samples {differ} / {total} = {differ / total:.2e}")
    assert differ / total <= 1e-5 and seen == {0, 1, 2}
    with pytest.raises(ValueError):
        L.gain(loud, peak, 3.0, -1.0)
    with pytest.raises(ValueError):
        L.gain(loud, peak, -23.0, 1.0)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tree(dev, tmp_path_factory):
    """24 kHz LibriTTS-layout corpus: speaker 26 is 12 dB below speaker 19; one file of quiet speech with a full-scale click; one
    file shorter than 400 ms.  Through prepare_align(normalize="loudness") once."""
    root = str(tmp_path_factory.mktemp("loudness"))
    cfg, wavs, labs = C.make_libritts(root, sr=24000, other_sr=24000, dur=1.0)
    corpus = cfg["path"]["corpus_path"]

    def add(spk, chap, name, x):
        folder = os.path.join(corpus, spk, chap)
        C._write(os.path.join(folder, name + ".wav"), 24000, x)
        with open(os.path.join(folder, name + ".normalized.txt"), "w") as f:
            f.write("some words\n")
        return os.path.join(cfg["path"]["raw_path"], spk, name + ".wav")
    loud_tone = C._signal("tone", 24000, 1.21, 13)
    add("26", "495", "26_495_000004_000000", loud_tone * 10 ** (-12 / 20))
    quiet = 0.01 * C._signal("noise", 24000, 1.5, 31)
    quiet[17000] = 1.0
    click = add("19", "198", "19_198_000009_000000", quiet)
    short = add("26", "495", "26_495_000009_000000", C._signal("tone", 24000, 0.3, 5))
    report = os.path.join(root, "report.jsonl")
    n = PA.prepare_align(cfg, device=dev, num_workers=2, normalize="loudness", target_lufs=-23, report=report)
    assert n == 6
    return cfg, [json.loads(line) for line in open(report)], click, short, list(wavs)


def test_prepare_align_normalises_to_the_target(tree):
    """every normal file, re-read from disk and measured by the reference, within 0.05 LU of -23 (int16 quantisation at that
    level: a quantisation noise of 1 / 12 LSB^2 under a signal of about 2300 LSB rms moves the loudness by about 1e-7 LU).  MI355X
    run: largest deviation below 5e-5 LU (printed as 0.0000); the test prints it."""
    cfg, rows, click, short, normal = tree
    assert len(rows) == 6 and all(tuple(r) == PA.REPORT_KEYS for r in rows)
    by_wav = {r["wav"]: r for r in rows}
    assert set(by_wav) == set(normal) | {click, short}
    worst = 0.0
    for path in normal:
        rate, pcm = wavfile.read(path)
        assert rate == 22050 and pcm.dtype == np.int16
        got = ref.loudness(pcm / 32768.0, 22050)
        worst = max(worst, abs(got + 23.0))
        r = by_wav[path]
        assert not r["limited"] and not r["fallback"] and r["clipped"] == 0 and abs(r["lufs_out"] + 23.0) < 1e-9
        assert abs(r["lufs_in"] + r["gain_db"] - r["lufs_out"]) < 1e-9
    print(f"largest deviation from the target: {worst:.1e} LU")
    assert worst <= 0.05
    tones = sorted(p for p in normal if p.endswith("_000000.wav"))           # speaker 19's tone, speaker 26's 12 dB below
    assert len(tones) == 2 and 11.0 < by_wav[tones[0]]["lufs_in"] - by_wav[tones[1]]["lufs_in"] < 13.0
    r = by_wav[click]
    assert r["limited"] and not r["fallback"] and r["lufs_out"] < -23.0
    peak = int(np.abs(wavfile.read(click)[1].astype(np.int32)).max())
    assert abs(peak - 10 ** (-1 / 20) * 32768) <= 1.0, peak
    r = by_wav[short]
    assert r["fallback"] and not r["limited"] and r["lufs_in"] is None and r["lufs_out"] is None
    peak = int(np.abs(wavfile.read(short)[1].astype(np.int32)).max())
    assert abs(peak - 10 ** (-1 / 20) * 32768) <= 1.0, peak


def test_root_loudness_reads_back_the_report(tree, capsys, monkeypatch):
    cfg, rows, click, short, normal = tree
    monkeypatch.setattr(sys, "argv", ["loudness.py", cfg["path"]["raw_path"], "--num_workers", "2"])
    runpy.run_path(os.path.join(ROOT, "loudness.py"), run_name="__main__")
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    got = {r["wav"]: r for r in lines[:-1]}
    assert lines[-1]["summary"]["files"] == 6 and lines[-1]["summary"]["measured"] == 5 and len(got) == 6
    for r in rows:
        if r["lufs_out"] is None:
            assert got[r["wav"]]["lufs"] is None and got[r["wav"]]["n_blocks"] == 0
        else:
            assert abs(got[r["wav"]]["lufs"] - r["lufs_out"]) <= 0.05, r["wav"]


def test_default_is_unchanged(dev, tmp_path):
    """prepare_align(cfg) as before and with normalize="peak" spelled out write the same bytes, and those stay within what
    tests/test_resample_gpu.py pins against the reference pipeline (1 LSB, at most 1e-3 of the samples)"""
    cfg, wavs, labs = C.make_libritts(str(tmp_path), sr=24000, other_sr=24000, dur=1.0)
    raw_a = cfg["path"]["raw_path"]
    assert PA.prepare_align(cfg, device=dev, num_workers=2) == 4
    cfg["path"]["raw_path"] = raw_b = raw_a + "_b"
    assert PA.prepare_align(cfg, device=dev, num_workers=2, normalize="peak") == 4
    differ = total = 0
    for path, (x, sr) in wavs.items():
        a, b = open(path, "rb").read(), open(path.replace(raw_a, raw_b), "rb").read()
        assert a == b, path
        pcm = wavfile.read(path)[1]
        want = C.ref_audio_fn([x], sr, 22050, 32768.0)[0]
        d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
        assert pcm.shape == want.shape and d.max() <= 1
        differ += int(np.count_nonzero(d))
        total += d.size
    assert differ / total <= 1e-3
    with pytest.raises(ValueError, match="report"):
        PA.prepare_align(cfg, device=dev, report=str(tmp_path / "r.jsonl"))
