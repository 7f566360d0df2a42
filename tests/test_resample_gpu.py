"""GPU sample-rate conversion and peak normalisation (fastspeech2_amd/resample.py, csrc/fs2_resample.hip) against known answers
and the fp64 numpy oracle (tests/resample_ref.py); prepare_align and Preprocessor(resample="gpu") end to end."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from fastspeech2_amd import preprocess as P
from fastspeech2_amd import prepare_align as PA
from fastspeech2_amd import resample as R
from tests import f0_signals as S
from tests import resample_corpus as C
from tests.resample_ref import factors, resample_ref, taps

pytestmark = pytest.mark.gpu

PAIRS = [(24000, 22050), (44100, 22050), (48000, 22050), (16000, 22050), (22050, 24000)]


def _batch(rows, dev, poison=np.nan):
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(lens)), poison, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :lens[b]] = r
    return torch.from_numpy(x).to(dev), lens


def _bound(y_ref, x):
    """half a float32 ulp of the fp64 sum, plus the two fp64 summation orders' difference (<= 45 terms, sum |h_phase| about 2)"""
    return 2.0 ** -24 * np.abs(y_ref) + 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("sr_in,sr_out", [(24000, 22050), (16000, 22050)])
def test_unit_impulse_reads_back_the_taps(dev, sr_in, sr_out):
    up, down = factors(sr_in, sr_out)
    assert (up, down) in ((147, 160), (441, 320))
    h, half = taps(up, down)
    n_in = 700
    rows = []
    for i0 in (0, n_in // 2, n_in - 1):
        x = np.zeros(n_in, np.float32)
        x[i0] = 1.0
        rows.append((i0, x))
    xb, lens = _batch([r for _, r in rows], dev)
    y, out_lens = R.resample_poly(xb, lens, sr_in, sr_out)
    y = y.cpu().numpy()
    n_out = -(-n_in * up // down)
    assert out_lens.tolist() == [n_out] * 3 and y.dtype == np.float32
    for b, (i0, _) in enumerate(rows):
        k = np.arange(n_out, dtype=np.int64) * down - i0 * up + half
        want = np.where((k >= 0) & (k <= 2 * half), h[np.clip(k, 0, 2 * half)], 0.0).astype(np.float32)
        assert np.count_nonzero(want) > 8 and np.array_equal(y[b], want), (i0, np.abs(y[b] - want).max())


def _signals(sr, seed):
    rng = np.random.default_rng(seed)
    sp, sp_sr = S.speech()
    sp = resample_ref(sp[:int(0.4 * sp_sr)], sp_sr, sr).astype(np.float32)
    return [S.tone(200, dur=0.35, fs=sr), 6.0 * S.tone(110, dur=0.2, fs=sr), S.glide(dur=0.5, fs=sr)[0], sp,
            rng.standard_normal(5003).astype(np.float32), rng.standard_normal(1).astype(np.float32),
            rng.standard_normal(7).astype(np.float32), rng.standard_normal(2).astype(np.float32)]


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_ragged_batch_matches_the_fp64_reference(dev, sr_in, sr_out):
    """tones, the glide, speech, noise; lengths 1, 2 and 7 (shorter than any phase of the filter); NaN beyond every row's length"""
    rows = _signals(sr_in, sr_in)
    xb, lens = _batch(rows, dev)
    y, yc, out_lens = R.resample_poly(xb, lens, sr_in, sr_out, clip=True)
    y, yc = y.cpu().numpy(), yc.cpu().numpy()
    up, down = factors(sr_in, sr_out)
    assert out_lens.dtype == torch.int64 and out_lens.tolist() == [-(-n * up // down) for n in lens]
    for b, x in enumerate(rows):
        ref = resample_ref(x, sr_in, sr_out)
        assert len(ref) == out_lens[b]
        got = y[b, :len(ref)].astype(np.float64)
        err = np.abs(got - ref)
        assert np.all(err <= _bound(ref, x)), (b, len(x), float((err - _bound(ref, x)).max()))
        assert np.array_equal(yc[b, :len(ref)], np.clip(y[b, :len(ref)], -1.0, 1.0)), b
    loud = y[1, :out_lens[1]]
    assert np.abs(loud).max() > 1.5 and np.abs(yc[1, :out_lens[1]]).max() == 1.0              # the clamp had something to do
    # batch independence: each row alone equals its row in the batch, bit for bit
    for b, x in enumerate(rows):
        xa, la = _batch([x], dev)
        ya, yca, ola = R.resample_poly(xa, la, sr_in, sr_out, clip=True)
        assert ola.tolist() == [int(out_lens[b])]
        assert np.array_equal(ya.cpu().numpy()[0], y[b, :out_lens[b]]) and np.array_equal(yca.cpu().numpy()[0], yc[b, :out_lens[b]]), b


@pytest.mark.parametrize("sr_in,sr_out", [(24000, 22050), (22050, 24000), (44100, 22050), (22050, 22050)])
def test_windows_equal_slices_of_the_full_result(dev, sr_in, sr_out):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(6000).astype(np.float32)
    up, down = factors(sr_in, sr_out)
    n_out = -(-len(x) * up // down)
    xf, lf = _batch([x], dev)
    if sr_in == sr_out:
        same, lens_same = R.resample_poly(xf, lf, sr_in, sr_out)
        assert same.data_ptr() == xf.data_ptr() and lens_same.tolist() == lf                 # the input, unchanged
        full = x
    else:
        full = R.resample_poly(xf, lf, sr_in, sr_out)[0].cpu().numpy()[0]
    assert len(full) == n_out
    wins = [(0, 100), (0, n_out), (1234, 777), (n_out - 50, 50), (n_out - 1, 1), (17, 0), (300, 2600)]
    # (a) the whole row handed over, windows chosen by out_begin / out_len
    xb, lens = _batch([x] * len(wins), dev)
    y, yc, ol = R.resample_poly(xb, lens, sr_in, sr_out, out_begin=[a for a, _ in wins], out_len=[n for _, n in wins], clip=True)
    assert ol.tolist() == [n for _, n in wins] and y.shape == (len(wins), n_out)
    y, yc = y.cpu().numpy(), yc.cpu().numpy()
    for b, (a, n) in enumerate(wins):
        assert np.array_equal(y[b, :n], full[a:a + n]) and np.array_equal(yc[b, :n], np.clip(full[a:a + n], -1, 1)), (a, n)
    # (b) only the input span each window depends on, with in_begin > 0 (NaN everywhere else)
    spans = [R.input_span(a, n, len(x), up, down) for a, n in wins]
    assert spans[2][0] > 0 and spans[3][0] > 0 and spans[2][1] < len(x) and spans[0] != (0, len(x))
    xs, ls = _batch([x[lo:hi] for lo, hi in spans], dev)
    y2, ol2 = R.resample_poly(xs, ls, sr_in, sr_out, out_begin=[a for a, _ in wins], out_len=[n for _, n in wins],
                              in_begin=[lo for lo, _ in spans])
    y2 = y2.cpu().numpy()
    for b, (a, n) in enumerate(wins):
        assert np.array_equal(y2[b, :n], full[a:a + n]), (a, n, spans[b])


def test_large_factors_and_the_unstaged_path(dev):
    """11025 -> 32000 Hz is up / down = 1280 / 441, the largest factor among the usual rates; 64000 -> 1000 Hz (1 / 64, 1282 taps per
    output) needs a tile beyond 64 KiB of LDS and takes the kernel's global-memory form.  Same bound: at 1282 terms the two fp64
    summation orders differ by at most about 2 x 1282 x 2^-53 x sum |h_phase| (about 1) x max|x| = 3e-13 max|x|."""
    rng = np.random.default_rng(11)
    for sr_in, sr_out, n in ((11025, 32000, 900), (64000, 1000, 6400), (8000, 48000, 300), (48000, 8000, 3000)):
        rows = [rng.standard_normal(n).astype(np.float32), rng.standard_normal(n // 3).astype(np.float32)]
        xb, lens = _batch(rows, dev)
        y, out_lens = R.resample_poly(xb, lens, sr_in, sr_out)
        y = y.cpu().numpy()
        for b, x in enumerate(rows):
            ref = resample_ref(x, sr_in, sr_out)
            assert out_lens[b] == len(ref)
            err = np.abs(y[b, :len(ref)].astype(np.float64) - ref)
            assert np.all(err <= _bound(ref, x)), (sr_in, sr_out, b, float((err - _bound(ref, x)).max()))


def test_peak_and_pcm_are_numpy_bit_for_bit(dev):
    rng = np.random.default_rng(5)
    x0 = (0.3 * rng.standard_normal(9000)).astype(np.float32)
    rows = [x0, -x0, np.zeros(4000, np.float32), x0[:3001] * 1e-3]
    xb, lens = _batch(rows, dev)
    y, out_lens = R.resample_poly(xb, lens, 24000, 22050)
    peak = R.peak_abs(y, out_lens)
    pcm = R.peaknorm_pcm(y, out_lens, peak, 32768.0)
    assert peak.dtype == torch.float32 and pcm.dtype == torch.int16 and pcm.shape == y.shape
    yh, peak, pcm = y.cpu().numpy(), peak.cpu().numpy(), pcm.cpu().numpy()
    signs = []
    for b in range(len(rows)):
        n = int(out_lens[b])
        yr = yh[b, :n]
        pk = np.max(np.abs(yr))
        assert peak[b] == pk and peak[b].dtype == np.float32, b
        if b == 2:
            assert pk == 0.0 and not pcm[b].any()                                            # zero row: zeros, not a division by zero
            continue
        with np.errstate(invalid="ignore"):
            want = (yr / pk * np.float32(32768.0)).astype(np.int16)
        assert np.array_equal(pcm[b, :n], want), (b, int(np.abs(pcm[b, :n].astype(np.int32) - want).max()))
        assert not pcm[b, n:].any()
        k = int(np.argmax(np.abs(yr)))
        signs.append(yr[k] > 0)
        assert pcm[b, k] == -32768                                                           # +peak * 32768 wraps, -peak is exact
        assert np.abs(pcm[b, :n].astype(np.int32)).max() == 32768
    assert signs[0] != signs[1]                                                              # a positive and a negative peak row
    # other full-scale values: 32767 keeps a positive peak at 32767
    pcm2 = R.peaknorm_pcm(y, out_lens, torch.from_numpy(peak).to(dev), 32767.0).cpu().numpy()
    for b in (0, 1):
        yr = yh[b, :int(out_lens[b])]
        assert np.array_equal(pcm2[b, :len(yr)], (yr / peak[b] * np.float32(32767.0)).astype(np.int16))


def test_argument_checks(dev):
    x = torch.zeros(2, 64, device=dev)
    with pytest.raises(ValueError):
        R.resample_poly(x.double(), [64, 64], 24000, 22050)
    with pytest.raises(ValueError):
        R.resample_poly(x[0], [64], 24000, 22050)
    with pytest.raises(ValueError):
        R.resample_poly(x, [64, 65], 24000, 22050)
    with pytest.raises(ValueError):
        R.resample_poly(x, [64], 24000, 22050)
    with pytest.raises(ValueError):
        R.resample_poly(x, [64, 64], 24000, 22050, in_begin=[0, 0])                          # a slice needs its window spelt out
    with pytest.raises(ValueError):
        R.resample_poly(x, [64, 64], 24000, 22050, out_begin=[0, -1], out_len=[1, 1])
    with pytest.raises(ValueError):
        R.resample_poly(x, [64, 64], 22050, 65537 * 3)
    with pytest.raises(ValueError):
        R.peaknorm_pcm(x, [64, 64], torch.ones(3, device=dev), 32768.0)
    y, ol = R.resample_poly(x[:, :0].contiguous(), [0, 0], 24000, 22050)
    assert y.shape == (2, 0) and ol.tolist() == [0, 0]


def test_prepare_align_end_to_end(dev, tmp_path):
    """24 kHz LibriTTS-layout tree -> GPU prepare_align, against float32(resample_ref(x)) -> numpy float32 y / max|y| * 32768 ->
    astype(int16): every sample within 1 LSB and at most 1e-3 of all samples different at all.  The GPU's y can differ from
    float32(y_ref) only where the fp64 sum sits within about 1e-14 of a float32 rounding midpoint, so the expected share is
    essentially zero; the cap is sized so that even the float32 pipeline against the same pipeline carried out in fp64 (2.1e-4 to
    4.5e-4 on 3 s signals at this rate pair) stays inside it.
    The MI355X run showed 0 differing samples of 97 462 (share 0); the test prints the share of each run."""
    cfg, wavs, labs = C.make_libritts(str(tmp_path), sr=24000, other_sr=24000, dur=1.0)
    n = PA.prepare_align(cfg, device=dev, num_workers=2)
    assert n == len(wavs) == 4 and C.listing(cfg["path"]["raw_path"]) == sorted(list(wavs) + list(labs))
    differ = total = 0
    for path, (x, sr) in wavs.items():
        rate, pcm = wavfile.read(path)
        want = C.ref_audio_fn([x], sr, 22050, 32768.0)[0]
        assert rate == 22050 and pcm.dtype == np.int16 and pcm.shape == want.shape, path
        d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1, (path, int(d.max()))
        differ += int(np.count_nonzero(d))
        total += d.size
    print(f"prepare_align share of differing samples: {differ} / {total} = {differ / total:.2e}")
    assert total > 80000 and differ / total <= 1e-3, (differ, total)
    for path, text in labs.items():
        assert open(path).read() == text


def test_preprocessor_resamples_on_the_gpu(dev, tmp_path, monkeypatch):
    """Preprocessor(pitch="gpu", resample="gpu") on a 24 kHz corpus against Preprocessor(pitch="gpu") on the same corpus resampled
    beforehand by resample_ref and stored as float32 wavs at 22 050 Hz: same metadata, file sets and durations; arrays and statistics
    within the bars check_against_golden sets between the product and the reference (mel 2e-4, pitch / energy 1e-4, stats 2e-5)."""
    import scipy.signal
    from tests.helpers import make_raw_corpus

    real = os.listdir
    monkeypatch.setattr(os, "listdir", lambda p: sorted(real(p)))
    cfg_a, _ = make_raw_corpus(str(tmp_path / "a"), sr=24000)
    cfg_b, _ = make_raw_corpus(str(tmp_path / "b"), sr=24000)
    for cfg in (cfg_a, cfg_b):
        cfg["preprocessing"]["audio"]["sampling_rate"] = 22050
    raw_b = cfg_b["path"]["raw_path"]
    for spk in os.listdir(raw_b):
        for f in os.listdir(os.path.join(raw_b, spk)):
            if f.endswith(".wav"):
                w, sr = P.load_wav(os.path.join(raw_b, spk, f), resample=False)
                assert sr == 24000
                wavfile.write(os.path.join(raw_b, spk, f), 22050, resample_ref(w, 24000, 22050).astype(np.float32))

    out_b = P.Preprocessor(cfg_b, device=dev, seed=3, pitch="gpu").build_from_path()

    calls = []
    real_load = P.load_wav

    def spy(path, *a, **kw):
        calls.append(kw.get("resample", True))
        return real_load(path, *a, **kw)

    def no_host_resampling(*a, **kw):
        raise AssertionError("the host resampled")
    monkeypatch.setattr(P, "load_wav", spy)
    monkeypatch.setattr(scipy.signal, "resample_poly", no_host_resampling)
    out_a = P.Preprocessor(cfg_a, device=dev, seed=3, pitch="gpu", resample="gpu", batch_seconds=2.5).build_from_path()
    monkeypatch.undo()
    assert calls and not any(calls), calls

    assert out_a == out_b and len(out_a) >= 3
    pre_a, pre_b = cfg_a["path"]["preprocessed_path"], cfg_b["path"]["preprocessed_path"]
    for name in ("train.txt", "val.txt", "speakers.json"):
        assert open(os.path.join(pre_a, name)).read() == open(os.path.join(pre_b, name)).read(), name
    sa, sb = (json.load(open(os.path.join(p, "stats.json"))) for p in (pre_a, pre_b))
    for k in ("pitch", "energy"):
        np.testing.assert_allclose(sa[k], sb[k], rtol=2e-5, atol=2e-5)
    for kind in ("mel", "pitch", "energy", "duration"):
        names = sorted(real(os.path.join(pre_b, kind)))
        assert names and sorted(real(os.path.join(pre_a, kind))) == names, kind
        for name in names:
            got, ref = np.load(os.path.join(pre_a, kind, name)), np.load(os.path.join(pre_b, kind, name))
            assert got.shape == ref.shape and got.dtype == ref.dtype, (kind, name, got.shape, ref.shape)
            if kind == "duration":
                assert np.array_equal(got, ref), name
            elif kind == "mel":
                assert np.abs(got - ref).max() <= 2e-4, (name, float(np.abs(got - ref).max()))
            else:
                np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4, err_msg=name)
