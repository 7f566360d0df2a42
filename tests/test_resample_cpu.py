"""Sample-rate conversion and prepare_align without a GPU: the numpy oracle (tests/resample_ref.py) against scipy's polyphase
resampler, the product's tap builder (fastspeech2_amd/resample.py), the corpus walkers / text / file layout of
fastspeech2_amd/prepare_align.py through its `audio_fn` seam, and the host-side pieces of `Preprocessor(resample="gpu")`."""
import os

import numpy as np
import pytest
from scipy.io import wavfile
from scipy.signal import firwin, resample_poly

from fastspeech2_amd import preprocess as P
from fastspeech2_amd import prepare_align as PA
from fastspeech2_amd import resample as R
from tests import resample_corpus as C
from tests.helpers import fake_pitch, make_raw_corpus
from tests.resample_ref import factors, resample_ref

PAIRS = [(24000, 22050), (44100, 22050), (48000, 22050), (16000, 22050), (22050, 24000)]


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_reference_equals_scipy_resample_poly(sr_in, sr_out):
    """two fp64 summation orders over <= 45 terms with sum |h_phase| about 2 differ by about 2e-14 max|x|; 1e-12 is headroom"""
    rng = np.random.default_rng(sr_in + sr_out)
    up, down = factors(sr_in, sr_out)
    for n in (1, 2, 37, 4001):
        x = rng.standard_normal(n)
        y, z = resample_ref(x, sr_in, sr_out), resample_poly(x, up, down)
        assert y.dtype == np.float64 and len(y) == len(z) == -(-n * up // down), (n, len(y), len(z))
        assert np.abs(y - z).max() <= 1e-12 * np.abs(x).max(), (n, np.abs(y - z).max())


@pytest.mark.parametrize("sr_in,sr_out", PAIRS + [(11025, 32000), (48000, 8000)])
def test_tap_builder_and_phase_table(sr_in, sr_out):
    up, down = R.ratio(sr_in, sr_out)
    assert (up, down) == factors(sr_in, sr_out)
    h, half = R.filter_taps(up, down)
    m = max(up, down)
    assert half == 10 * m and h.dtype == np.float64
    assert np.array_equal(h, up * firwin(2 * half + 1, 1.0 / m, window=("kaiser", 5.0)))        # exactly, not approximately
    tab = R.phase_table(h, up)
    T = tab.shape[1]
    assert tab.shape[0] == up and T % 2 == 0 and T in (-(-len(h) // up), -(-len(h) // up) + 1) and tab.flags["C_CONTIGUOUS"]
    # a permutation of h padded with zeros: tab[p][s] = h[p + (T - 1 - s) up]
    k = np.arange(up)[:, None] + (T - 1 - np.arange(T))[None, :] * up
    inside = k < len(h)
    assert np.array_equal(tab[inside], h[k[inside]]) and not tab[~inside].any()
    assert np.array_equal(np.sort(k[inside]), np.arange(len(h)))
    # and the dot-product form of the module docstring gives the specified sum
    rng = np.random.default_rng(1)
    x = rng.standard_normal(300)
    ref = resample_ref(x, sr_in, sr_out)
    xp = np.concatenate([np.zeros(T), x, np.zeros(T + half // up + 2)])
    for j in (0, 1, len(ref) // 2, len(ref) - 1):
        p, q = (j * down + half) % up, (j * down + half) // up
        assert abs(tab[p] @ xp[q + 1:q + 1 + T] - ref[j]) <= 1e-12 * np.abs(x).max(), j


def test_ratio_limits_and_input_span():
    assert R.ratio(22050, 22050) == (1, 1)
    assert np.array_equal(R.phase_table(*[R.filter_taps(1, 1)[0], 1]), [[0.0, 1.0]])          # same rate: the identity filter
    with pytest.raises(ValueError):
        R.ratio(0, 22050)
    with pytest.raises(ValueError):
        R.ratio(22050, 65537 * 3)                                                            # coprime, factor above the limit
    up, down = 147, 160
    h, half = R.filter_taps(up, down)
    n_in = 5000
    for a, n in ((0, 10), (1000, 500), (4500, R.out_length(n_in, up, down) - 4500)):
        lo, hi = R.input_span(a, n, n_in, up, down)
        i = np.arange(n_in)
        used = np.zeros(n_in, bool)
        for j in (a, a + n - 1):
            k = j * down - i * up + half
            used |= (k >= 0) & (k <= 2 * half)
        assert 0 <= lo <= hi <= n_in and lo <= np.nonzero(used)[0].min() and hi > np.nonzero(used)[0].max()
        assert hi - lo <= n * down // up + 2 * half // up + 3                                 # only the span the window needs
    assert R.input_span(5, 0, n_in, up, down) == (0, 0)


def test_gpu_functions_refuse_cpu_tensors():
    import torch
    x = torch.zeros(1, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.resample_poly(x, [8], 24000, 22050)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.peak_abs(x, [8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.peaknorm_pcm(x, [8], torch.ones(1), 32768.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PA.prepare_align(C.config("LJSpeech", "nowhere", "nowhere"), device="cpu")
    from fastspeech2_amd import audio
    assert audio.resample_poly is R.resample_poly and audio.peak_abs is R.peak_abs and audio.peaknorm_pcm is R.peaknorm_pcm


@pytest.mark.parametrize("layout", ["ljspeech", "libritts", "aishell3"])
def test_prepare_align_layouts_with_injected_audio_fn(tmp_path, layout):
    cfg, wavs, labs = {"ljspeech": C.make_ljspeech, "libritts": C.make_libritts, "aishell3": C.make_aishell3}[layout](str(tmp_path))
    calls = []

    def audio_fn(ws, sr_in, sr_out, max_wav_value):
        calls.append((sr_in, sr_out, max_wav_value, [len(w) for w in ws]))
        assert all(w.dtype == np.float32 and w.ndim == 1 for w in ws)
        return C.ref_audio_fn(ws, sr_in, sr_out, max_wav_value)

    n = PA.prepare_align(cfg, device="cpu", audio_fn=audio_fn, num_workers=2)
    raw = cfg["path"]["raw_path"]
    assert n == len(wavs)
    assert C.listing(raw) == sorted(list(wavs) + list(labs))                                 # a missing wav leaves no .wav and no .lab
    for path, text in labs.items():
        assert open(path, encoding="utf-8").read() == text, path
    for path, (x, sr) in wavs.items():
        rate, pcm = wavfile.read(path)
        assert rate == 22050 and pcm.dtype == np.int16 and pcm.ndim == 1, (path, rate, pcm.dtype)
        assert np.array_equal(pcm, C.ref_audio_fn([x], sr, 22050, 32768.0)[0]), path
        assert len(pcm) == -(-len(x) * 22050 // sr) and np.abs(pcm.astype(np.int32)).max() >= 32767
    # one source rate per batch, every utterance exactly once, each batch longest first
    rates = sorted(sr for _, sr in wavs.values())
    assert sorted(c[0] for c in calls for _ in c[3]) == rates and len(calls) == len(set(rates))
    assert all(c[1] == 22050 and c[2] == 32768.0 and c[3] == sorted(c[3], reverse=True) for c in calls)
    by_rate = {}
    for x, sr in wavs.values():
        by_rate.setdefault(sr, []).append(len(x))
    assert all(sorted(c[3]) == sorted(by_rate[c[0]]) for c in calls)


def test_prepare_align_packs_several_batches_and_rejects_unknown_corpus(tmp_path):
    cfg, wavs, _ = C.make_libritts(str(tmp_path))
    calls = []

    def audio_fn(ws, sr_in, sr_out, max_wav_value):
        calls.append((sr_in, len(ws)))
        return C.ref_audio_fn(ws, sr_in, sr_out, max_wav_value)

    assert PA.prepare_align(cfg, device="cpu", audio_fn=audio_fn, batch_seconds=0.6, num_workers=1) == 4
    assert sum(n for _, n in calls) == 4 and len(calls) >= 3, calls                          # 24 kHz rows split, 16 kHz row alone
    for path, (x, sr) in wavs.items():
        assert np.array_equal(wavfile.read(path)[1], C.ref_audio_fn([x], sr, 22050, 32768.0)[0]), path
    with pytest.raises(ValueError, match="LJSpeech, AISHELL3 and LibriTTS"):
        PA.prepare_align(C.config("VCTK", "a", "b"), audio_fn=audio_fn)


def test_prepare_align_warns_on_a_silent_file(tmp_path):
    cfg, wavs, _ = C.make_ljspeech(str(tmp_path))
    src = os.path.join(cfg["path"]["corpus_path"], "wavs", "LJ001-0002.wav")
    wavfile.write(src, 22050, np.zeros(500, np.int16))
    with pytest.warns(UserWarning, match="silent file"):
        PA.prepare_align(cfg, device="cpu", num_workers=1,
                         audio_fn=lambda ws, a, b, m: [np.zeros(len(w), np.int16) if not w.any() else C.ref_audio_fn([w], a, b, m)[0] for w in ws])
    assert not wavfile.read(os.path.join(cfg["path"]["raw_path"], "LJSpeech", "LJ001-0002.wav"))[1].any()


def test_preprocessor_gpu_resampling_needs_the_gpu_pitch_backend(tmp_path):
    cfg, _ = make_raw_corpus(str(tmp_path))
    with pytest.raises(ValueError, match="pitch='gpu'"):
        P.Preprocessor(cfg, device="cpu", resample="gpu", pitch=None)
    with pytest.raises(ValueError, match="pitch='gpu'"):
        P.Preprocessor(cfg, device="cpu", resample="gpu", pitch_fn=fake_pitch)
    with pytest.raises(ValueError, match="resample must be"):
        P.Preprocessor(cfg, device="cpu", resample="host", pitch_fn=fake_pitch)
    assert P.Preprocessor(cfg, device="cpu", pitch_fn=fake_pitch).resample is None            # the default: today's host path


def test_load_wav_keeps_the_native_rate_on_request(tmp_path):
    t = np.arange(4410) / 44100.0
    stereo = np.stack([np.sin(2 * np.pi * 200 * t), 0.5 * np.sin(2 * np.pi * 300 * t)], axis=1)
    wavfile.write(str(tmp_path / "s.wav"), 44100, (stereo * 20000).astype(np.int16))
    w, sr = P.load_wav(str(tmp_path / "s.wav"), resample=False)
    assert sr == 44100 and isinstance(sr, int) and w.dtype == np.float32 and w.shape == (4410,)
    mono = ((stereo * 20000).astype(np.int16).astype(np.float32) / 32768.0).mean(axis=1)
    assert np.array_equal(w, mono)
    # the default is untouched: resampled on the host with scipy's float32 path
    d = P.load_wav(str(tmp_path / "s.wav"))
    assert isinstance(d, np.ndarray) and np.array_equal(d, resample_poly(mono, 1, 2).astype(np.float32))
    assert np.array_equal(P.load_wav(str(tmp_path / "s.wav"), 44100), mono)
