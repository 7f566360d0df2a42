"""Known-answer signals and the ragged batches of the spectral-envelope tests (tests/test_world_cpu.py, tests/test_world_gpu.py) and
of the script that measures their bars (tests/golden/make_world_bars.py): all-pole filters with known poles, their exact cepstra,
band-limited pulse trains in their steady state, and hand-written F0 rows that reach every branch of the envelope's specification."""
import json
import os

import numpy as np

FS, HOP = 22050, 256
FRAME_PERIOD = HOP / FS * 1000
BARS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_bars.json")
FORMANTS = {2: ((900.0, 250.0),), 8: ((700.0, 180.0), (1300.0, 220.0), (2700.0, 300.0), (3800.0, 350.0))}      # (centre, bandwidth) Hz
PITCHES = (120.0, 220.0)


def bars():
    with open(BARS_PATH) as f:
        return json.load(f)


def poles(order, fs=FS):
    p = np.array([np.exp(-np.pi * bw / fs + 2j * np.pi * fc / fs) for fc, bw in FORMANTS[order]])
    return np.concatenate([p, p.conj()])


def response(order, w, fs=FS):
    """H(e^{iw}) = 1 / prod_p (1 - p e^{-iw}): minimum phase, all poles inside the unit circle"""
    z = np.exp(-1j * np.asarray(w, np.float64))
    return 1.0 / np.prod(1.0 - poles(order, fs)[:, None] * z[None, :], axis=0)


def exact_cepstrum(order, M, fs=FS):
    """c_0 .. c_M with ln |H(w)| = sum_q c_q cos(q w): c_0 = 0, c_q = sum_p p^q / q"""
    q = np.arange(1, M + 1)
    c = np.zeros(M + 1)
    c[1:] = np.sum(poles(order, fs)[:, None] ** q[None, :], axis=0).real / q
    return c


def pulse_train(f0, order=8, dur=0.5, fs=FS):
    """every harmonic of f0 below Nyquist at amplitude |H| and phase arg H: the steady-state response of H to a band-limited pulse
    train, peak 0.5, float32"""
    n = np.arange(int(dur * fs))
    h = np.arange(1, int(np.ceil(fs / 2.0 / f0)))
    w = 2.0 * np.pi * f0 * h / fs
    H = response(order, w, fs)
    x = np.sum(np.abs(H)[:, None] * np.cos(w[:, None] * n[None, :] + np.angle(H)[:, None]), axis=0)
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def frame_count(n, fs, frame_period):
    return 1 + int(n / fs / (frame_period / 1000))


def ragged_case():
    """fs = 22050 (N = 1024, F0 limit 64.8 Hz): one sample; shorter than one window; two ordinary rows.  -> (rows, f0 rows)"""
    rng = np.random.RandomState(7)
    lens = [1, 300, 5000, 4097]
    src = pulse_train(180.0, dur=0.3)
    rows = [(src[1000:1000 + n] + 2e-3 * rng.randn(n)).astype(np.float32) for n in lens]
    frames = [frame_count(n, FS, FRAME_PERIOD) for n in lens]
    assert frames == [1, 2, 20, 17]
    f0 = [np.array([0.0]),
          np.array([65.0, 800.0]),                                          # both windows clamped at both ends of 300 samples
          np.array([65.0, 0.0, 64.0, 800.0, 65.0] + [180.0, 181.5, 0.0, 240.25, 64.79, 64.80, 500.0, 2756.25, 2756.3, 99.9,
                                                     130.0, 71.0, 400.0, 180.0, 65.0]),
          np.array([180.0] * 8 + [0.0] + [123.4, 333.3, 65.0, 799.9, 180.0, 64.0, 250.0, 65.0])]
    assert [len(v) for v in f0] == frames
    return rows, f0


def wide_case():
    """fs = 48000 (N = 2048), frame period 5 ms"""
    rng = np.random.RandomState(11)
    fs, n = 48000, 2500
    x = (pulse_train(100.0, dur=n / fs + 0.01, fs=fs)[:n] + 2e-3 * rng.randn(n)).astype(np.float32)
    return fs, 5.0, [x], [np.full(frame_count(n, fs, 5.0), 100.0)]


# ------------------------------------------------------------------------------------------------ measurements on the oracle
def envelope_error_db(f0, order=8):
    """RMS over frames and over the bins from f0 to 0.9 Nyquist of (10 log10 envelope - 20 log10 |H|) with its mean over those
    bins removed per frame; frames whose window reaches past either end of the signal are left out"""
    from tests import world_ref as W
    x = pulse_train(f0, order)
    F = frame_count(len(x), FS, FRAME_PERIOD)
    env = W.envelope(x, np.full(F, f0), FS, FRAME_PERIOD)
    n = W.fft_size(FS)
    k = np.arange(n // 2 + 1)
    sel = (k * FS / n >= f0) & (k * FS / n <= 0.9 * FS / 2)
    want = 20.0 * np.log10(np.abs(response(order, 2.0 * np.pi * k[sel] / n)))
    half = int(1.5 * FS / f0 + 0.5)
    inside = [f for f in range(F) if f * HOP - half >= 0 and f * HOP + half < len(x)]
    d = 10.0 * np.log10(env[inside][:, sel]) - want[None, :]
    d -= d.mean(axis=1, keepdims=True)
    return float(np.sqrt(np.mean(d * d)))


def log_mel(x):
    """the project's natural-log mel of the test configuration, in numpy float64: (n_mel, frames)"""
    from fastspeech2_amd.audio import slaney_mel_filterbank
    from tests import gl_ref
    from tests.test_align_cpu import config
    pp = config("/nowhere")["preprocessing"]
    assert pp["audio"]["sampling_rate"] == FS and pp["stft"]["hop_length"] == HOP
    stft = gl_ref.STFT(pp["stft"]["filter_length"], HOP, pp["stft"]["win_length"])
    basis = np.asarray(slaney_mel_filterbank(FS, pp["stft"]["filter_length"], pp["mel"]["n_mel_channels"], pp["mel"]["mel_fmin"],
                                             pp["mel"]["mel_fmax"]), np.float64)
    mag, _ = stft.transform(np.clip(np.asarray(x, np.float64), -1.0, 1.0)[None, :])
    return np.log(np.maximum(basis @ mag[0], 1e-5))


def pair_mcds(order=8):
    """the 120 / 220 Hz renderings through one filter: (world MCD at the true F0, K = 24, tabulated alpha; mel-DCT MCD, K = 13;
    frames per side; world path length)"""
    from tests import dtw_ref as R
    from tests import world_ref as W
    xs = [pulse_train(f, order) for f in PITCHES]
    F = frame_count(len(xs[0]), FS, FRAME_PERIOD)
    ca, cb = (W.world_cepstra(x, np.full(F, f), FS, FRAME_PERIOD) for x, f in zip(xs, PITCHES))
    total, pi, pj = R.dtw(ca, cb)
    world = R.scores(total, pi, pj, F, F)
    ma, mb = (log_mel(x)[:, :F] for x in xs)
    mel = R.score_pair(ma, mb)
    return world["mcd_db"], mel["mcd_db"], F, world["path_len"]
