"""F0 specification (fastspeech2_amd/pitch.py) without a GPU: the numpy oracle tests/f0_ref.py passes the known-answer bars,
DIO's frame count, the Preprocessor's pitch="gpu" guard and preprocess.py's --pitch resolution."""
import sys
import types

import numpy as np
import pytest

from fastspeech2_amd import pitch
from fastspeech2_amd import preprocess as P
from tests import f0_ref as R
from tests.f0_signals import (FRAME_PERIOD, FS, HOP, TONE_F0, far_from_signal, glide, interior, tone, tones_with_silence)
from tests.helpers import make_raw_corpus


@pytest.mark.parametrize("f0", TONE_F0)
def test_oracle_constant_tones(f0):
    x = tone(f0)
    f, _, t = R.dio_stonemask(x, FS, FRAME_PERIOD)
    v = f[interior(t, len(x))]
    assert np.mean(v > 0) >= 0.98
    assert np.all(np.abs(v[v > 0] / f0 - 1) <= 0.005)


def test_oracle_glide_and_silence():
    x, true = glide()
    f, _, t = R.dio_stonemask(x, FS, FRAME_PERIOD)
    m = interior(t, len(x))
    assert np.mean((f[m] > 0) & (np.abs(f[m] / true(t[m]) - 1) <= 0.02)) >= 0.95
    x = tones_with_silence()
    f, _, t = R.dio_stonemask(x, FS, FRAME_PERIOD)
    far = far_from_signal(x, t)
    assert far.sum() >= 10 and np.all(f[far] == 0)
    f, _, t = R.dio_stonemask(np.zeros(5000, np.float32), FS, FRAME_PERIOD)
    assert np.all(f == 0)


def test_frame_count_formula():
    fp = HOP / FS * 1000
    for k in (0, 1, 2, 3, 7, 86, 100, 861, 1000, 4321):
        for n in (k * HOP - 1, k * HOP, k * HOP + 1):
            if n < 0:
                continue
            want = 1 + int(n / FS / (fp / 1000))
            assert pitch.frame_count(n, FS, fp) == want
            assert want in (n // HOP + 1, n // HOP)                 # float rounding may land one below at exact multiples
    # at exact hop multiples the double expression decides: both outcomes occur
    exact = [pitch.frame_count(k * HOP, FS, fp) - (k + 1) for k in range(1, 2000)]
    assert set(exact) <= {0, -1}
    assert pitch.frame_count(0, FS, fp) == 1 and pitch.frame_count(HOP - 1, FS, fp) == 1


def test_constants():
    assert pitch.bands() == [71.0 * 2 ** ((i + 1) / 2) for i in range(7)]
    assert [pitch.matlab_round(FS / b / 2) for b in pitch.bands()] == [110, 78, 55, 39, 27, 19, 14]
    g = pitch.lowcut_taps(FS)
    assert len(g) == 883 and abs(g.sum()) < 1e-12 and np.allclose(g, g[::-1])
    assert pitch.voice_range_minimum(FRAME_PERIOD) == 3
    assert abs(pitch.nuttall(440).sum() - 1) < 1e-12


def test_preprocessor_gpu_pitch_on_cpu_fails_loudly(tmp_path):
    cfg, _ = make_raw_corpus(str(tmp_path))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.Preprocessor(cfg, device="cpu", pitch="gpu")
    with pytest.raises(ValueError):
        P.Preprocessor(cfg, device="cpu", pitch="cpu")
    with pytest.raises(ValueError):
        P.Preprocessor(cfg, pitch="gpu", pitch_fn=lambda w, s, h: None)


def test_cli_pitch_resolution(monkeypatch):
    monkeypatch.setitem(sys.modules, "pyworld", None)                 # import pyworld -> ImportError
    assert P.resolve_pitch("auto") == "gpu"
    assert P.resolve_pitch("gpu") == "gpu" and P.resolve_pitch("pyworld") is None
    fake = types.ModuleType("pyworld")
    fake.dio = lambda x, fs, frame_period: (np.zeros(3), np.zeros(3))
    fake.stonemask = lambda x, f0, t, fs: f0
    monkeypatch.setitem(sys.modules, "pyworld", fake)
    assert P.resolve_pitch("auto") is None
    assert P.resolve_pitch("gpu") == "gpu"
    with pytest.raises(ValueError):
        P.resolve_pitch("harvest")
