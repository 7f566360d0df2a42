"""CPU: the host side of fastspeech2_amd/loudness.py (coefficients, block sizes, the chunked recursion's tables, the gain rule,
prepare_align's option checks) and the fp64 restatement tests/loudness_ref.py against the published answers of ITU-R BS.1770-4."""
import numpy as np
import pytest
from scipy.signal import lfilter

from fastspeech2_amd import loudness as L
from fastspeech2_amd import prepare_align as PA
from tests import loudness_ref as ref
from tests import resample_corpus as C

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz), as the bilinear re-parametrisation reproduces them
SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
SHELF_A = (1.0, -1.69065929318241, 0.73248077421585)
HP_B = (1.0, -2.0, 1.0)
HP_A = (1.0, -1.99004745483398, 0.99007225036621)


def _sine(fs, dur, amp=1.0, f=997.0):
    return amp * np.sin(2.0 * np.pi * f * np.arange(int(dur * fs)) / fs)


def test_k_weighting_is_the_standards_table_at_48_khz():
    (b1, a1), (b2, a2) = L.k_weighting(48000)
    for got, want in ((b1, SHELF_B), (a1, SHELF_A), (b2, HP_B), (a2, HP_A)):
        assert np.abs(np.asarray(got) - np.asarray(want)).max() <= 1e-12, (got, want)
    (b1, a1), (b2, a2) = ref.coefficients(48000)
    for got, want in ((b1, SHELF_B), (a1, SHELF_A), (b2, HP_B), (a2, HP_A)):
        assert np.abs(got - np.asarray(want)).max() <= 1e-12, (got, want)


@pytest.mark.parametrize("fs", [16000, 22050, 24000, 44100, 11025])
def test_k_weighting_equals_the_reference_at_other_rates(fs):
    for (b, a), (rb, ra) in zip(L.k_weighting(fs), ref.coefficients(fs)):
        assert np.abs(np.asarray(b) - rb).max() <= 1e-14 and np.abs(np.asarray(a) - ra).max() <= 1e-14
    with pytest.raises(ValueError):
        L.k_weighting(0)


def test_full_scale_997_hz_sine_reads_minus_3_01():
    loud = ref.loudness(_sine(48000, 3.0), 48000)
    print(f"997 Hz full scale at 48 kHz: {loud:.4f} LKFS")
    assert abs(loud - (-3.01)) <= 0.01
    assert abs(ref.loudness(_sine(48000, 3.0, amp=0.1), 48000) - (loud - 20.0)) <= 1e-9
    at_22k = ref.loudness(_sine(22050, 3.0), 22050)
    print(f"997 Hz full scale at 22.05 kHz: {at_22k:.4f} LKFS")
    assert abs(at_22k - (-2.981)) <= 0.01


def test_relative_gate_drops_the_quiet_part():
    fs = 22050
    x = np.concatenate([_sine(fs, 2.0), _sine(fs, 4.0, amp=0.01)])
    z = ref.block_energies(x, fs)
    loud, _, n_abs, n_rel, _ = ref.gated(z)
    print(f"gated {loud:.4f}, ungated {ref.ungated(x, fs):.4f}, blocks {len(z)} / {n_abs} / {n_rel}")
    assert abs(loud - (-3.32)) <= 0.01
    assert abs(ref.ungated(x, fs) - (-7.75)) <= 0.01
    assert n_abs == len(z) and 0 < n_rel < n_abs                         # the relative gate, not the absolute one, dropped blocks
    assert ref.gated(np.zeros(0))[0] != ref.gated(np.zeros(0))[0]           # no block: NaN
    assert ref.gated(np.zeros(5))[0] == float("-inf")


@pytest.mark.parametrize("chunk", [64, 2205])
def test_chunked_recursion_equals_lfilter(chunk):
    """zero-state chunks + scan of the end states with A^L + zero-input correction = the cascade over the whole row"""
    fs = 22050
    (b1, a1), (b2, a2) = L.k_weighting(fs)
    AL, R = L.chunk_tables(fs, chunk)
    assert AL.shape == (4, 4) and R.shape == (4, chunk)
    rng = np.random.default_rng(chunk)
    for n in (chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
        x = rng.standard_normal(n) * (1.0 + np.sin(np.arange(n) / 50.0))
        want = lfilter(b2, a2, lfilter(b1, a1, x))
        got, S = np.empty(n), np.zeros(4)
        for c0 in range(0, n, chunk):
            xc = x[c0:c0 + chunk]
            y1, zf1 = lfilter(b1, a1, xc, zi=np.zeros(2))
            y, zf2 = lfilter(b2, a2, y1, zi=np.zeros(2))
            got[c0:c0 + len(xc)] = y + S @ R[:, :len(xc)]
            S = np.concatenate([zf1, zf2]) + AL @ S                       # a short last chunk's state is not used
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (n, float(np.abs(got - want).max()))


def test_block_sizes_and_counts():
    assert L.block_sizes(11025) == (4410, 1102)                           # 4 h != n
    assert L.block_sizes(48000) == (19200, 4800) and L.block_sizes(22050) == (8820, 2205)
    for fs in (11025, 16000, 22050):
        n, h = L.block_sizes(fs)
        assert (n, h) == ref.sizes(fs)
        for length, want in ((n - 1, 0), (n, 1), (n + h - 1, 1), (n + h, 2), (0, 0)):
            assert L.n_blocks(length, fs) == want == len(ref.block_energies(np.ones(length), fs)), (fs, length)


def test_prepare_align_refuses_bad_options_before_reading(tmp_path):
    cfg = C.config("LibriTTS", str(tmp_path / "absent"), str(tmp_path / "raw"))
    with pytest.raises(ValueError, match="audio_fn"):
        PA.prepare_align(cfg, audio_fn=C.ref_audio_fn, normalize="loudness")
    for target in (-70.5, 0.5, float("nan")):
        with pytest.raises(ValueError, match="target_lufs"):
            PA.prepare_align(cfg, normalize="loudness", target_lufs=target)
    with pytest.raises(ValueError, match="ceiling_db"):
        PA.prepare_align(cfg, normalize="loudness", ceiling_db=0.5)
    with pytest.raises(ValueError, match="normalize"):
        PA.prepare_align(cfg, normalize="rms")
    assert not (tmp_path / "raw").exists()


def test_gain_rule():
    # the target is reached where the peak allows it
    g, limited, fallback = L.gain_rule(-30.0, 0.2, target=-23.0, ceiling_db=-1.0)
    assert abs(20 * np.log10(g) - 7.0) <= 1e-12 and not limited and not fallback
    # the ceiling binds: peak 0.5 times 7 dB would pass -1 dBFS
    g, limited, fallback = L.gain_rule(-30.0, 0.5, target=-23.0, ceiling_db=-1.0)
    assert abs(g * 0.5 - 10 ** (-1 / 20)) <= 1e-15 and limited and not fallback
    for loud in (float("nan"), float("-inf")):
        g, limited, fallback = L.gain_rule(loud, 0.25, target=-23.0, ceiling_db=-1.0)
        assert abs(g * 0.25 - 10 ** (-1 / 20)) <= 1e-15 and fallback and not limited
    g, limited, fallback = L.gain_rule(float("nan"), 0.0)
    assert g == 0.0 and fallback
    # arrays, and agreement with the restatement
    loud, peak = np.array([-30.0, -30.0, np.nan, -12.0]), np.array([0.2, 0.5, 0.25, 0.9])
    g, limited, fallback = L.gain_rule(loud, peak, -23.0, -1.0)
    for k in range(4):
        rg, rl, rf = ref.gain(loud[k], peak[k], -23.0, -1.0)
        assert abs(g[k] - rg) <= 1e-15 * rg and bool(limited[k]) == rl and bool(fallback[k]) == rf
    with pytest.raises(ValueError):
        L.check_options(target_lufs=1.0)
