"""The host side of the harmonics-to-noise ratio (fastspeech2_amd/hnr.py) and the numpy restatement tests/hnr_ref.py, without a GPU:
the window and its autocorrelation table, the refusals, the row and summary rules with their NaN handling, the specification's known
answers on the restatement (each is verified here before tests/test_hnr_gpu.py holds a kernel to it), and `batch_bytes`."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import hnr as H
from fastspeech2_amd import metrics as M
from tests import hnr_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
LD = np.longdouble
FS, HOP = 22050, 256
TONES = (100.0, 147.0, 220.5, 300.0)


# ------------------------------------------------------------------------------------------------ window and table
def test_window_sizes_and_constants():
    assert H.window(22050) == (698, 1397, 312) and H.window(4000) == (126, 253, 58) and H.window(48000)[2] == 678
    for fs in (4000, 16000, 22050, 44100, 48000, 129000):
        assert H.window(fs) == ref.window(fs)
    assert (H.F0_FLOOR, H.F0_CEIL, H.PERIODS, H.SEARCH, H.R_LO, H.R_HI, H.SILENT) == (71.0, 800.0, 4.5, 1.2, 1e-3, 1 - 1e-6, 1e-20)
    assert (H.F0_FLOOR, H.F0_CEIL, H.SEARCH, H.R_LO, H.R_HI, H.SILENT) == (ref.F0_FLOOR, ref.F0_CEIL, ref.SEARCH, ref.R_LO, ref.R_HI, ref.SILENT)
    assert 10 * math.log10(H.R_LO / (1 - H.R_LO)) == pytest.approx(-30, abs=0.01) and 10 * math.log10(H.R_HI / (1 - H.R_HI)) == pytest.approx(60, abs=0.01)


@pytest.mark.parametrize("fs", (4000, 22050))
def test_the_table_is_the_sampled_windows_own_autocorrelation(fs):
    h, N, lmax = H.window(fs)
    w, rw = H.tables(fs)
    assert w.shape == (N,) and rw.shape == (lmax + 1,) and w.dtype == rw.dtype == np.float64
    assert rw[0] == 1.0 and np.all(rw > 0) and np.all(np.diff(rw) < 0) and np.all(w > 0) and w[h] == w.max()
    # symmetric about the centre sample, and the longdouble window, up to the rounding of the cosine's argument: an argument of up
    # to 2 pi carries an error of up to 2 pi EPS / 2, which the cosine passes on at most in full and the factor 0.5 halves
    assert np.abs(w - w[::-1]).max() <= 2 * math.pi * EPS
    wl, rwl = ref.tables(fs, LD)
    assert np.abs(w - wl).max() <= 2 * math.pi * EPS
    for tau in (1, lmax // 2, lmax):                                        # the definition is symmetric in the two factors
        assert rw[tau] == pytest.approx(float(np.dot(w[tau:], w[:N - tau]) / np.dot(w, w)), abs=4 * EPS)
    assert np.abs(rw - rwl).max() <= 8 * EPS and np.abs(ref.tables(fs)[1] - rwl).max() <= 8 * EPS
    # built from the samples, not from the closed form of the Hann window's autocorrelation (Boersma 1993, as remembered), which is an
    # integral: a sum of N samples of a window whose slope vanishes at both ends departs from its integral in the fourth order of the
    # step (Euler-Maclaurin), here taken as (2 pi / N)^4; at 4 kHz that departure is far above rounding, and it is in the table
    x = np.arange(lmax + 1) / (N + 1.0)
    analytic = (1 - x) * (2 / 3 + np.cos(2 * np.pi * x) / 3) + np.sin(2 * np.pi * x) / (2 * np.pi)
    assert np.abs(rw - analytic).max() <= (2 * math.pi / N) ** 4 and (fs != 4000 or np.abs(rw - analytic).max() > 1000 * N * EPS)


# ------------------------------------------------------------------------------------------------ refusals
def test_rates_and_host_tensors_are_refused_before_any_launch():
    for fs in (200000, 50, 22050.5, 0, -4000):
        with pytest.raises(ValueError):
            H.window(fs)
        with pytest.raises(ValueError):
            H.tables(fs)
    y, f0 = torch.zeros(1, 4000), torch.zeros(1, 16, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        H.frames(y, [4000], f0, [16], FS, HOP)
    with pytest.raises(ValueError):
        H.frames(y, [4000], f0, [16], 200000, HOP)
    with pytest.raises(ValueError):
        H.frames(y, [4000], f0, [16], FS, 0)
    with pytest.raises(ValueError, match="GPU"):
        H.side(torch.zeros(1, 16, 3, dtype=torch.float64), [16])
    with pytest.raises(ValueError, match="GPU"):
        H.on_path(torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.int32), torch.ones(1, dtype=torch.int32),
                  torch.zeros(1, 2, 3, dtype=torch.float64), [2], torch.zeros(1, 2, 3, dtype=torch.float64), [2])
    wav = [np.zeros(4000, np.float32)]
    with pytest.raises(ValueError, match="harmonics"):
        M.score_pairs(wav, wav, None, FS, HOP, f0=False, hnr=True)
    with pytest.raises(ValueError, match="hnr"):
        M.run({"preprocessing": {"audio": {"sampling_rate": FS}, "stft": {"hop_length": HOP}}}, "/nowhere", "/nowhere/val.txt", f0=False, hnr=True)
    with pytest.raises(ValueError):
        M.run({"preprocessing": {"audio": {"sampling_rate": 200000}, "stft": {"hop_length": HOP}}}, "/nowhere", "/nowhere/val.txt", hnr=True)


def test_batch_bytes_grows_by_28_bytes_per_frame_and_side():
    for n, T1, T2 in ((1, 1, 1), (32, 800, 900), (3, 2048, 17)):
        plain = M.batch_bytes(n, T1, T2, 13, 256, 0, True, True, True)
        assert M.batch_bytes(n, T1, T2, 13, 256, 0, True, True, True, hnr=True) - plain == n * (T1 + T2) * 28
        assert M.batch_bytes(n, T1, T2, 13, 256, 0, True, True, True, hnr=False) == plain
    assert M.HNR_FRAME_BYTES == H.FRAME_BYTES == 3 * 8 + 4


def test_a_score_fn_receives_the_switch_as_a_keyword(tmp_path):
    seen = {}

    def score_fn(r, s, **kw):
        seen.update(kw)
        return []

    src = tmp_path / "val.txt"
    src.write_text("")
    cfg = {"preprocessing": {"audio": {"sampling_rate": FS}, "stft": {"hop_length": HOP, "filter_length": 1024}},
           "path": {"raw_path": str(tmp_path), "preprocessed_path": str(tmp_path)}}
    M.run(cfg, str(tmp_path), str(src), score_fn=score_fn, hnr=True)
    assert seen == {}                                                       # no item: the stage is not called at all
    src.write_text("u0|spk|{AA}|t\n")
    from scipy.io import wavfile
    os.makedirs(tmp_path / "spk")
    for p in (tmp_path / "spk" / "u0.wav", tmp_path / "u0.wav"):
        wavfile.write(str(p), FS, np.zeros(4000, np.int16))
    row = {"mcd_db": 1.0, "path_len": 5, "frames_ref": 4, "frames_syn": 4, **H.row_scores([3, 1.0, 2.0, 4.0, 4.0, 2.0, 6.0], [4, 1.0, 8.0], [4, 2.0, 8.0])}
    rows, _, summary = M.run(cfg, str(tmp_path), str(src), score_fn=lambda r, s, **kw: seen.update(kw) or [dict(row)], hnr=True, wavelet=True)
    assert seen == {"hnr": True, "wavelet": True} and rows[0]["hnr_cells"] == 3 and summary["hnr_unscored_utterances"] == 0


# ------------------------------------------------------------------------------------------------ rows and summary
def test_row_rules_and_their_nan_handling():
    row = H.row_scores([100, 10.0, 12.5, 400.0, 100.0, 100.0, 900.0], [120, 10.5, 480.0], [110, 12.0, 110.0])
    assert tuple(row) == H.row_keys() == ref.KEYS
    assert row == {"hnr_mean_db_ref": 10.5, "hnr_mean_db_syn": 12.0, "hnr_std_db_ref": 2.0, "hnr_std_db_syn": 1.0, "hnr_frames_ref": 120,
                   "hnr_frames_syn": 110, "hnr_cells": 100, "hnr_diff_db": 2.5, "hnr_rmse_db": 3.0, "hnr_corr": 0.5}
    none = H.row_scores([0.0] * 7, [5, 3.0, 0.0], [0, 0.0, 0.0])
    assert none["hnr_cells"] == 0 and all(math.isnan(none[k]) for k in ("hnr_diff_db", "hnr_rmse_db", "hnr_corr", "hnr_mean_db_syn", "hnr_std_db_syn"))
    assert none["hnr_mean_db_ref"] == 3.0 and none["hnr_std_db_ref"] == 0.0 and none["hnr_frames_syn"] == 0
    one = H.row_scores([1, 4.0, 6.0, 0.0, 0.0, 0.0, 4.0], [1, 4.0, 0.0], [1, 6.0, 0.0])
    assert one["hnr_diff_db"] == 2.0 and one["hnr_rmse_db"] == 2.0 and math.isnan(one["hnr_corr"])
    flat = H.row_scores([50, 4.0, 6.0, 50 * 1e-24, 3.0, 0.0, 9.0], [50, 4.0, 0.0], [50, 6.0, 3.0])          # Sxx at the floor of cwt_corr
    assert math.isnan(flat["hnr_corr"]) and flat["hnr_rmse_db"] == math.sqrt(9.0 / 50)
    assert H.CORR_FLOOR == M.CORR_FLOOR


def test_summary_rules_and_their_nan_handling():
    a = H.row_scores([100, 10.0, 12.0, 400.0, 100.0, 100.0, 900.0], [100, 10.0, 400.0], [300, 12.0, 100.0])
    b = H.row_scores([300, 20.0, 18.0, 1.0, 1.0, 1.0, 300.0], [300, 20.0, 0.0], [100, 16.0, 0.0])
    c = H.row_scores([0.0] * 7, [0, 0.0, 0.0], [7, 1.0, 0.0])
    d = H.row_scores([1, 4.0, 6.0, 0.0, 0.0, 0.0, 4.0], [1, 4.0, 0.0], [1, 6.0, 0.0])
    out = H.summarize([a, b, c, d])
    assert out["hnr_frames_ref"] == 401 and out["hnr_frames_syn"] == 408 and out["hnr_cells"] == 401
    assert out["hnr_mean_db_ref"] == (10.0 * 100 + 20.0 * 300 + 4.0) / 401 and out["hnr_mean_db_syn"] == (12.0 * 300 + 16.0 * 100 + 7.0 + 6.0) / 408
    assert out["hnr_diff_db"] == pytest.approx((2.0 * 100 - 2.0 * 300 + 2.0) / 401, abs=1e-14)
    assert out["hnr_rmse_db"] == pytest.approx(math.sqrt((900.0 + 300.0 + 4.0) / 401), abs=1e-14)
    assert out["hnr_corr_mean"] == 0.75 and out["hnr_corr_nan_utterances"] == 2 and out["hnr_unscored_utterances"] == 1
    only = H.summarize([c])
    assert only["hnr_unscored_utterances"] == 1 and only["hnr_cells"] == 0 and only["hnr_frames_ref"] == 0
    assert all(math.isnan(only[k]) for k in ("hnr_mean_db_ref", "hnr_diff_db", "hnr_rmse_db", "hnr_corr_mean")) and only["hnr_mean_db_syn"] == 1.0
    merged = M.summarize([dict(a, path_len=120, mcd_db=1.0), dict(c, path_len=9, mcd_db=2.0)])
    assert merged["hnr_unscored_utterances"] == 1 and "hnr_cells" not in M.summarize([{"path_len": 3, "mcd_db": 1.0}])


# ------------------------------------------------------------------------------------------------ the known answers
def _interior(T):
    """the frames whose window lies inside a signal of T - 1 hops: four frames from either end at 22050 Hz, hop 256"""
    return slice(4, T - 4)


@pytest.mark.parametrize("f", TONES)
def test_known_answer_a_tone_in_white_noise_scores_its_snr(f):
    rng = np.random.default_rng(9701)
    T = ref.n_frames(FS, HOP)
    track = np.full(T, f)
    for snr in (20.0, 10.0, 0.0):
        fr = ref.frames(ref.tone(f, FS, FS, rng, snr), track, FS, HOP)[0][_interior(T)]
        assert len(fr) >= 20 and fr[:, 2].all()
        print(f"{f} Hz at {snr} dB: mean HNR {fr[:, 1].mean():.3f} dB over {len(fr)} frames")
        assert abs(fr[:, 1].mean() - snr) <= 1.0
    clean = ref.frames(ref.tone(f, FS, FS), track, FS, HOP)[0][_interior(T)]
    print(f"{f} Hz clean: min HNR {clean[:, 1].min():.2f} dB")
    assert clean[:, 2].all() and clean[:, 1].min() >= 30.0


def test_known_answer_white_noise_is_far_below_zero():
    rng = np.random.default_rng(9702)
    y = (0.1 * rng.standard_normal(FS)).astype(np.float32)
    T = ref.n_frames(FS, HOP)
    fr = ref.frames(y, np.full(T, 150.0), FS, HOP)[0][_interior(T)]
    print(f"white noise at 150 Hz: mean HNR {fr[:, 1].mean():.2f} dB, max {fr[:, 1].max():.2f} dB")
    assert fr[:, 2].all() and fr[:, 1].mean() < -5.0


def test_unvoiced_silent_and_unsearchable_frames_are_invalid():
    y = ref.tone(150.0, 6000, FS)
    for f0 in (0.0, -1.0, float("nan"), 1e-300, 30.0, 20000.0):              # 30 Hz: l0 above LMAX - 1; 20 kHz: l1 = 1 below l0 = 2
        q = ref.frame(y, 10, f0, FS, HOP)
        assert (q["r"], q["hnr"], q["valid"], q["lag"]) == (0, 0, 0, 0)
    assert ref.frame(np.zeros(6000, np.float32), 10, 150.0, FS, HOP)["valid"] == 0
    assert ref.frame(np.full(6000, 0.25, np.float32), 10, 150.0, FS, HOP)["valid"] == 0      # a constant: its mean goes, nothing is left
    q = ref.frame(y, 10, 150.0, FS, HOP)
    assert q["valid"] == 1 and q["lag"] == 147 and ref.frame(y, 10, ref.F0_FLOOR, FS, HOP)["lag"] <= ref.window(FS)[2] - 1



def test_a_pair_against_itself_and_noise_added_to_the_synthesized_side():
    rng = np.random.default_rng(9703)
    y = np.concatenate([ref.tone(f, FS // 3, FS, rng, 35.0) for f in (120.0, 180.0, 150.0)])
    T = ref.n_frames(len(y), HOP)
    f0 = np.repeat([120.0, 180.0, 150.0], -(-T // 3))[:T]
    f0[::17] = 0.0
    same = ref.pair_scores(y, f0, y.copy(), f0, FS, HOP)
    assert same["hnr_diff_db"] == 0 and same["hnr_rmse_db"] == 0 and abs(same["hnr_corr"] - 1) <= 4 * EPS
    assert same["hnr_cells"] == same["hnr_frames_ref"] == int((f0 > 0).sum()) and same["hnr_mean_db_ref"] == same["hnr_mean_db_syn"]
    means, diffs = [same["hnr_mean_db_syn"]], [0.0]
    for snr in (30.0, 20.0, 10.0):
        row = ref.pair_scores(y, f0, ref.noisier(y, rng, snr), f0, FS, HOP)
        print(f"noise at {snr} dB on the synthesized side: mean {row['hnr_mean_db_syn']:.2f} dB, diff {row['hnr_diff_db']:.2f} dB")
        means.append(row["hnr_mean_db_syn"])
        diffs.append(row["hnr_diff_db"])
        assert row["hnr_mean_db_ref"] == same["hnr_mean_db_ref"] and row["hnr_rmse_db"] >= abs(row["hnr_diff_db"])
    assert all(b < a for a, b in zip(means, means[1:])) and all(b < a for a, b in zip(diffs, diffs[1:])) and diffs[1] < 0
    # the host's rows agree with the restatement's on the same sums
    fa = ref.frames(y, f0, FS, HOP)[0]
    k = np.arange(T)
    host = H.row_scores(ref.path_sums(k, k, fa, fa), ref.side(fa), ref.side(fa))
    assert host == {key: (int(v) if isinstance(v, (int, np.integer)) else float(v)) for key, v in same.items()}


# ------------------------------------------------------------------------------------------------ the bars
def test_the_two_restatements_agree_and_the_bars_file_is_current():
    bars = json.load(open(os.path.join(ROOT, "tests", "golden", "hnr_bars.json")))
    assert bars["factor"] == 16 and set(bars["distance"]) == set(ref.CASES) | set(ref.PATH_CASES)
    assert bars["cases"] == {k: {"fs": v[0], "hop": v[1], "seed": v[2], "rows": [list(r) for r in v[3]]} for k, v in ref.CASES.items()}
    assert 100 * sum(bars["left_out"].values()) <= sum(bars["valid_frames"].values())
    fs, hop, rows = ref.case_input("fs4000")
    valid = 0
    for y, f0 in rows:
        fr, lag, rp, _ = ref.frames(y, f0, fs, hop)
        frl, lagl, rpl, _ = ref.frames(y, f0, fs, hop, LD, lags=lag)
        assert np.array_equal(lag, lagl) and float(np.abs(fr[:, 1] - frl[:, 1]).max()) <= bars["distance"]["fs4000"]["hnr"]
        assert float(np.nanmax(np.abs(rp - rpl))) <= bars["distance"]["fs4000"]["rprime"]
        valid += int(fr[:, 2].sum())
    assert valid == bars["valid_frames"]["fs4000"]
    _, _, long_rows = ref.case_input("fs22050")
    fr = ref.frames(*long_rows[2], 22050, 256)[0]
    T = len(fr)
    assert not fr[3:6, 2].any() and not fr[9, 2] and fr[7, 2] and fr[8, 2] and not fr[27:33, 2].any() and fr[26, 2] and fr[T - 2, 2]
    assert all(v > 0 for v in bars["distance"]["fs22050"].values()) and bars["distance"]["none_shared"] == {"path_mean": 0.0, "path_sums": 0.0}
