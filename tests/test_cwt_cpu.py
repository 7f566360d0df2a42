"""The host side of the wavelet prosody scores (fastspeech2_amd/cwt.py) and the numpy restatement tests/cwt_ref.py, without a GPU:
the tables against the longdouble formula, the cut-off, the refusals, `row_scores` / `summarize` on hand-made sums, the known
answers on the restatement (each is verified here before tests/test_cwt_gpu.py holds a kernel to it), and `batch_bytes`."""
import json
import math
import os

import numpy as np
import pytest

from fastspeech2_amd import cwt as C
from fastspeech2_amd import metrics as M
from tests import cwt_ref as ref

EPS = 2.0 ** -52
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sr,hop", ref.RATES)
def test_tables_are_the_longdouble_formula_up_to_their_cut_off(sr, hop):
    """The bar: d / a, x x, 1 - x x, exp, the two powers and three products each round once, and the rounding of d / a is
    amplified by at most |x psi'(x)| < 4 psi(0): no entry is further than 16 fp64 epsilons of the scale's peak from the formula."""
    tab, support, a = C.tables(sr, hop)
    assert tab.shape == (10, 2048) and tab.dtype == np.float64 and support.dtype == np.int32
    for i in range(1, 11):
        want = ref.table(i, sr, hop, LD)
        n = int(support[i - 1])
        assert n == len(want) == ref.cutoff(i, sr, hop) + 1 == min(2048, int(10 * ref.scale_fraction(i, sr, hop)) + 1)
        assert float(np.abs(tab[i - 1, :n].astype(LD) - want).max()) <= 16 * EPS * float(want[0])
        assert not tab[i - 1, n:].any()
        assert a[i - 1] == float(ref.scale_fraction(i, sr, hop)) == ref.scales(sr, hop)[i - 1]
        assert tab[i - 1, 0] == pytest.approx(a[i - 1] ** -0.5 * (i + 2.5) ** -2.5 * 2 / (math.sqrt(3) * math.pi ** 0.25), rel=1e-14)
    assert C.scales_ms() == [20, 40, 80, 160, 320, 640, 1280, 2560, 5120, 10240]
    assert np.allclose(a * hop / sr * 1000, C.scales_ms(), rtol=1e-15)


def test_the_cut_off_is_exact_where_ten_scales_is_an_integer_and_neglects_less_than_1e_19_of_the_peak():
    assert [ref.cutoff(i, 16000, 200) for i in (1, 2, 7, 8)] == [16, 32, 1024, 2047]      # 10 a_1 = 16 frames exactly
    assert C.tables(16000, 200)[1].tolist() == [17, 33, 65, 129, 257, 513, 1025, 2048, 2048, 2048]
    assert C.tables(22050, 256)[1].tolist()[:3] == [18, 35, 69]
    for sr, hop in ref.RATES:
        a1 = ref.scales(sr, hop, LD)[0]
        assert abs(float(ref.psi((ref.cutoff(1, sr, hop) + 1) / a1, LD) / ref.psi(LD(0), LD))) < 1e-19


def test_a_first_scale_below_one_frame_and_a_missing_f0_are_refused_before_any_launch():
    for fn in (C.scales, C.tables):
        with pytest.raises(ValueError):
            fn(16000, 400)                                                  # a hop of 25 ms: a_1 = 0.8 frames
        with pytest.raises(ValueError):
            fn(22050.5, 256)
    assert C.scales(16000, 320)[0] == 1.0
    with pytest.raises(ValueError):
        ref.scales(16000, 400)
    wav = [np.zeros(4000, np.float32)]
    with pytest.raises(ValueError, match="wavelet"):
        M.score_pairs(wav, wav, None, 22050, 256, f0=False, wavelet=True)
    with pytest.raises(ValueError, match="wavelet"):
        M.run({"preprocessing": {"audio": {"sampling_rate": 22050}, "stft": {"hop_length": 256}}}, "/nowhere", "/nowhere/val.txt", f0=False,
              wavelet=True)
    with pytest.raises(ValueError):
        M.run({"preprocessing": {"audio": {"sampling_rate": 16000}, "stft": {"hop_length": 400}}}, "/nowhere", "/nowhere/val.txt", wavelet=True)


def test_batch_bytes_grows_by_88_bytes_per_frame_and_side():
    for n, T1, T2 in ((1, 1, 1), (32, 800, 900), (3, 2048, 17)):
        plain = M.batch_bytes(n, T1, T2, 13, 256, 0, True, True)
        assert M.batch_bytes(n, T1, T2, 13, 256, 0, True, True, wavelet=True) - plain == n * (T1 + T2) * 88
        assert M.batch_bytes(n, T1, T2, 13, 256, 0, True, True, wavelet=False) == plain
    assert M.WAVELET_FRAME_BYTES == 8 * (1 + C.SCALES)


# ------------------------------------------------------------------------------------------------ rows and summary
def _sums(sxx, syy, sxy, sd2):
    return np.tile(np.array([sxx, syy, sxy, sd2], np.float64), (15, 1))


def test_row_scores_on_hand_made_sums():
    stats_r, stats_s = [40, 5.0, 0.25, 0], [30, 4.5, 0.125, 0]
    s = _sums(4.0, 9.0, 3.0, 50.0)
    s[3] = [1e-24 * 100, 9.0, 3.0, 2.0]                                     # at the floor: no correlation, the RMSE stays
    s[12] = [4.0, 0.0, 0.0, 8.0]
    pr, ps = np.full(10, 200.0), np.full(10, 50.0)
    ps[9] = 0.0
    row = C.row_scores(s, 100, pr, 200, stats_r, ps, 50, stats_s)
    assert set(row) == set(C.row_keys()) == set(ref.KEYS)
    assert [len(row[k]) for k in C.row_keys()[:7]] == [10, 10, 5, 5, 10, 10, 10]
    assert row["cwt_corr"][0] == 0.5 and math.isnan(row["cwt_corr"][3]) and row["cwt_rmse"][3] == math.sqrt(2.0 / 100)
    assert row["cwt_rmse"][0] == math.sqrt(0.5) and row["cwt_level_corr"][0] == 0.5 and math.isnan(row["cwt_level_corr"][2])
    assert row["cwt_level_rmse"][2] == math.sqrt(8.0 / 100)
    assert row["cwt_power_db_ref"][0] == 0.0 and row["cwt_power_db_syn"][0] == 0.0 and row["cwt_power_ratio_db"][0] == 0.0
    assert row["cwt_power_db_syn"][9] == -math.inf and row["cwt_power_ratio_db"][9] == -math.inf
    assert (row["lf0_mean_ref"], row["lf0_mean_syn"], row["lf0_std_ref"], row["lf0_std_syn"]) == (5.0, 4.5, 0.25, 0.125)
    json.dumps(row)
    one = C.row_scores(_sums(4.0, 9.0, 3.0, 0.0), 1, pr, 200, stats_r, ps, 50, stats_s)        # a path of one cell has no correlation
    assert np.isnan(one["cwt_corr"]).all() and one["cwt_rmse"] == [0.0] * 10
    for flat_r, flat_s in ((1, 0), (0, 1), (1, 1)):                         # known answer 6: a flat side gives all NaN
        row = C.row_scores(s, 100, pr, 200, [0, 0.0, 0.0, flat_r], ps, 50, [30, 4.5, 0.125, flat_s])
        assert set(row) == set(C.row_keys()) and [len(row[k]) for k in C.row_keys()[:7]] == [10, 10, 5, 5, 10, 10, 10]
        assert all(np.isnan(np.asarray(v, np.float64)).all() for v in row.values())


def test_summarize_on_hand_made_rows_counts_a_flat_row_once():
    stats = [40, 5.0, 0.25, 0]
    p = np.full(10, 100.0)
    a = C.row_scores(_sums(4.0, 9.0, 3.0, 100.0), 100, p, 100, stats, 2 * p, 100, stats)
    b = C.row_scores(_sums(4.0, 4.0, 4.0, 0.0), 300, p, 100, stats, p / 2, 100, stats)
    b["cwt_corr"][1] = float("nan")
    flat = C.row_scores(_sums(1.0, 1.0, 1.0, 1.0), 50, p, 100, [0, 0.0, 0.0, 1], p, 100, stats)
    rows = [dict(r, path_len=P, mcd_db=1.0) for r, P in ((a, 100), (b, 300), (flat, 50))]
    out = C.summarize(rows)
    assert out["wavelet_flat_utterances"] == 1 and out["cwt_scales_ms"] == C.scales_ms()
    assert out["cwt_corr_mean"][0] == 0.75 and out["cwt_corr_weighted"][0] == (0.5 * 100 + 1.0 * 300) / 400
    assert out["cwt_corr_mean"][1] == 0.5 and out["cwt_corr_weighted"][1] == 0.5
    assert out["cwt_corr_nan_utterances"] == [1, 2] + [1] * 8 and out["cwt_level_rmse_nan_utterances"] == [1] * 5
    assert out["cwt_rmse_mean"][4] == 0.5 and out["cwt_rmse_weighted"][4] == 0.25 and len(out["cwt_level_corr_mean"]) == 5
    assert out["cwt_power_ratio_db_by_scale"] == pytest.approx([0.0] * 10, abs=1e-14) and len(out["cwt_power_ratio_db_by_scale"]) == 10
    json.dumps(out)
    only_flat = C.summarize(rows[2:])
    assert only_flat["wavelet_flat_utterances"] == 1 and np.isnan(only_flat["cwt_corr_mean"]).all() and np.isnan(only_flat["cwt_power_ratio_db_by_scale"]).all()
    merged = M.summarize(rows)
    assert merged["wavelet_flat_utterances"] == 1 and "cwt_corr_mean" not in M.summarize([{"path_len": 3, "mcd_db": 1.0}])


# ------------------------------------------------------------------------------------------------ the known answers, on the restatement
def test_known_answer_1_two_voiced_frames():
    f0 = np.zeros(9)
    f0[2], f0[6] = 100.0, 400.0
    want = [math.log(100.0)] * 3 + [math.log(100.0 * 4.0 ** (k / 4.0)) for k in (1, 2, 3)] + [math.log(400.0)] * 3
    for dtype in (np.float64, LD):
        c = ref.contour(f0, dtype)
        assert c["n_voiced"] == 2 and c["flat"] == 0
        assert float(np.abs(c["x"] - np.array(want)).max()) <= 2 * EPS * math.log(400.0)     # one rounding here, one in `want`
        assert abs(float(c["m"]) - float(np.mean(want))) <= 4 * EPS * 6 and abs(float(c["sd"]) - float(np.std(want))) <= 4 * EPS * 6
        assert abs(float(c["z"].sum())) <= 64 * EPS and abs(float((c["z"] ** 2).sum()) - 9) <= 64 * EPS


def test_known_answer_2_a_pair_against_itself():
    f0 = ref.case_input("mixed5")[4]
    pi, pj = ref.diagonal(len(f0))
    for sr, hop in ref.RATES:
        row = ref.row_scores(f0, f0.copy(), pi, pj, sr, hop)
        assert not np.any(row["cwt_rmse"]) and not np.any(row["cwt_level_rmse"]) and not np.any(row["cwt_power_ratio_db"])
        assert np.abs(row["cwt_corr"] - 1).max() <= 1e-15 and np.abs(row["cwt_level_corr"] - 1).max() <= 1e-15


def test_known_answer_3_halved_excursions_show_in_lf0_std_only():
    """The synthesized ln F0 is 0.5 x + c at the voiced frames up to the rounding of exp and ln (2 EPS of ln F0, about 1e-15), and
    the interpolation is linear, so z is the reference's up to that over sd: the correlations are 1 to second order in it."""
    f0 = ref.case_input("mixed5")[4]
    pi, pj = ref.diagonal(len(f0))
    row = ref.row_scores(f0, ref.halved(f0), pi, pj, *ref.RATES[0])
    assert abs(row["lf0_std_syn"] - 0.5 * row["lf0_std_ref"]) <= 8 * EPS * 6
    assert np.abs(row["cwt_corr"] - 1).max() <= 8 * EPS and np.abs(row["cwt_level_corr"] - 1).max() <= 8 * EPS
    assert row["lf0_std_ref"] > 0.1


@pytest.mark.parametrize("sr,hop", ref.RATES)
def test_known_answer_4_a_cosine_peaks_at_its_scale(sr, hop):
    t = np.arange(2048, dtype=np.float64)
    a = ref.scales(sr, hop)
    weight = np.array([ref.scale_weight(i) for i in range(1, 11)])
    assert np.array_equal(weight, C.scale_weights())
    for i in (3, 4, 5):
        z = np.cos(2 * np.pi * t / (2 * np.pi * a[i - 1] / math.sqrt(2.5)))
        _, power = ref.transform(z, sr, hop)
        assert int(np.argmax(power / weight ** 2)) + 1 == i


def test_known_answer_5_a_moving_average_takes_the_small_scales_away():
    f0 = ref.wiggly()
    pi, pj = ref.diagonal(len(f0))
    row = ref.row_scores(f0, ref.moving_average(f0), pi, pj, *ref.RATES[0])
    assert row["cwt_power_ratio_db"][0] < row["cwt_power_ratio_db"][4] and row["cwt_power_ratio_db"][0] < 0
    assert row["lf0_std_syn"] < row["lf0_std_ref"]


def test_known_answer_6_a_flat_side_is_all_nan_on_the_restatement():
    f0 = ref.case_input("mixed5")[4]
    pi, pj = ref.diagonal(len(f0))
    for flat in (np.zeros(len(f0)), np.full(len(f0), 150.0)):
        assert ref.contour(flat)["flat"] == 1 and not ref.contour(flat)["z"].any()
        row = ref.row_scores(f0, flat, pi, pj, *ref.RATES[0])
        assert set(row) == set(ref.KEYS) and all(np.isnan(np.asarray(v, np.float64)).all() for v in row.values())


def test_the_fft_and_the_direct_sum_restatements_agree_and_the_bars_file_is_current():
    bars = json.load(open(os.path.join(ROOT, "tests", "golden", "cwt_bars.json")))
    assert bars["factor"] == 16 and set(bars["distance"]) == set(ref.CASES) | set(ref.PATH_CASES)
    assert bars["cases"] == {k: {"seed": v[0], "rows": [list(r) for r in v[1]]} for k, v in ref.CASES.items()}
    z = ref.contour(ref.case_input("mixed5")[0])["z"]
    (W, p), (Wl, pl) = ref.transform(z, *ref.RATES[0]), ref.transform(z, *ref.RATES[0], LD)
    assert float(np.abs(W - Wl).max()) <= bars["distance"]["mixed5"]["W_22050_256"]
    zero = {k for k, v in bars["distance"]["degenerate"].items() if v == 0}
    assert zero == {"z", "W_22050_256", "W_16000_200", "power_22050_256", "power_16000_200"}     # 0 by definition: flat rows
    assert all(v > 0 for name in ("lengths", "mixed5") for v in bars["distance"][name].values())
