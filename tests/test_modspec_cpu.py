"""Over-smoothing scores without a GPU: the known answers of the specification (fastspeech2_amd/modspec.py) through the numpy
restatement tests/modspec_ref.py, the host code (band tables, twiddles, row scores, the summary merge, `metrics.run` through its
`score_fn` seam) and the refusals that need no device.  The bars are those of tests/golden/modspec_bars.json: 16 times the distance
between the fp64 and the longdouble restatement on the same input (tests/golden/make_modspec_bars.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import metrics as M
from fastspeech2_amd import modspec as MS
from tests import modspec_ref as ref
from tests.test_stoi_cpu import _fake, corpus  # noqa: F401  (the three-utterance tmp_path corpus)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "modspec_bars.json")))
LN_FLOOR = math.log(MS.FLOOR)


def bar(case, key):
    return BARS["factor"] * BARS["distance"][case][key]


def test_the_bars_belong_to_these_inputs():
    assert BARS["factor"] == 16 and BARS["cosine"] == [ref.COSINE_A, ref.COSINE_T, ref.COSINE_CYCLES]
    assert BARS["constant"] == [ref.CONSTANT, ref.CONSTANT_T]
    assert BARS["cases"] == {k: {"seed": v[0], "K": v[1], "frames": list(v[2])} for k, v in ref.CASES.items()}
    assert set(ref.EVERY_T) == set(ref.CASES["k13"][2]) == set(ref.CASES["k1"][2])
    assert (ref.N, ref.FLOOR, ref.MIN_FRAMES) == (MS.NFFT, MS.FLOOR, MS.MIN_FRAMES) and tuple(float(e) for e in ref.EDGES_HZ) == MS.EDGES_HZ


# ------------------------------------------------------------------------------------------------ known answers
def test_a_cosine_puts_its_power_into_one_bin():
    A, T = ref.COSINE_A, ref.COSINE_T
    c = ref.chain(ref.case_input("cosine")[0])
    ms = c["logms"][0]
    assert abs(ms[256] - math.log(A * A * T / 4 + MS.FLOOR)) <= bar("cosine", "logms")
    others = np.array([f for f in range(0, ref.HALF + 1, 4) if f != 256])
    assert np.abs(ms[others] - LN_FLOOR).max() <= bar("cosine", "logms")
    assert abs(c["gv"][0] - A * A / 2) <= bar("cosine", "gv") and abs(c["mean"][0]) <= 1e-16


def test_a_constant_has_no_variance_and_no_modulation():
    c = ref.chain(ref.case_input("constant")[0], [ref.band_bins(22050, 256)[0]])
    assert c["gv"][0] == 0 and c["mean"][0] == ref.CONSTANT
    assert np.abs(c["logms"] - LN_FLOOR).max() <= bar("constant", "logms")
    assert np.abs(c["bands"][0] - LN_FLOOR * MS.DB).max() <= bar("constant", "bands_22050_256")


def test_smoothing_lowers_the_variance_and_every_band_from_4_hz_up():
    """a seeded noise trajectory against itself filtered with (1/4, 1/2, 1/4): seed 11, 1024 frames, on the restatement alone"""
    assert (ref.SMOOTH_SEED, ref.SMOOTH_T) == (11, 1024)
    x = np.random.default_rng(ref.SMOOTH_SEED).standard_normal((ref.SMOOTH_T, 1))
    for sr, hop in ref.RATES:
        bins, hz = ref.band_bins(sr, hop)
        a, b = ref.chain(x, [bins]), ref.chain(ref.smoothed(x), [bins])
        assert b["gv"][0] < a["gv"][0]
        high = [j for j, (lo, _) in enumerate(hz) if lo >= 4]
        assert len(high) == 4
        print(sr, hop, (b["bands"][0][0] - a["bands"][0][0]).tolist())
        for j in high:
            assert b["bands"][0][0, j] < a["bands"][0][0, j], (sr, hop, j)
        drop = a["bands"][0][0, high] - b["bands"][0][0, high]
        assert np.all(np.diff(drop) > 0) and drop[-1] > 10                  # the higher the band, the more is missing
        r = ref.row_scores(x, ref.smoothed(x), bins)
        assert r["gv_ratio_db"] < 0 and r["ms_dist_db"] > 1 and np.all(np.diff(r["ms_band_db_syn"] - r["ms_band_db_ref"])[3:] < 0)


def test_the_longdouble_restatement_agrees_with_the_fft():
    c = ref.case_input("one_row")[0][:40, :2]
    tables = [ref.band_bins(*r)[0] for r in ref.RATES]
    a, b = ref.chain(c, tables), ref.chain(c, tables, np.longdouble)
    assert b["logms"].dtype == np.longdouble and np.abs(a["logms"] - b["logms"]).max() < 1e-10
    assert np.abs(a["m2"] - b["m2"]).max() < 1e-12 and np.abs(a["bands"][1] - b["bands"][1]).max() < 1e-10


# ------------------------------------------------------------------------------------------------ host code
@pytest.mark.parametrize("sr,hop", ref.RATES)
def test_band_bins(sr, hop):
    bins, hz = MS.band_bins(sr, hop)
    assert (bins, hz) == ref.band_bins(sr, hop)
    assert len(bins) == len(hz) == 8 and bins[0][0] == 1 and bins[-1][1] == MS.NFFT // 2 + 1
    for (lo, hi), (nlo, _) in zip(bins, bins[1:] + [(MS.NFFT // 2 + 1, None)]):
        assert lo < hi == nlo                                               # non-empty, ascending, disjoint, no gap
    assert [h[0] for h in hz] == list(MS.EDGES_HZ) and hz[-1][1] == sr / (2 * hop) and [h[1] for h in hz[:-1]] == list(MS.EDGES_HZ[1:])
    rate = sr / hop
    for (lo, hi), (flo, fhi) in zip(bins, hz):
        assert lo * rate / MS.NFFT >= flo > (lo - 1) * rate / MS.NFFT or lo == 1
        assert (hi - 1) * rate / MS.NFFT < fhi or hi == MS.NFFT // 2 + 1


def test_band_bins_drops_what_the_frame_rate_cannot_hold():
    bins, hz = MS.band_bins(8000, 400)                                      # 20 frames a second: Nyquist 10 Hz
    assert [h[0] for h in hz] == [0.0, 0.5, 1.0, 2.0, 4.0, 8.0] and hz[-1] == (8.0, 10.0) and bins[-1][1] == 2049
    assert (bins, hz) == ref.band_bins(8000, 400)
    bins, hz = MS.band_bins(16000, 250)                                     # Nyquist exactly 32 Hz: no band above it
    assert hz[-1] == (16.0, 32.0) and len(hz) == 7 and bins[-1][1] == 2049 and (bins, hz) == ref.band_bins(16000, 250)
    for bad in ((22050.5, 256), (0, 256), (22050, 0)):
        with pytest.raises(ValueError):
            MS.band_bins(*bad)


def test_twiddles():
    tw = MS.twiddles()
    assert tw.shape == (4096, 2) and tw.dtype == np.float64 and tw.flags["C_CONTIGUOUS"]
    assert np.abs(tw[:, 0] ** 2 + tw[:, 1] ** 2 - 1).max() < 1e-15 and tw[0].tolist() == [1, 0] and tw[1024].tolist() == pytest.approx([0, 1])
    j = np.arange(4096)
    assert np.abs(tw[:, 0] - np.cos(2 * np.pi * j / 4096)).max() == 0


def _row(gr, gs, br, bs, Tr=100, Ts=100):
    K = len(gr)
    return MS.row_scores(np.array(gr) * Tr, np.array(br, float).reshape(K, -1), Tr, np.array(gs) * Ts, np.array(bs, float).reshape(K, -1), Ts)


def test_row_scores_by_hand():
    r = _row([1.0, 4.0, 0.0], [0.1, 4.0, 2.0], [[0, 0], [0, 0], [0, 0]], [[3, 4], [0, 0], [0, 0]])
    assert r["gv_ref"] == [1.0, 4.0, 0.0] and r["gv_syn"] == pytest.approx([0.1, 4.0, 2.0])
    assert r["gv_ratio_db"] == pytest.approx(-5.0)                           # (-10 + 0) / 2: the k with a zero variance is left out
    assert r["ms_band_db_syn"] == pytest.approx([1.0, 4 / 3]) and r["ms_band_db_ref"] == [0, 0]
    assert r["ms_dist_db"] == pytest.approx(math.sqrt(25 / 6)) and r["ms_db_syn"] == [[3, 4], [0, 0], [0, 0]]
    r = _row([0.0], [1.0], [[1, 2]], [[1, 2]])
    assert math.isnan(r["gv_ratio_db"]) and r["ms_dist_db"] == 0
    # fewer than 32 frames on either side: no MS on both sides, GV stays; one frame: no GV either
    r = _row([1.0], [2.0], [[1, 2]], [[1, 2]], Tr=31, Ts=500)
    assert math.isnan(r["ms_dist_db"]) and np.isnan(r["ms_db_ref"]).all() and np.isnan(r["ms_band_db_syn"]).all()
    assert r["gv_ratio_db"] == pytest.approx(10 * math.log10(2))
    r = _row([0.0], [2.0], [[1, 2]], [[1, 2]], Tr=1, Ts=500)
    assert np.isnan(r["gv_ref"]).all() and r["gv_syn"] == pytest.approx([2.0]) and math.isnan(r["gv_ratio_db"])
    r = _row([1.0], [2.0], [[1, 2]], [[1, 2]], Tr=32, Ts=32)
    assert r["ms_dist_db"] == 0


def test_the_summary_merge_on_hand_made_rows():
    rows = [dict(_row([1.0, 2.0], [0.5, 2.0], [[0, 0], [0, 0]], [[1, -1], [1, -3]]), frames_ref=100, frames_syn=100),
            dict(_row([3.0, 2.0], [1.5, 6.0], [[2, 2], [2, 2]], [[1, 1], [1, 1]]), frames_ref=100, frames_syn=100),
            dict(_row([9.0, 9.0], [9.0, 9.0], [[9, 9], [9, 9]], [[0, 0], [0, 0]], Tr=20), frames_ref=20, frames_syn=100),
            dict(_row([0.0, 0.0], [1.0, 1.0], [[9, 9], [9, 9]], [[0, 0], [0, 0]], Tr=1, Ts=1), frames_ref=1, frames_syn=1)]
    s = MS.summarize(rows)
    # corpus means over rows 0 and 1: ref [[1, 1], [1, 1]], syn [[1, 0], [1, -1]] -> diff [[0, -1], [0, -2]]
    assert s["ms_diff_db_by_band"] == pytest.approx([0.0, -1.5]) and s["ms_dist_db_corpus"] == pytest.approx(math.sqrt(5 / 4))
    # GV means over rows 0..2 (row 3 has one frame): ref [13/3, 13/3], syn [11/3, 17/3]
    assert s["gv_ratio_db_by_coef"] == pytest.approx([10 * math.log10(11 / 13), 10 * math.log10(17 / 13)])
    assert s["smoothing_too_short_utterances"] == 2 and s["ms_dist_db_nan_utterances"] == 2 and s["gv_ratio_db_nan_utterances"] == 1
    assert s["ms_dist_db_mean"] == pytest.approx((rows[0]["ms_dist_db"] + rows[1]["ms_dist_db"]) / 2)
    assert s["gv_ratio_db_mean"] == pytest.approx(np.mean([r["gv_ratio_db"] for r in rows[:3]]))
    s = MS.summarize(rows[2:])
    assert s["ms_diff_db_by_band"] is None and math.isnan(s["ms_dist_db_corpus"]) and math.isnan(s["ms_dist_db_mean"])
    assert MS.summarize(rows[3:])["gv_ratio_db_by_coef"] is None
    json.dumps(MS.summarize(rows))


def test_batch_bytes_counts_the_new_buffers():
    base = M.batch_bytes(3, 100, 120, 13, 256, 0, False)
    assert M.batch_bytes(3, 100, 120, 13, 256, 0, False, smoothing=True) == base + 3 * 2 * 13 * (2 + 8) * 8
    assert M.batch_bytes(3, 100, 120, 13, 256, 0, False, False) == base and M.SMOOTHING_BANDS == len(MS.EDGES_HZ)


def test_bad_arguments_are_value_errors_without_a_device():
    c = torch.zeros(2, 40, 13, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        MS.moments(c, [40, 40])
    with pytest.raises(ValueError, match="no CPU fallback"):
        MS.modspec(c, [40, 40], torch.zeros(2, 13, dtype=torch.float64), [(1, 5)])
    for lens in ([0, 40], [40, 2049]):
        with pytest.raises(ValueError, match="frames"):
            MS.moments(c, lens)
    for bins in ([], [(5, 5)], [(1, 9), (8, 12)], [(1, 2050)], [(-1, 4)], [(1, 2)] * 17):
        with pytest.raises(ValueError, match="band"):
            MS.modspec(c, [40, 40], torch.zeros(2, 13, dtype=torch.float64), bins)


# ------------------------------------------------------------------------------------------------ metrics.run / score.py
def _smooth_fake(seen):
    def fn(refs, syns, **kw):
        seen.append(kw)
        rows = _fake(refs, syns)
        for k, r in enumerate(rows):
            r.update(_row([1.0, 2.0], [0.5, 1.0 + k], [[0, 0], [0, 0]], [[-1, -2], [-3, -4]], Tr=r["frames_ref"], Ts=r["frames_syn"]))
        return rows
    return fn


def test_run_without_smoothing_is_what_it_was_and_with_it_adds_the_keys(corpus, capsys):  # noqa: F811
    import score
    from tests.test_align_cpu import config
    base = M.run(config(corpus), os.path.join(corpus, "result"), os.path.join(corpus, "val.txt"), score_fn=_fake)
    off = M.run(config(corpus), os.path.join(corpus, "result"), os.path.join(corpus, "val.txt"), score_fn=_fake, smoothing=False)
    assert off == base and "ms_bands_hz" not in base[2] and set(base[2]) == {"utterances", "mcd_db_mean", "mcd_db_weighted", "skipped",
                                                                              "reference_window"}
    seen = []
    out = os.path.join(corpus, "scores.jsonl")
    argv = ["-p", os.path.join(corpus, "preprocess.yaml"), "-t", os.path.join(corpus, "train.yaml"), "--source",
            os.path.join(corpus, "val.txt"), "--out", out]
    assert score.parse_args(argv).smoothing is False
    rows, skipped, summary = score.main(argv + ["--smoothing"], score_fn=_smooth_fake(seen))
    assert seen == [{"smoothing": True}] and not skipped and len(rows) == 3
    new = {"gv_ref", "gv_syn", "gv_ratio_db", "ms_db_ref", "ms_db_syn", "ms_band_db_ref", "ms_band_db_syn", "ms_dist_db"}
    for r, b in zip(rows, base[0]):
        assert new <= set(r) and {k: v for k, v in r.items() if k not in new} == b
    assert summary["ms_bands_hz"] == [list(h) for h in MS.band_bins(22050, 256)[1]] and len(summary["ms_bands_hz"]) == 8
    assert summary["ms_diff_db_by_band"] == pytest.approx([-2.0, -3.0]) and summary["ms_dist_db_corpus"] == pytest.approx(math.sqrt(7.5))
    assert summary["gv_ratio_db_by_coef"] == pytest.approx([10 * math.log10(0.5), 0.0])
    assert summary["smoothing_too_short_utterances"] == 0 and summary["gv_ratio_db_nan_utterances"] == 0
    assert {k: summary[k] for k in base[2]} == base[2]
    assert [json.loads(line) for line in open(out)] == rows
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["ms_dist_db_mean"] == pytest.approx(summary["ms_dist_db_mean"])
    seen.clear()
    score.main(argv + ["--smoothing", "--prosody"], score_fn=lambda r, s, **kw: seen.append(kw) or _smooth_fake([])(r, s))
    assert seen == [{"prosody": True, "smoothing": True}]
