"""GPU over-smoothing scores (fastspeech2_amd/modspec.py, csrc/fs2_modspec.hip) against the fp64 restatement tests/modspec_ref.py:
the moments kernel, then the modulation-spectrum kernel on the restatement's own means, bin by bin and per band at two band
tables, then `measure`, `metrics.score_pairs` and score.py --smoothing end to end.  Floating outputs are held to the bars of
tests/golden/modspec_bars.json: per case and output 16 times the distance between the fp64 and the longdouble restatement on that
case's input (tests/golden/make_modspec_bars.py), never anything a kernel gave.  Every batch's padding is NaN."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml
from scipy.io import wavfile

from fastspeech2_amd import metrics as M
from fastspeech2_amd import modspec as MS
from tests import f0_signals as S
from tests import modspec_ref as ref
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "modspec_bars.json")))
TABLES = [ref.band_bins(sr, hop)[0] for sr, hop in ref.RATES]
BAND_KEYS = [f"bands_{sr}_{hop}" for sr, hop in ref.RATES]
SLACK = -7.0


def bar(case, key):
    return BARS["factor"] * BARS["distance"][case][key]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the rows of a case and the restatement's chain of each, computed once"""
    rows = ref.case_input(name)
    return rows, [ref.chain(c, TABLES) for c in rows]


def _batch(rows, dev, strided=False):
    """(B, Tmax, K) with NaN beyond every row's frames; `strided`: a view into a larger NaN buffer, unit stride in k only"""
    lens, K = [len(r) for r in rows], rows[0].shape[1]
    pad = (3, 5) if strided else (0, 0)
    x = np.full((len(rows), max(lens) + pad[0], K + pad[1]), np.nan)
    for b, r in enumerate(rows):
        x[b, :lens[b], :K] = r
    c = torch.from_numpy(x).to(dev)[:, :max(lens), :K]
    assert c.is_contiguous() != strided or len(rows) * K == 1
    return c, lens


def _worst(got, want):
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max())


@pytest.mark.parametrize("name", list(ref.CASES))
def test_moments_logms_and_bands_against_the_restatement(dev, name):
    """k40 runs on non-contiguous batch and frame strides and writes into buffers larger than needed, whose slack must stay"""
    rows, chains = _case(name)
    odd = name == "k40"
    c, lens = _batch(rows, dev, strided=odd)
    B, K = len(rows), rows[0].shape[1]
    slack = lambda *shape: torch.full(shape, SLACK, dtype=torch.float64, device=dev) if odd else None     # noqa: E731
    out = slack(B, K + 2, 3)
    mom = MS.moments(c, lens, out=out)
    assert mom.dtype == torch.float64 and mom.shape == ((B, K + 2, 3) if odd else (B, K, 2))
    momh = mom.cpu().numpy()
    want_mean, want_m2 = np.stack([ch["mean"] for ch in chains]), np.stack([ch["m2"] for ch in chains])
    w_mean, w_m2 = _worst(momh[:, :K, 0], want_mean), _worst(momh[:, :K, 1], want_m2)
    print(f"{name}: mean {w_mean:.2e} (bar {bar(name, 'mean'):.2e}), M2 {w_m2:.2e} (bar {bar(name, 'm2'):.2e})")
    assert w_mean <= bar(name, "mean") and w_m2 <= bar(name, "m2")
    for b, T in enumerate(lens):
        assert _worst(momh[b, :K, 1] / T, chains[b]["gv"]) <= bar(name, "gv")
        if T == 1:
            assert np.array_equal(momh[b, :K, 0], rows[b][0]) and not momh[b, :K, 1].any()
    if odd:
        assert np.all(momh[:, K:] == SLACK) and np.all(momh[:, :, 2] == SLACK)
    mean = torch.from_numpy(want_mean).to(dev)                             # the restatement's means: this kernel alone is under test
    for table, key in zip(TABLES, BAND_KEYS):
        J = len(table)
        ob, ol = slack(B, K + 3, J + 2), slack(B, K + 1, MS.NFFT // 2 + 8)
        bands, logms = MS.modspec(c, lens, mean, table, logms=True, out=ob, out_logms=ol)
        bh, lh = bands.cpu().numpy(), logms.cpu().numpy()
        w_l = _worst(lh[:, :K, :2049], np.stack([ch["logms"] for ch in chains]))
        w_b = _worst(bh[:, :K, :J], np.stack([ch["bands"][TABLES.index(table)] for ch in chains]))
        print(f"{name} {key}: logms {w_l:.2e} (bar {bar(name, 'logms'):.2e}), bands {w_b:.2e} (bar {bar(name, key):.2e})")
        assert w_l <= bar(name, "logms") and w_b <= bar(name, key)
        if odd:
            assert np.all(bh[:, K:] == SLACK) and np.all(bh[:, :, J:] == SLACK) and np.all(lh[:, K:] == SLACK) and np.all(lh[:, :, 2049:] == SLACK)
        else:
            assert bands.shape == (B, K, J) and logms.shape == (B, K, 2049)
            only = MS.modspec(c, lens, mean, table)                         # without the full-resolution output: the same bands
            assert only.cpu().numpy().tobytes() == bh.tobytes()
    # both kernels chained, the second on the first's means
    m2, bands = MS.measure(c, lens, TABLES[0])
    assert m2.cpu().numpy().tobytes() == np.ascontiguousarray(momh[:, :K, 1]).tobytes()
    assert _worst(bands.cpu().numpy(), np.stack([ch["bands"][0] for ch in chains])) <= bar(name, BAND_KEYS[0])


def test_two_launches_give_the_same_bytes_and_a_row_does_not_depend_on_its_batch(dev):
    rows, _ = _case("k13")
    c, lens = _batch(rows, dev)
    first, second = MS.moments(c, lens), MS.moments(c, lens)
    assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()
    a, b = MS.modspec(c, lens, first[:, :, 0], TABLES[0], logms=True), MS.modspec(c, lens, second[:, :, 0], TABLES[0], logms=True)
    for u, v in zip(a, b):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    c1, l1 = _batch(rows[3:4], dev)                                          # B = 1: the same bytes as the row in the batch
    m1 = MS.moments(c1, l1)
    assert m1.cpu().numpy().tobytes() == first[3:4].cpu().numpy().tobytes()
    one = MS.modspec(c1, l1, m1[:, :, 0], TABLES[0], logms=True)
    assert one[0].cpu().numpy().tobytes() == a[0][3:4].cpu().numpy().tobytes() and one[1].cpu().numpy().tobytes() == a[1][3:4].cpu().numpy().tobytes()


def test_the_cosine_and_the_constant_on_the_device(dev):
    A, T = ref.COSINE_A, ref.COSINE_T
    c, lens = _batch(ref.case_input("cosine"), dev)
    mom = MS.moments(c, lens)
    bands, logms = MS.modspec(c, lens, mom[:, :, 0], TABLES[0], logms=True)
    ms, momh = logms.cpu().numpy()[0, 0], mom.cpu().numpy()[0, 0]
    assert abs(ms[256] - math.log(A * A * T / 4 + MS.FLOOR)) <= bar("cosine", "logms")
    others = np.array([f for f in range(0, 2049, 4) if f != 256])
    assert np.abs(ms[others] - math.log(MS.FLOOR)).max() <= bar("cosine", "logms")
    assert abs(momh[1] / T - A * A / 2) <= bar("cosine", "gv") and abs(momh[0]) <= 1e-16
    assert _worst(ms, _case("cosine")[1][0]["logms"][0]) <= bar("cosine", "logms")
    c, lens = _batch(ref.case_input("constant"), dev)
    mom = MS.moments(c, lens)
    bands, logms = MS.modspec(c, lens, mom[:, :, 0], TABLES[0], logms=True)
    assert mom.cpu().numpy()[0, 0].tolist() == [ref.CONSTANT, 0.0]
    assert np.abs(logms.cpu().numpy() - math.log(MS.FLOOR)).max() <= bar("constant", "logms")
    assert np.abs(bands.cpu().numpy() - math.log(MS.FLOOR) * MS.DB).max() <= bar("constant", BAND_KEYS[0])


def test_bad_arguments_are_refused_before_launch(dev):
    from fastspeech2_amd import _lib, ops
    c = torch.zeros(2, 40, 13, dtype=torch.float64, device=dev)
    mean = torch.zeros(2, 13, dtype=torch.float64, device=dev)
    bins = TABLES[0]
    for bad_c, lens in ((c, [0, 40]), (c, [40, 41]), (c, [40]), (c.float(), [40, 40]), (c[:, :, ::2], [40, 40]), (c[0], [40]),
                        (torch.zeros(1, 2049, 1, dtype=torch.float64, device=dev), [2049]),
                        (torch.zeros(1, 4, 129, dtype=torch.float64, device=dev), [4]), (c[:1].expand(2, 40, 13), [40, 40])):
        with pytest.raises(ValueError):
            MS.moments(bad_c, lens)
        with pytest.raises(ValueError):
            MS.modspec(bad_c, lens, mean, bins)
    for bad_mean in (mean.cpu(), mean.float(), mean[:, :12], mean[:1].expand(2, 13)):
        with pytest.raises(ValueError):
            MS.modspec(c, [40, 40], bad_mean, bins)
    with pytest.raises(ValueError):
        MS.moments(c, [40, 40], out=torch.zeros(2, 13, 1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        MS.modspec(c, [40, 40], mean, bins, out=torch.zeros(2, 13, len(bins) - 1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        MS.modspec(c, [40, 40], mean, bins, out_logms=torch.zeros(2, 13, 2048, dtype=torch.float64, device=dev))
    # the C entry points themselves
    lens = torch.tensor([40, 40], dtype=torch.int32, device=dev)
    tw = MS._twiddles_on(dev)
    out = torch.zeros(2, 13, 8, dtype=torch.float64, device=dev)
    table = np.ascontiguousarray(np.array(bins, np.int32))
    swapped = table.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    call = lambda t, n, floor, ldo_k, T, K: _lib.call(                     # noqa: E731
        "fs2_modspec", c.data_ptr(), c.stride(0), c.stride(1), lens.data_ptr(), mean.data_ptr(), 13, 1, tw.data_ptr(), t.ctypes.data, n, floor,
        out.data_ptr(), 13 * ldo_k, ldo_k, None, 0, 0, 2, T, K, ops._stream())
    for args in ((swapped, 8, 1e-12, 8, 40, 13), (table, 17, 1e-12, 17, 40, 13), (table, 8, 0.0, 8, 40, 13), (table, 8, 1e-12, 7, 40, 13),
                 (table, 8, 1e-12, 8, 2049, 13), (table, 8, 1e-12, 8, 40, 129), (table, 8, 1e-12, 8, 0, 13)):
        with pytest.raises(ValueError):
            call(*args)
    with pytest.raises(ValueError):
        _lib.call("fs2_traj_moments", c.data_ptr(), c.stride(0), c.stride(1), lens.data_ptr(), out.data_ptr(), 13, 1, 2, 40, 13, ops._stream())
    assert _lib.load().fs2_modspec_nfft() == MS.NFFT == 2 * M.max_frames() and not out.any()


# ------------------------------------------------------------------------------------------------ end to end
def _tones(f0s, durs):
    return np.concatenate([S.tone(f, d) for f, d in zip(f0s, durs)])


def _pairs():
    """four short (recorded, synthesized) pairs: a copy, another rhythm, another melody, and a side of 20 frames"""
    base = _tones((200.0, 260.0, 150.0), (0.25, 0.2, 0.3))
    return [(base, base.copy()), (base, _tones((200.0, 260.0, 150.0), (0.3, 0.15, 0.4))), (base, _tones((110.0, 330.0), (0.4, 0.3))),
            (base, S.tone(180.0, (19 * S.HOP + 10) / S.FS))]


def _stft(cfg):
    from fastspeech2_amd import audio as Audio
    pp = cfg["preprocessing"]
    return Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"], pp["mel"]["n_mel_channels"],
                              pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])


def _cepstra(stft, wavs, frames, dev):
    """what score_pairs' own front end gives for these waveforms: `metrics.cepstra` of the clamped audio's mel, row by row"""
    out = []
    for w, T in zip(wavs, frames):
        y = torch.from_numpy(w[None]).to(dev)
        mel, _, _ = stft.mel_spectrogram_ragged(y.clamp(-1.0, 1.0), [len(w)])
        out.append(M.cepstra(mel, [T], 13).cpu().numpy()[0, :T])
    return out


def test_score_pairs_keeps_every_old_key_and_adds_the_restatements_scores(dev):
    pairs = _pairs()
    stft = _stft(config("/nowhere"))
    refs, syns = [p[0] for p in pairs], [p[1] for p in pairs]
    plain = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev)
    rows = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, smoothing=True)
    again = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, smoothing=True, budget=1)       # one pair per batch
    assert json.dumps(rows) == json.dumps(again)
    new = {"gv_ref", "gv_syn", "gv_ratio_db", "ms_db_ref", "ms_db_syn", "ms_band_db_ref", "ms_band_db_syn", "ms_dist_db"}
    for r, p in zip(rows, plain):
        assert set(r) == set(p) | new and json.dumps({k: v for k, v in r.items() if k not in new}) == json.dumps(p)
    assert [r["frames_syn"] for r in rows][3] == 20 and all(r["frames_ref"] >= 32 for r in rows)
    bins = MS.band_bins(S.FS, S.HOP)[0]
    ca = _cepstra(stft, refs, [r["frames_ref"] for r in rows], dev)
    cb = _cepstra(stft, syns, [r["frames_syn"] for r in rows], dev)
    want = [ref.row_scores(a, b, bins) for a, b in zip(ca, cb)]
    exact = [ref.row_scores(a, b, bins, np.longdouble) for a, b in zip(ca, cb)]
    for key in sorted(new):
        dist = [np.abs(np.asarray(w[key], np.longdouble) - e[key]) for w, e in zip(want[:3], exact[:3])]
        limit = 16 * float(max(d.max() for d in dist))                      # the bar of this input: the restatement's own rounding
        worst = max(float(np.abs(np.asarray(r[key]) - w[key]).max()) for r, w in zip(rows[:3], want[:3]))
        print(f"{key}: largest distance {worst:.2e}, bar {limit:.2e}")
        assert worst <= limit, key
    assert rows[0]["ms_dist_db"] == 0 and rows[0]["gv_ratio_db"] == 0 and rows[1]["ms_dist_db"] > 0
    short = rows[3]                                                         # 20 frames on one side: no MS on either, GV stays
    assert math.isnan(short["ms_dist_db"]) and np.isnan(short["ms_db_ref"]).all() and np.isnan(short["ms_band_db_syn"]).all()
    assert np.isfinite(short["gv_syn"]).all() and np.isfinite(short["gv_ratio_db"])
    for key in ("gv_ref", "gv_syn"):
        assert float(np.abs(np.asarray(short[key]) - want[3][key]).max()) <= 16 * float(np.abs(want[3][key] - exact[3][key]).max())
    summary = M.summarize(rows)
    assert summary["smoothing_too_short_utterances"] == 1 and summary["ms_dist_db_nan_utterances"] == 1 and len(summary["ms_diff_db_by_band"]) == 8
    assert "ms_dist_db_mean" not in M.summarize(plain)


def test_score_smoothing_end_to_end(dev, tmp_path, capsys):
    import score
    root = str(tmp_path)
    for k, (x, y) in enumerate(_pairs()[1:]):
        for folder, w in ((os.path.join("raw", "spk"), x), ("result", y)):
            os.makedirs(os.path.join(root, folder), exist_ok=True)
            wavfile.write(os.path.join(root, folder, f"u{k}.wav"), S.FS, np.round(w * 32767).astype(np.int16))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"u{k}|spk|{{AA B}}|text {k}\n" for k in range(3)))
    for name, doc in (("preprocess.yaml", config(root)), ("train.yaml", {"path": {"result_path": os.path.join(root, "result")}})):
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    argv = ["-p", os.path.join(root, "preprocess.yaml"), "-t", os.path.join(root, "train.yaml"), "--source", os.path.join(root, "val.txt"),
            "--no_f0", "--out", os.path.join(root, "s.jsonl")]
    plain, _, summary0 = score.main(argv)
    capsys.readouterr()
    rows, skipped, summary = score.main(argv + ["--smoothing"])
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    new = {"ms_bands_hz", "ms_diff_db_by_band", "ms_dist_db_corpus", "gv_ratio_db_by_coef", "gv_ratio_db_mean", "gv_ratio_db_nan_utterances",
           "ms_dist_db_mean", "ms_dist_db_nan_utterances", "smoothing_too_short_utterances"}
    assert not skipped and set(summary) == set(summary0) | new and not new & set(summary0) and set(said) == set(summary)
    assert {k: summary[k] for k in summary0} == summary0 and "gv_ref" not in plain[0]
    assert summary["smoothing_too_short_utterances"] == 1 and rows[2]["frames_syn"] == 20 and math.isnan(rows[2]["ms_dist_db"])
    assert summary["ms_bands_hz"] == [list(h) for h in MS.band_bins(S.FS, S.HOP)[1]] and len(summary["gv_ratio_db_by_coef"]) == 13
    assert len(summary["ms_diff_db_by_band"]) == 8 and np.isfinite(summary["ms_diff_db_by_band"]).all() and summary["ms_dist_db_corpus"] > 0
    assert summary["ms_dist_db_mean"] == pytest.approx(np.mean([r["ms_dist_db"] for r in rows[:2]]), abs=1e-12)
    assert [json.loads(line)["basename"] for line in open(os.path.join(root, "s.jsonl"))] == ["u0", "u1", "u2"]
