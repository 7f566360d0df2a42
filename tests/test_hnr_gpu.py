"""GPU harmonics-to-noise ratio (fastspeech2_amd/hnr.py, csrc/fs2_hnr.hip) against the fp64 restatement tests/hnr_ref.py: each kernel
alone, fed the restatement's own upstream values (the frame kernel the audio and the track, the side and path kernels the
restatement's frames), then the known answers of the specification, `metrics.score_pairs(hnr=True)` and score.py --hnr end to end.
Floating outputs are held to the bars of tests/golden/hnr_bars.json: per case and output 16 times the distance between the fp64 and
the longdouble restatement of that stage on that case's input (tests/golden/make_hnr_bars.py), never anything a kernel gave.  The
lag tau* is compared where the restatement's best lag leads its runner-up by more than the bar of r'; at the other frames, at most
1 % of the valid ones, r and hnr are compared with the restatement evaluated at the kernel's lag.  Every batch's padding is NaN."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import yaml
from scipy.io import wavfile

from fastspeech2_amd import hnr as H
from fastspeech2_amd import metrics as M
from tests import f0_signals as S
from tests import hnr_ref as ref
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "hnr_bars.json")))
SLACK = -7.0
LD = np.longdouble


def bar(case, key):
    return BARS["factor"] * BARS["distance"][case][key]


def same(u, v):
    return u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _case(name):
    """the rows of a case and the restatement's frames of each, computed once"""
    fs, hop, rows = ref.case_input(name)
    return fs, hop, rows, [ref.frames(y, f0, fs, hop) for y, f0 in rows]


def _audio(rows, dev, strided=False):
    """[(y, f0)] -> y (B, Nmax) float32, lens, f0 (B, Tmax) float64, frames: NaN beyond every row; `strided`: views into larger buffers"""
    lens, frames = [len(y) for y, _ in rows], [len(f) for _, f in rows]
    pad = 5 if strided else 0
    yb, fb = np.full((len(rows), max(lens) + pad), np.nan, np.float32), np.full((len(rows), max(frames) + pad), np.nan)
    for b, (y, f) in enumerate(rows):
        yb[b, :lens[b]], fb[b, :frames[b]] = y, f
    return torch.from_numpy(yb).to(dev)[:, :max(lens)], lens, torch.from_numpy(fb).to(dev)[:, :max(frames)], frames


def _frames3(rows, dev, strided=False):
    """[(T, 3)] -> (B, Tmax, 3) float64 with NaN beyond every row's frames; `strided`: wider rows and a longer batch stride"""
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(lens) + (2 if strided else 0), 3 + (2 if strided else 0)), np.nan)
    for b, r in enumerate(rows):
        x[b, :lens[b], :3] = r
    return torch.from_numpy(x).to(dev)[:, :max(lens), :3], lens


def _check_frames(name, b, y, f0, fs, hop, got, got_lag, want):
    """one row of the frame kernel's output against the restatement, by the comparison rule of the module docstring -> the number
    of valid frames and of those left out of the lag comparison"""
    fr, lag, _, margin = want
    assert np.array_equal(got[:, 2], fr[:, 2]) and np.isfinite(got).all()
    valid = fr[:, 2] != 0
    assert not got[~valid].any() and not got_lag[~valid].any()
    sure = valid & (margin > bar(name, "rprime"))
    assert np.array_equal(got_lag[sure], lag[sure])
    if not np.array_equal(got_lag[valid], lag[valid]):                      # a tie within rounding: the restatement at the kernel's lag
        fr = ref.frames(y, f0, fs, hop, lags=got_lag)[0]
    if valid.any():
        w_r, w_h = float(np.abs(got[valid, 0] - fr[valid, 0]).max()), float(np.abs(got[valid, 1] - fr[valid, 1]).max())
        print(f"{name}[{b}] T={len(f0)} valid={int(valid.sum())}: r {w_r:.2e} (bar {bar(name, 'r'):.2e}), hnr {w_h:.2e} (bar {bar(name, 'hnr'):.2e})")
        assert w_r <= bar(name, "r") and w_h <= bar(name, "hnr")
    return int(valid.sum()), int((valid & ~sure).sum())


# ------------------------------------------------------------------------------------------------ each kernel alone
@pytest.mark.parametrize("name", list(ref.CASES))
def test_frames_against_the_restatement(dev, name):
    """fs4000 runs on strided views and writes into buffers larger than needed, whose slack must stay.  The cases hold T = 1, a row
    shorter than one window, frames crossing either end, F0 at F0_FLOOR and F0_CEIL, unvoiced frames and an all-zero stretch."""
    fs, hop, rows, want = _case(name)
    odd = name == "fs4000"
    y, lens, f0, frames = _audio(rows, dev, strided=odd)
    B, Tmax = len(rows), max(frames)
    out = torch.full((B, Tmax + 2, 4), SLACK, dtype=torch.float64, device=dev) if odd else None
    out_lag = torch.full((B, Tmax + 3), -7, dtype=torch.int32, device=dev) if odd else None
    fr, lag = H.frames(y, lens, f0, frames, fs, hop, out=out, out_lag=out_lag)
    frh, lagh = fr.cpu().numpy(), lag.cpu().numpy()
    assert fr.shape == ((B, Tmax + 2, 4) if odd else (B, Tmax, 3)) and lag.dtype == torch.int32
    n_valid = n_left = 0
    for b, (yb, fb) in enumerate(rows):
        T = frames[b]
        v, left = _check_frames(name, b, yb, fb, fs, hop, frh[b, :T, :3], lagh[b, :T], want[b])
        n_valid, n_left = n_valid + v, n_left + left
        if odd:
            assert np.all(frh[b, T:] == SLACK) and np.all(frh[b, :, 3] == SLACK) and np.all(lagh[b, T:] == -7)
    assert n_valid == BARS["valid_frames"][name] and 100 * n_left <= n_valid
    if name == "fs22050":                                                   # the long row's special frames are what they are meant to be
        g, l = frh[2, :frames[2]], lagh[2, :frames[2]]
        lmax = H.window(fs)[2]
        assert not g[3:6, 2].any() and not g[9, 2] and not g[27:33, 2].any() and g[7, 2] and g[8, 2]
        assert 259 <= l[7] <= lmax - 1 and 23 <= l[8] <= 33


def test_a_ragged_batch_two_runs_and_the_rows_alone_give_the_same_bytes(dev):
    for name in ("fs4000", "fs22050"):
        fs, hop, rows, want = _case(name)
        y, lens, f0, frames = _audio(rows, dev)
        (f1, l1), (f2, l2) = H.frames(y, lens, f0, frames, fs, hop), H.frames(y, lens, f0, frames, fs, hop)
        s1, s2 = H.side(f1, frames), H.side(f2, frames)
        assert same(s1, s2)
        for b, T in enumerate(frames):
            ya, la, fa, ta = _audio(rows[b:b + 1], dev)
            fr, lg = H.frames(ya, la, fa, ta, fs, hop)
            assert same(f1[b, :T], f2[b, :T]) and same(l1[b, :T], l2[b, :T]) and same(f1[b, :T], fr[0]) and same(l1[b, :T], lg[0])
            assert same(s1[b], H.side(fr, ta)[0])


@pytest.mark.parametrize("name", list(ref.CASES))
def test_side_moments_against_the_restatement(dev, name):
    _, _, rows, want = _case(name)
    fr, frames = _frames3([w[0] for w in want], dev, strided=name == "fs4000")      # the restatement's frames: this kernel alone
    out = torch.full((len(rows), 5), SLACK, dtype=torch.float64, device=dev)
    stats = H.side(fr, frames, out=out).cpu().numpy()
    for b, w in enumerate(want):
        n, m, m2 = ref.side(w[0])
        print(f"{name}[{b}]: n {int(n)}, mean {abs(stats[b, 1] - m):.2e} (bar {bar(name, 'side_mean'):.2e}), M2 {abs(stats[b, 2] - m2):.2e} "
              f"(bar {bar(name, 'side_m2'):.2e})")
        assert stats[b, 0] == n and abs(stats[b, 1] - m) <= bar(name, "side_mean") and abs(stats[b, 2] - m2) <= bar(name, "side_m2")
    assert np.all(stats[:, 3:] == SLACK)
    none = H.side(torch.zeros(1, 4, 3, dtype=torch.float64, device=dev), [4]).cpu().numpy()
    assert none.tolist() == [[0.0, 0.0, 0.0]]


def test_path_sums_on_the_hand_built_paths(dev):
    """P_v = 0, P_v = 1, invalid frames on one side only, a diagonal and a corner path with invalid frames on both sides, as one
    ragged launch on non-contiguous frames and into an oversized buffer; then each pair alone gives the same bytes"""
    names = list(ref.PATH_CASES)
    data = [ref.path_case(n) for n in names]
    fa, al = _frames3([d[0] for d in data], dev, strided=True)
    fb, bl = _frames3([d[1] for d in data], dev, strided=True)
    L = max(al) + max(bl) - 1
    pi, pj = np.full((len(data), L), -1, np.int32), np.full((len(data), L), -1, np.int32)
    for b, d in enumerate(data):
        pi[b, :len(d[2])], pj[b, :len(d[3])] = d[2], d[3]
    plen = torch.tensor([len(d[2]) for d in data], dtype=torch.int32, device=dev)
    pi, pj = torch.from_numpy(pi).to(dev), torch.from_numpy(pj).to(dev)
    out = torch.full((len(names), 9), SLACK, dtype=torch.float64, device=dev)
    sums = H.on_path(pi, pj, plen, fa, al, fb, bl, out=out)
    again = H.on_path(pi, pj, plen, fa, al, fb, bl)
    assert same(sums[:, :7], again)
    sh = sums.cpu().numpy()
    for b, (name, d) in enumerate(zip(names, data)):
        want = ref.path_sums(d[2], d[3], d[0], d[1])
        w_m, w_s = float(np.abs(sh[b, 1:3] - want[1:3]).max()), float(np.abs(sh[b, 3:7] - want[3:]).max())
        print(f"{name}: P_v {int(want[0])}, means {w_m:.2e} (bar {bar(name, 'path_mean'):.2e}), sums {w_s:.2e} (bar {bar(name, 'path_sums'):.2e})")
        assert sh[b, 0] == want[0] and w_m <= bar(name, "path_mean") and w_s <= bar(name, "path_sums")
        one = H.on_path(pi[b:b + 1, :len(d[2])].contiguous(), pj[b:b + 1, :len(d[2])].contiguous(), plen[b:b + 1], *_frames3([d[0]], dev),
                        *_frames3([d[1]], dev))
        assert same(one[0], again[b])
    assert np.all(sh[:, 7:] == SLACK) and sh[0, :7].tolist() == [0.0] * 7 and sh[1, 0] == 1 and sh[1, 3:6].tolist() == [0.0] * 3
    assert sh[2, 0] == 40 - 13 and sh[1, 6] > 0
    rows = [H.row_scores(sh[b, :7], [1, 0.0, 0.0], [1, 0.0, 0.0]) for b in range(3)]
    assert np.isnan([rows[0][k] for k in ("hnr_diff_db", "hnr_rmse_db", "hnr_corr")]).all() and np.isnan(rows[1]["hnr_corr"])
    assert rows[1]["hnr_diff_db"] == sh[1, 2] - sh[1, 1] and np.isfinite(rows[2]["hnr_corr"])


def test_bad_arguments_are_refused_before_launch(dev):
    from fastspeech2_amd import _lib, ops
    y = torch.zeros(2, 4000, dtype=torch.float32, device=dev)
    f0 = torch.full((2, 16), 150.0, dtype=torch.float64, device=dev)
    good = (y, [4000, 4000], f0, [16, 16])
    H.frames(*good, 22050, 256)
    for args in ((y.double(), [4000, 4000], f0, [16, 16]), (y, [4000, 4001], f0, [16, 16]), (y, [4000, 0], f0, [16, 16]), (y, [4000], f0, [16, 16]),
                 (y, [4000, 4000], f0.float(), [16, 16]), (y, [4000, 4000], f0, [16, 17]), (y, [4000, 4000], f0, [0, 16]), (y, [4000, 4000], f0[:1], [16]),
                 (y[:, ::2], [2000, 2000], f0, [16, 16]), (y[0], [4000], f0, [16, 16]), (y.cpu(), [4000, 4000], f0, [16, 16]),
                 (y, [4000, 4000], f0.cpu(), [16, 16]), (y[:1].expand(2, 4000), [4000, 4000], f0, [16, 16]),
                 (y, [4000, 4000], torch.zeros(2, 2049, dtype=torch.float64, device=dev), [2049, 16])):
        with pytest.raises(ValueError):
            H.frames(*args, 22050, 256)
    for fs, hop in ((200000, 256), (50, 1), (22050.5, 256), (22050, 0), (22050, 2.5)):
        with pytest.raises(ValueError):
            H.frames(*good, fs, hop)
    with pytest.raises(ValueError):
        H.frames(*good, 22050, 256, out=torch.zeros(2, 15, 3, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        H.frames(*good, 22050, 256, out=torch.zeros(2, 16, 2, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        H.frames(*good, 22050, 256, out_lag=torch.zeros(2, 16, dtype=torch.int64, device=dev))
    fr = torch.zeros(2, 16, 3, dtype=torch.float64, device=dev)
    for bad, lens in ((fr[:, :, :2], [16, 16]), (fr.float(), [16, 16]), (fr, [16, 17]), (fr, [16]), (fr[0], [16]), (fr[:1].expand(2, 16, 3), [16, 16])):
        with pytest.raises(ValueError):
            H.side(bad, lens)
    pi = torch.zeros(2, 31, dtype=torch.int32, device=dev)
    plen = torch.ones(2, dtype=torch.int32, device=dev)
    for args in ((pi, pi[:, :30], plen, fr, [16, 16], fr, [16, 16]), (pi, pi, plen[:1], fr, [16, 16], fr, [16, 16]), (pi, pi, plen, fr[:1], [16], fr, [16, 16]),
                 (pi, pi, plen, fr, [16, 17], fr, [16, 16]), (pi, pi, plen, fr, [16, 16], fr.float(), [16, 16]), (pi.long(), pi.long(), plen, fr, [16, 16], fr, [16, 16]),
                 (pi, pi, plen, fr, [16, 16], fr.cpu(), [16, 16])):
        with pytest.raises(ValueError):
            H.on_path(*args)
    with pytest.raises(ValueError):
        H.on_path(pi, pi, plen, fr, [16, 16], fr, [16, 16], out=torch.zeros(2, 6, dtype=torch.float64, device=dev))
    # the C entry points themselves
    lens = torch.tensor([4000, 4000], dtype=torch.int32, device=dev)
    frames = torch.tensor([16, 16], dtype=torch.int32, device=dev)
    w, rw = H._tables_on(dev, 22050)
    lag = torch.zeros(2, 16, dtype=torch.int32, device=dev)
    ok = dict(ldf=16, h=698, lmax=312, ldo_b=48, ldo_t=3, ldl=16, T=16, hop=256, fs=22050.0)
    for change in (dict(ldf=15), dict(h=0), dict(h=4096), dict(lmax=2), dict(lmax=1397), dict(ldo_b=47), dict(ldo_t=2), dict(ldl=15), dict(T=0),
                   dict(T=2049), dict(hop=0), dict(fs=0.0)):
        a = dict(ok, **change)
        with pytest.raises(ValueError):
            _lib.call("fs2_hnr_frames", y.data_ptr(), 4000, lens.data_ptr(), f0.data_ptr(), a["ldf"], frames.data_ptr(), w.data_ptr(), rw.data_ptr(),
                      a["fs"], a["hop"], a["h"], a["lmax"], fr.data_ptr(), a["ldo_b"], a["ldo_t"], lag.data_ptr(), a["ldl"], 2, a["T"], ops._stream())
    stats = torch.zeros(2, 3, dtype=torch.float64, device=dev)
    for ldf_b, ldf_t, lds in ((47, 3, 3), (48, 2, 3), (48, 3, 2)):
        with pytest.raises(ValueError):
            _lib.call("fs2_hnr_side", fr.data_ptr(), ldf_b, ldf_t, frames.data_ptr(), stats.data_ptr(), lds, 2, 16, ops._stream())
    sums = torch.zeros(2, 7, dtype=torch.float64, device=dev)
    for lda_b, lda_t, ldo, T1 in ((47, 3, 7, 16), (48, 2, 7, 16), (48, 3, 6, 16), (48, 3, 7, 0), (48, 3, 7, 17)):
        with pytest.raises(ValueError):
            _lib.call("fs2_hnr_on_path", pi.data_ptr(), pi.data_ptr(), 31, plen.data_ptr(), fr.data_ptr(), lda_b, lda_t, fr.data_ptr(), 48, 3,
                      frames.data_ptr(), frames.data_ptr(), sums.data_ptr(), ldo, 2, T1, 16, ops._stream())
    assert _lib.load().fs2_hnr_max_window() == H.MAX_WINDOW and not fr.any() and not lag.any() and not stats.any() and not sums.any()


# ------------------------------------------------------------------------------------------------ the known answers, on the device
def test_known_answers_on_the_device(dev):
    """the pass conditions of tests/test_hnr_cpu.py on signals made the same way, as one batch of 17 rows"""
    fs, hop = 22050, 256
    rng = np.random.default_rng(9701)
    T = ref.n_frames(fs, hop)
    rows, what = [], []
    for f in (100.0, 147.0, 220.5, 300.0):
        for snr in (20.0, 10.0, 0.0, None):
            rows.append((ref.tone(f, fs, fs, rng, snr), np.full(T, f)))
            what.append((f, snr))
    rows.append(((0.1 * np.random.default_rng(9702).standard_normal(fs)).astype(np.float32), np.full(T, 150.0)))
    y, lens, f0, frames = _audio(rows, dev)
    fr, _ = H.frames(y, lens, f0, frames, fs, hop)
    stats = H.side(fr, frames).cpu().numpy()
    hnr = fr.cpu().numpy()[:, 4:T - 4]
    assert hnr.shape[1] >= 20 and hnr[:, :, 2].all() and np.all(stats[:, 0] == T)
    for b, (f, snr) in enumerate(what):
        print(f"{f} Hz at {snr} dB: mean {hnr[b, :, 1].mean():.3f} dB, min {hnr[b, :, 1].min():.2f} dB")
        if snr is None:
            assert hnr[b, :, 1].min() >= 30.0
        else:
            assert abs(hnr[b, :, 1].mean() - snr) <= 1.0
    print(f"white noise at 150 Hz: mean {hnr[16, :, 1].mean():.2f} dB")
    assert hnr[16, :, 1].mean() < -5.0


# ------------------------------------------------------------------------------------------------ end to end
def _tones(f0s, durs, rng=None, snr=None):
    y = np.concatenate([S.tone(f, d) for f, d in zip(f0s, durs)])
    return y if snr is None else ref.noisier(y, rng, snr)


def _pairs():
    """four short (recorded, synthesized) pairs of tone sequences: a copy, a noisier copy, another melody in noise, a shorter side"""
    rng = np.random.default_rng(9801)
    base = _tones((200.0, 260.0, 150.0), (0.25, 0.2, 0.3), rng, 30.0)
    return [(base, base.copy()), (base, ref.noisier(base, rng, 10.0)), (base, _tones((110.0, 330.0), (0.4, 0.3), rng, 15.0)),
            (base, _tones((180.0, 240.0), (0.2, 0.25), rng, 20.0))]


def _stft(cfg):
    from fastspeech2_amd import audio as Audio
    pp = cfg["preprocessing"]
    return Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"], pp["mel"]["n_mel_channels"],
                              pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])


def test_score_pairs_keeps_every_old_key_and_adds_the_chained_restatements_scores(dev, monkeypatch):
    """The audio, the F0 tracks and the path each batch hands to the kernels are recorded on the way; the restatement's whole chain
    on them is the reference, and the bar of a key is 16 times the distance between that chain in fp64 and in longdouble (at the
    fp64 chain's lags)."""
    pairs = _pairs()
    stft = _stft(config("/nowhere"))
    refs, syns = [p[0] for p in pairs], [p[1] for p in pairs]
    plain = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, wavelet=True)
    rows = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, wavelet=True, hnr=True)
    seen = {"side": [], "path": []}
    measure, on_path = H.measure, H.on_path

    def spy_measure(y, lens, f0, frames, fs, hop):
        seen["side"].append([(y[b, :n].cpu().numpy(), f0[b, :T].cpu().numpy()) for b, (n, T) in enumerate(zip(lens, frames))])
        return measure(y, lens, f0, frames, fs, hop)

    def spy_on_path(pi, pj, plen, *rest):
        seen["path"].append([(pi[b, :int(P)].cpu().numpy(), pj[b, :int(P)].cpu().numpy()) for b, P in enumerate(plen.cpu())])
        return on_path(pi, pj, plen, *rest)

    monkeypatch.setattr(H, "measure", spy_measure)
    monkeypatch.setattr(H, "on_path", spy_on_path)
    again = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, wavelet=True, hnr=True, budget=1)       # one pair per batch
    assert json.dumps(rows) == json.dumps(again) and len(seen["path"]) == 4 and len(seen["side"]) == 8
    new = set(ref.KEYS)
    for r, p in zip(rows, plain):
        assert set(r) == set(p) | new and json.dumps({k: v for k, v in r.items() if k not in new}) == json.dumps(p)
    order = sorted(range(4), key=lambda i: (-rows[i]["frames_ref"], -rows[i]["frames_syn"], i))     # longest first: the batches' order
    want, exact = [None] * 4, [None] * 4
    for n, i in enumerate(order):
        (ya, f0a), (yb, f0b), (pi, pj) = seen["side"][2 * n][0], seen["side"][2 * n + 1][0], seen["path"][n][0]
        assert len(f0a) == rows[i]["frames_ref"] and len(f0b) == rows[i]["frames_syn"] and len(pi) == rows[i]["path_len"]
        fa, la = ref.frames(ya, f0a, S.FS, S.HOP)[:2]
        fb, lb = ref.frames(yb, f0b, S.FS, S.HOP)[:2]
        want[i] = ref.row_scores(fa, fb, pi, pj)
        exact[i] = ref.row_scores(ref.frames(ya, f0a, S.FS, S.HOP, LD, lags=la)[0], ref.frames(yb, f0b, S.FS, S.HOP, LD, lags=lb)[0], pi, pj, LD)
    for key in ref.KEYS:
        got, w = (np.array([r[key] for r in src], np.float64) for src in (rows, want))
        assert np.array_equal(np.isnan(got), np.isnan(w)), key
        ok = ~np.isnan(w)
        limit = 16 * float(np.abs(np.array([r[key] for r in want], LD) - np.array([r[key] for r in exact], LD))[ok].max())
        worst = float(np.abs(got - w)[ok].max())
        print(f"{key}: largest distance {worst:.2e}, bar {limit:.2e}")
        assert worst <= limit, key
    assert rows[0]["hnr_diff_db"] == 0.0 and rows[0]["hnr_rmse_db"] == 0.0 and rows[1]["hnr_diff_db"] < -5.0 and rows[0]["hnr_cells"] > 20
    assert rows[1]["hnr_mean_db_ref"] == rows[0]["hnr_mean_db_ref"] and rows[1]["hnr_mean_db_syn"] < rows[0]["hnr_mean_db_syn"]
    summary = M.summarize(rows)
    assert summary["hnr_unscored_utterances"] == 0 and summary["hnr_cells"] == sum(r["hnr_cells"] for r in rows) and summary["hnr_diff_db"] < 0
    assert "hnr_cells" not in M.summarize(plain) and set(M.summarize(plain)) < set(summary)
    pyin = M.score_pairs(refs[:1], syns[:1], stft, S.FS, S.HOP, device=dev, hnr=True, f0_estimator="pyin", cepstra="world", n_mcep=None)
    assert new <= set(pyin[0]) and pyin[0]["hnr_diff_db"] == 0.0 and pyin[0]["f0_estimator"] == "pyin" and pyin[0]["cepstra"] == "world"
    with pytest.raises(ValueError):
        M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, f0=False, hnr=True)


def test_score_hnr_end_to_end(dev, tmp_path, capsys):
    import score
    root = str(tmp_path)
    for k, (x, y) in enumerate(_pairs()[1:]):
        for folder, w in ((os.path.join("raw", "spk"), x), ("result", y)):
            os.makedirs(os.path.join(root, folder), exist_ok=True)
            wavfile.write(os.path.join(root, folder, f"u{k}.wav"), S.FS, np.round(np.clip(w, -1, 1) * 32767).astype(np.int16))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"u{k}|spk|{{AA B}}|text {k}\n" for k in range(3)))
    for name, doc in (("preprocess.yaml", config(root)), ("train.yaml", {"path": {"result_path": os.path.join(root, "result")}})):
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    argv = ["-p", os.path.join(root, "preprocess.yaml"), "-t", os.path.join(root, "train.yaml"), "--source", os.path.join(root, "val.txt"),
            "--out", os.path.join(root, "s.jsonl")]
    plain, _, summary0 = score.main(argv)
    capsys.readouterr()
    rows, skipped, summary = score.main(argv + ["--hnr"])
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    new = {"hnr_frames_ref", "hnr_frames_syn", "hnr_mean_db_ref", "hnr_mean_db_syn", "hnr_cells", "hnr_diff_db", "hnr_rmse_db", "hnr_corr_mean",
           "hnr_corr_nan_utterances", "hnr_unscored_utterances"}
    assert not skipped and set(summary) == set(summary0) | new and not new & set(summary0) and set(said) == set(summary)
    assert {k: summary[k] for k in summary0} == summary0 and "hnr_cells" not in plain[0] and set(ref.KEYS) <= set(rows[0])
    for r, p in zip(rows, plain):
        assert json.dumps({k: v for k, v in r.items() if k not in ref.KEYS}) == json.dumps(p)
    assert summary["hnr_unscored_utterances"] == 0 and summary["hnr_cells"] == sum(r["hnr_cells"] for r in rows) and rows[0]["hnr_diff_db"] < -5.0
    written = [json.loads(line) for line in open(os.path.join(root, "s.jsonl"))]
    assert [r["basename"] for r in written] == ["u0", "u1", "u2"] and written[0]["hnr_corr"] == rows[0]["hnr_corr"]
    with pytest.raises(SystemExit):
        score.main(argv + ["--hnr", "--no_f0"])
