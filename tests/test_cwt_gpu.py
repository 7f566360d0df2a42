"""GPU wavelet prosody scores (fastspeech2_amd/cwt.py, csrc/fs2_cwt.hip) against the fp64 restatement tests/cwt_ref.py: each kernel
alone, fed the restatement's own upstream values (the contour kernel the F0 tracks, the transform kernel the restatement's z, the
path kernel the restatement's W), then the known answers of the specification, `metrics.score_pairs(wavelet=True)` and score.py
--wavelet end to end.  Floating outputs are held to the bars of tests/golden/cwt_bars.json: per case and output 16 times the
distance between the fp64 and the longdouble restatement of that stage on that case's input (tests/golden/make_cwt_bars.py), never
anything a kernel gave; where that distance is 0 (the z, W and power of flat rows) the kernel matches exactly.  Every batch's
padding is NaN."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml
from scipy.io import wavfile

from fastspeech2_amd import cwt as C
from fastspeech2_amd import metrics as M
from tests import cwt_ref as ref
from tests import f0_signals as S
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "cwt_bars.json")))
SLACK = -7.0
EPS = 2.0 ** -52
LD = np.longdouble


def bar(case, key):
    return BARS["factor"] * BARS["distance"][case][key]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the tracks of a case, the restatement's contour of each, and its transform of that z at both rate pairs, computed once"""
    rows = ref.case_input(name)
    contours = [ref.contour(f0) for f0 in rows]
    return rows, contours, {rate: [ref.transform(c["z"], *rate) for c in contours] for rate in ref.RATES}


def _batch(rows, dev, strided=False):
    """(B, Tmax) with NaN beyond every row's frames; `strided`: a view into a larger NaN buffer"""
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(lens) + (5 if strided else 0)), np.nan)
    for b, r in enumerate(rows):
        x[b, :lens[b]] = r
    return torch.from_numpy(x).to(dev)[:, :max(lens)], lens


def _batch3(rows, dev, strided=False):
    """[(10, T)] -> (B, 10, Tmax) with NaN beyond every row's frames; `strided`: non-contiguous batch and scale strides"""
    lens = [r.shape[1] for r in rows]
    x = np.full((len(rows), 10 + (2 if strided else 0), max(lens) + (3 if strided else 0)), np.nan)
    for b, r in enumerate(rows):
        x[b, :10, :lens[b]] = r
    return torch.from_numpy(x).to(dev)[:, :10, :max(lens)], lens


def _worst(got, want):
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max())


def _slack(dev, *shape):
    return torch.full(shape, SLACK, dtype=torch.float64, device=dev)


# ------------------------------------------------------------------------------------------------ each kernel alone
@pytest.mark.parametrize("name", list(ref.CASES))
def test_contour_against_the_restatement(dev, name):
    """mixed5 runs on a strided view and writes into a buffer larger than needed, whose slack must stay"""
    rows, contours, _ = _case(name)
    odd = name == "mixed5"
    f0, lens = _batch(rows, dev, strided=odd)
    B, Tmax = len(rows), max(lens)
    out = _slack(dev, B, Tmax + 4) if odd else None
    z, stats = C.contour(f0, lens, out=out)
    zh, sh = z.cpu().numpy(), stats.cpu().numpy()
    assert stats.shape == (B, 4) and z.shape == ((B, Tmax + 4) if odd else (B, Tmax))
    for b, (T, c) in enumerate(zip(lens, contours)):
        assert sh[b, 0] == c["n_voiced"] and sh[b, 3] == c["flat"]
        w_z, w_m, w_sd = _worst(zh[b, :T], c["z"]), abs(sh[b, 1] - c["m"]), abs(sh[b, 2] - c["sd"])
        print(f"{name}[{b}] T={T}: z {w_z:.2e} (bar {bar(name, 'z'):.2e}), m {w_m:.2e} (bar {bar(name, 'm'):.2e}), sd {w_sd:.2e} "
              f"(bar {bar(name, 'sd'):.2e})")
        assert w_z <= bar(name, "z") and w_m <= bar(name, "m") and w_sd <= bar(name, "sd")
        if c["flat"]:
            assert not zh[b, :T].any()
        if odd:
            assert np.all(zh[b, T:] == SLACK)
    if name == "degenerate":
        assert sh[:, 3].tolist() == [1, 1, 1] and sh[0].tolist() == [0, 0, 0, 1] and sh[1, 0] == 256 and sh[2, 0] == 1


def test_a_flat_row_of_any_length_is_zero_and_says_so(dev):
    """all unvoiced, a constant track and one voiced frame at frame counts that are no power of two: whatever the rounding of the
    mean leaves in sd, it is below 1e-12, and z, flat and the voiced count are exact"""
    rows = [np.zeros(257), np.full(300, 150.0), ref.track(np.random.default_rng(5), 77, "one"), np.full(1, 220.0), np.full(2048, 97.3)]
    f0, lens = _batch(rows, dev)
    z, stats = C.contour(f0, lens)
    zh, sh = z.cpu().numpy(), stats.cpu().numpy()
    assert sh[:, 0].tolist() == [0, 300, 1, 1, 2048] and sh[:, 3].tolist() == [1] * 5 and np.all(sh[:, 2] <= 1e-12) and sh[0, 1] == 0
    for b, T in enumerate(lens):
        assert not zh[b, :T].any()
        if b:
            assert abs(sh[b, 1] - math.log(rows[b].max())) <= 2 * EPS * 6        # the device's logarithm and one division


@pytest.mark.parametrize("rate", ref.RATES, ids=lambda r: f"{r[0]}_{r[1]}")
@pytest.mark.parametrize("name", list(ref.CASES))
def test_transform_against_the_restatement(dev, name, rate):
    rows, contours, transforms = _case(name)
    odd = name == "mixed5"
    z, lens = _batch([c["z"] for c in contours], dev, strided=odd)           # the restatement's z: this kernel alone is under test
    B, Tmax = len(rows), max(lens)
    out, outp = (_slack(dev, B, 12, Tmax + 3), _slack(dev, B, 13)) if odd else (None, None)
    W, power = C.transform(z, lens, *rate, out=out, out_power=outp)
    Wh, ph = W.cpu().numpy(), power.cpu().numpy()
    kw, kp = f"W_{rate[0]}_{rate[1]}", f"power_{rate[0]}_{rate[1]}"
    for b, (T, (Wr, pr)) in enumerate(zip(lens, transforms[rate])):
        w_w, w_p = _worst(Wh[b, :10, :T], Wr), _worst(ph[b, :10], pr)
        print(f"{name}[{b}] T={T} {kw}: W {w_w:.2e} (bar {bar(name, kw):.2e}), power {w_p:.2e} (bar {bar(name, kp):.2e})")
        assert w_w <= bar(name, kw) and w_p <= bar(name, kp)
        if contours[b]["flat"]:
            assert not Wh[b, :10, :T].any() and not ph[b, :10].any()
        if odd:
            assert np.all(Wh[b, :10, T:] == SLACK)
    if odd:
        assert np.all(Wh[:, 10:] == SLACK) and np.all(ph[:, 10:] == SLACK)
    else:
        assert W.shape == (B, 10, Tmax) and power.shape == (B, 10)


@functools.lru_cache(maxsize=None)
def _path_case(name):
    f0a, f0b, pi, pj = ref.path_case(name)
    Wa, Wb = (ref.transform(ref.contour(f)["z"], *ref.RATES[0])[0] for f in (f0a, f0b))
    return Wa, Wb, pi, pj, ref.path_sums(pi, pj, Wa, Wb)


def _paths(cases, dev, strided=False):
    """the hand-built path cases as one ragged launch: path rows end with -1 as `metrics.backtrack` leaves them"""
    data = [_path_case(n) for n in cases]
    Wa, al = _batch3([d[0] for d in data], dev, strided)
    Wb, bl = _batch3([d[1] for d in data], dev, strided)
    L = max(al) + max(bl) - 1
    pi, pj = np.full((len(data), L), -1, np.int32), np.full((len(data), L), -1, np.int32)
    for b, d in enumerate(data):
        pi[b, :len(d[2])], pj[b, :len(d[3])] = d[2], d[3]
    plen = torch.tensor([len(d[2]) for d in data], dtype=torch.int32, device=dev)
    return torch.from_numpy(pi).to(dev), torch.from_numpy(pj).to(dev), plen, Wa, al, Wb, bl, [d[4] for d in data]


def test_path_sums_on_the_hand_built_paths(dev):
    """diagonal, all-horizontal-then-vertical, and that one at the frame bound (P = 4095), as one ragged launch on non-contiguous
    transforms and into an oversized buffer"""
    names = list(ref.PATH_CASES)
    pi, pj, plen, Wa, al, Wb, bl, want = _paths(names, dev, strided=True)
    assert int(plen.max()) == 4095
    out = _slack(dev, len(names), 17, 6)
    sums = C.on_path(pi, pj, plen, Wa, al, Wb, bl, out=out).cpu().numpy()
    for b, name in enumerate(names):
        worst = _worst(sums[b, :15, :4], want[b])
        print(f"{name}: sums {worst:.2e} (bar {bar(name, 'sums'):.2e})")
        assert worst <= bar(name, "sums")
    assert np.all(sums[:, 15:] == SLACK) and np.all(sums[:, :, 4:] == SLACK)
    assert np.all(sums[0, :15, 3] > 0)                                      # the diagonal pair is two different tracks


def test_path_sums_on_a_real_dtw_path(dev):
    """two pairs of random cepstra through `metrics.dtw`; the bar is 16 times the restatement's own fp64-to-longdouble distance on
    this path, measured here"""
    rng = np.random.default_rng(9401)
    al, bl = [120, 90], [150, 64]
    a = torch.from_numpy(rng.standard_normal((2, 120, 13)).cumsum(axis=1)).to(dev)
    b = torch.from_numpy(rng.standard_normal((2, 150, 13)).cumsum(axis=1)).to(dev)
    _, plen, pi, pj = M.dtw(a, al, b, bl)
    Wa = [ref.transform(ref.contour(ref.track(rng, T, "runs"))["z"], *ref.RATES[1])[0] for T in al]
    Wb = [ref.transform(ref.contour(ref.track(rng, T, "runs"))["z"], *ref.RATES[1])[0] for T in bl]
    sums = C.on_path(pi, pj, plen, _batch3(Wa, dev)[0], al, _batch3(Wb, dev)[0], bl).cpu().numpy()
    assert sums.shape == (2, 15, 4)
    for p in range(2):
        P = int(plen[p])
        qi, qj = pi[p, :P].cpu().numpy(), pj[p, :P].cpu().numpy()
        assert max(al[p], bl[p]) <= P < al[p] + bl[p] and qi[-1] == al[p] - 1 and qj[-1] == bl[p] - 1
        want, exact = ref.path_sums(qi, qj, Wa[p], Wb[p]), ref.path_sums(qi, qj, Wa[p], Wb[p], LD)
        limit = 16 * float(np.abs(want - exact).max())
        worst = _worst(sums[p], want)
        print(f"dtw[{p}] P={P}: sums {worst:.2e} (bar {limit:.2e})")
        assert 0 < limit and worst <= limit


def test_two_launches_give_the_same_bytes_and_a_row_does_not_depend_on_its_batch(dev):
    rows, contours, _ = _case("lengths")
    f0, lens = _batch(rows, dev)
    (z1, s1), (z2, s2) = C.contour(f0, lens), C.contour(f0, lens)
    same = lambda u, v: u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()     # noqa: E731
    T = lens[4]
    f1, l1 = _batch(rows[4:5], dev)
    za, sa = C.contour(f1, l1)
    assert same(z1[:, :1], z2[:, :1]) and same(s1, s2) and same(s1[4:5], sa) and same(z1[4:5, :T], za)
    for b, n in enumerate(lens):
        assert same(z1[b, :n], z2[b, :n])
    zin, _ = _batch([c["z"] for c in contours], dev)
    (W1, p1), (W2, p2) = C.transform(zin, lens, *ref.RATES[0]), C.transform(zin, lens, *ref.RATES[0])
    Wa, pa = C.transform(_batch([contours[4]["z"]], dev)[0], l1, *ref.RATES[0])
    assert same(p1, p2) and same(p1[4:5], pa) and same(W1[4:5, :, :T], Wa)
    for b, n in enumerate(lens):
        assert same(W1[b, :, :n], W2[b, :, :n])
    args = _paths(list(ref.PATH_CASES), dev)[:7]
    one = _paths(["corner"], dev)[:7]
    q1, q2, qa = C.on_path(*args), C.on_path(*args), C.on_path(*one)
    assert same(q1, q2) and same(q1[1:2], qa)


# ------------------------------------------------------------------------------------------------ the known answers, on the device
def _pair_on_device(f0_ref, f0_syn, dev, rate=ref.RATES[0]):
    """the three kernels chained on one pair along the diagonal -> its row"""
    T = len(f0_ref)
    assert len(f0_syn) == T
    Wa, pa, sa = C.measure(_batch([f0_ref], dev)[0], [T], *rate)
    Wb, pb, sb = C.measure(_batch([f0_syn], dev)[0], [T], *rate)
    k = torch.arange(T, dtype=torch.int32, device=dev)[None]
    sums = C.on_path(k, k.clone(), torch.tensor([T], dtype=torch.int32, device=dev), Wa, [T], Wb, [T])
    return C.row_scores(sums.cpu().numpy()[0], T, pa.cpu().numpy()[0], T, sa.cpu().numpy()[0], pb.cpu().numpy()[0], T, sb.cpu().numpy()[0])


def test_known_answer_1_two_voiced_frames(dev):
    """x = z sd + m: a product, a sum and the device's logarithm away from the closed form, so within 4 fp64 epsilons of ln 400"""
    f0 = np.zeros(9)
    f0[2], f0[6] = 100.0, 400.0
    z, stats = C.contour(_batch([f0], dev)[0], [9])
    zh, (nv, m, sd, flat) = z.cpu().numpy()[0], stats.cpu().numpy()[0]
    want = np.array([math.log(100.0)] * 3 + [math.log(100.0 * 4.0 ** (k / 4.0)) for k in (1, 2, 3)] + [math.log(400.0)] * 3)
    assert (nv, flat) == (2, 0) and float(np.abs(zh * sd + m - want).max()) <= 4 * EPS * math.log(400.0)
    assert _worst(zh, ref.contour(f0)["z"]) <= 16 * float(np.abs(ref.contour(f0)["z"] - ref.contour(f0, LD)["z"]).max())


def test_known_answers_2_3_5_and_6_on_pairs(dev):
    f0 = ref.case_input("mixed5")[4]
    same = _pair_on_device(f0, f0.copy(), dev)                              # 2: a pair against itself
    assert same["cwt_rmse"] == [0.0] * 10 and same["cwt_level_rmse"] == [0.0] * 5 and same["cwt_power_ratio_db"] == [0.0] * 10
    assert np.abs(np.array(same["cwt_corr"] + same["cwt_level_corr"]) - 1).max() <= 1e-15
    half = _pair_on_device(f0, ref.halved(f0), dev)                         # 3: the bars of tests/test_cwt_cpu.py, with their reasons
    assert abs(half["lf0_std_syn"] - 0.5 * half["lf0_std_ref"]) <= 8 * EPS * 6
    assert np.abs(np.array(half["cwt_corr"] + half["cwt_level_corr"]) - 1).max() <= 8 * EPS
    wiggly = ref.wiggly()
    smooth = _pair_on_device(wiggly, ref.moving_average(wiggly), dev)       # 5: a 9-frame moving average
    assert smooth["cwt_power_ratio_db"][0] < smooth["cwt_power_ratio_db"][4] and smooth["cwt_power_ratio_db"][0] < 0
    rows = [dict(same, path_len=len(f0)), dict(half, path_len=len(f0))]
    for flat in (np.zeros(len(f0)), np.full(len(f0), 150.0)):               # 6: a flat side
        row = _pair_on_device(f0, flat, dev)
        assert set(row) == set(ref.KEYS) and all(np.isnan(np.asarray(v, np.float64)).all() for v in row.values())
        rows.append(dict(row, path_len=len(f0)))
    summary = C.summarize(rows)
    assert summary["wavelet_flat_utterances"] == 2 and summary["cwt_corr_nan_utterances"] == [2] * 10
    assert summary["cwt_rmse_mean"] == pytest.approx([0.0] * 10, abs=1e-14)


@pytest.mark.parametrize("rate", ref.RATES, ids=lambda r: f"{r[0]}_{r[1]}")
def test_known_answer_4_a_cosine_peaks_at_its_scale(dev, rate):
    t = np.arange(2048, dtype=np.float64)
    a = ref.scales(*rate)
    z = [np.cos(2 * np.pi * t / (2 * np.pi * a[i - 1] / math.sqrt(2.5))) for i in (3, 4, 5)]
    _, power = C.transform(_batch(z, dev)[0], [2048] * 3, *rate)
    assert (np.argmax(power.cpu().numpy() / C.scale_weights() ** 2, axis=1) + 1).tolist() == [3, 4, 5]


def test_bad_arguments_are_refused_before_launch(dev):
    from fastspeech2_amd import _lib, ops
    f0 = torch.zeros(2, 40, dtype=torch.float64, device=dev)
    for bad, lens in ((f0, [0, 40]), (f0, [40, 41]), (f0, [40]), (f0.float(), [40, 40]), (f0[:, ::2], [20, 20]), (f0[0], [40]), (f0.cpu(), [40, 40]),
                      (torch.zeros(1, 2049, dtype=torch.float64, device=dev), [2049]), (f0[:1].expand(2, 40), [40, 40])):
        with pytest.raises(ValueError):
            C.contour(bad, lens)
        with pytest.raises(ValueError):
            C.transform(bad, lens, 22050, 256)
    with pytest.raises(ValueError):
        C.transform(f0, [40, 40], 16000, 400)
    with pytest.raises(ValueError):
        C.contour(f0, [40, 40], out=torch.zeros(2, 39, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        C.transform(f0, [40, 40], 22050, 256, out=torch.zeros(2, 9, 40, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        C.transform(f0, [40, 40], 22050, 256, out_power=torch.zeros(2, 9, dtype=torch.float64, device=dev))
    W = torch.zeros(2, 10, 40, dtype=torch.float64, device=dev)
    pi = torch.zeros(2, 79, dtype=torch.int32, device=dev)
    plen = torch.ones(2, dtype=torch.int32, device=dev)
    for args in ((pi, pi[:, :78], plen, W, [40, 40], W, [40, 40]), (pi, pi, plen[:1], W, [40, 40], W, [40, 40]), (pi, pi, plen, W[:, :9], [40, 40], W, [40, 40]),
                 (pi, pi, plen, W, [40, 41], W, [40, 40]), (pi, pi, plen, W, [40, 40], W.float(), [40, 40]), (pi.long(), pi.long(), plen, W, [40, 40], W, [40, 40]),
                 (pi, pi, plen, W[:1].expand(2, 10, 40), [40, 40], W, [40, 40])):
        with pytest.raises(ValueError):
            C.on_path(*args)
    with pytest.raises(ValueError):
        C.on_path(pi, pi, plen, W, [40, 40], W, [40, 40], out=torch.zeros(2, 15, 3, dtype=torch.float64, device=dev))
    # the C entry points themselves
    lens = torch.tensor([40, 40], dtype=torch.int32, device=dev)
    z = torch.zeros(2, 40, dtype=torch.float64, device=dev)
    stats = torch.zeros(2, 4, dtype=torch.float64, device=dev)
    for ldf, ldz, lds, T in ((39, 40, 4, 40), (40, 39, 4, 40), (40, 40, 3, 40), (2049, 2049, 4, 2049), (40, 40, 4, 0)):
        with pytest.raises(ValueError):
            _lib.call("fs2_cwt_contour", f0.data_ptr(), ldf, lens.data_ptr(), z.data_ptr(), ldz, stats.data_ptr(), lds, 2, T, ops._stream())
    with pytest.raises(ValueError):
        _lib.call("fs2_cwt_contour", f0.data_ptr(), 40, lens.data_ptr(), f0.data_ptr(), 40, stats.data_ptr(), 4, 2, 40, ops._stream())
    tab, support = C._tables_on(dev, 22050, 256)
    power = torch.zeros(2, 10, dtype=torch.float64, device=dev)
    wide = support.copy()
    wide[9] = 2049
    for sup, ldw_b, ldw_i, ldp in ((wide, 400, 40, 10), (support, 399, 40, 10), (support, 400, 39, 10), (support, 400, 40, 9)):
        with pytest.raises(ValueError):
            _lib.call("fs2_cwt_transform", z.data_ptr(), 40, lens.data_ptr(), tab.data_ptr(), 2048, sup.ctypes.data, W.data_ptr(), ldw_b, ldw_i,
                      power.data_ptr(), ldp, 2, 40, ops._stream())
    sums = torch.zeros(2, 15, 4, dtype=torch.float64, device=dev)
    for ldr_b, ldo_b, ldo_c, T1 in ((399, 60, 4, 40), (400, 59, 4, 40), (400, 60, 3, 40), (400, 60, 4, 41), (400, 60, 4, 0)):
        with pytest.raises(ValueError):
            _lib.call("fs2_cwt_on_path", pi.data_ptr(), pi.data_ptr(), 79, plen.data_ptr(), W.data_ptr(), ldr_b, 40, W.data_ptr(), 400, 40,
                      lens.data_ptr(), lens.data_ptr(), sums.data_ptr(), ldo_b, ldo_c, 2, T1, 40, ops._stream())
    assert _lib.load().fs2_cwt_scales() == C.SCALES and not z.any() and not W.any() and not sums.any()


# ------------------------------------------------------------------------------------------------ end to end
def _tones(f0s, durs):
    return np.concatenate([S.tone(f, d) for f, d in zip(f0s, durs)])


def _pairs():
    """four short (recorded, synthesized) pairs of tone sequences: a copy, another rhythm, another melody, a shorter side"""
    base = _tones((200.0, 260.0, 150.0), (0.25, 0.2, 0.3))
    return [(base, base.copy()), (base, _tones((200.0, 260.0, 150.0), (0.3, 0.15, 0.4))), (base, _tones((110.0, 330.0), (0.4, 0.3))),
            (base, _tones((180.0, 240.0), (0.2, 0.25)))]


def _stft(cfg):
    from fastspeech2_amd import audio as Audio
    pp = cfg["preprocessing"]
    return Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"], pp["mel"]["n_mel_channels"],
                              pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])


def test_score_pairs_keeps_every_old_key_and_adds_the_chained_restatements_scores(dev, monkeypatch):
    """The F0 tracks and the path each batch hands to the wavelet kernels are recorded on the way; the restatement's whole chain on
    them is the reference, and the bar of a key is 16 times the distance between that chain in fp64 and in longdouble."""
    pairs = _pairs()
    stft = _stft(config("/nowhere"))
    refs, syns = [p[0] for p in pairs], [p[1] for p in pairs]
    plain = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev)
    rows = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, wavelet=True)
    seen = {"f0": [], "path": []}
    measure, on_path = C.measure, C.on_path

    def spy_measure(f0, lens, *rate):
        seen["f0"].append([f0[b, :T].cpu().numpy() for b, T in enumerate(lens)])
        return measure(f0, lens, *rate)

    def spy_on_path(pi, pj, plen, *rest):
        seen["path"].append([(pi[b, :int(P)].cpu().numpy(), pj[b, :int(P)].cpu().numpy()) for b, P in enumerate(plen.cpu())])
        return on_path(pi, pj, plen, *rest)

    monkeypatch.setattr(C, "measure", spy_measure)
    monkeypatch.setattr(C, "on_path", spy_on_path)
    again = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, wavelet=True, budget=1)       # one pair per batch
    assert json.dumps(rows) == json.dumps(again) and len(seen["path"]) == 4 and len(seen["f0"]) == 8
    new = set(ref.KEYS)
    for r, p in zip(rows, plain):
        assert set(r) == set(p) | new and json.dumps({k: v for k, v in r.items() if k not in new}) == json.dumps(p)
    order = sorted(range(4), key=lambda i: (-rows[i]["frames_ref"], -rows[i]["frames_syn"], i))     # longest first: the batches' order
    want, exact = [None] * 4, [None] * 4
    for n, i in enumerate(order):
        f0a, f0b, (pi, pj) = seen["f0"][2 * n][0], seen["f0"][2 * n + 1][0], seen["path"][n][0]
        assert len(f0a) == rows[i]["frames_ref"] and len(f0b) == rows[i]["frames_syn"] and len(pi) == rows[i]["path_len"]
        want[i] = ref.row_scores(f0a, f0b, pi, pj, S.FS, S.HOP)
        exact[i] = ref.row_scores(f0a, f0b, pi, pj, S.FS, S.HOP, LD)
    for key in ref.KEYS:
        got, w, e = (np.array([np.asarray(r[key], np.float64) for r in src]) for src in (rows, want, exact))
        assert np.array_equal(np.isnan(got), np.isnan(w)), key
        ok = ~np.isnan(w)
        limit = 16 * float(np.abs(w.astype(LD) - np.array([np.asarray(r[key], LD) for r in exact]))[ok].max())
        worst = float(np.abs(got - w)[ok].max())
        print(f"{key}: largest distance {worst:.2e}, bar {limit:.2e}")
        assert worst <= limit, key
    assert rows[0]["cwt_rmse"] == [0.0] * 10 and max(rows[2]["cwt_rmse"]) > 0 and np.isfinite(rows[1]["cwt_corr"]).all()
    summary = M.summarize(rows)
    assert summary["wavelet_flat_utterances"] == 0 and len(summary["cwt_corr_weighted"]) == 10 and summary["cwt_scales_ms"][0] == 20
    assert "cwt_corr_mean" not in M.summarize(plain)
    with pytest.raises(ValueError):
        M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, f0=False, wavelet=True)


def test_score_wavelet_end_to_end(dev, tmp_path, capsys):
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
            "--out", os.path.join(root, "s.jsonl")]
    plain, _, summary0 = score.main(argv)
    capsys.readouterr()
    rows, skipped, summary = score.main(argv + ["--wavelet"])
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    new = {"cwt_scales_ms", "cwt_power_ratio_db_by_scale", "wavelet_flat_utterances"} | {
        k + s for k in ("cwt_corr", "cwt_rmse", "cwt_level_corr", "cwt_level_rmse") for s in ("_mean", "_weighted", "_nan_utterances")}
    assert not skipped and set(summary) == set(summary0) | new and not new & set(summary0) and set(said) == set(summary)
    assert {k: summary[k] for k in summary0} == summary0 and "cwt_corr" not in plain[0] and set(ref.KEYS) <= set(rows[0])
    assert summary["cwt_scales_ms"] == C.scales_ms() and summary["wavelet_flat_utterances"] == 0
    assert summary["cwt_rmse_mean"] == pytest.approx(np.mean([r["cwt_rmse"] for r in rows], axis=0), abs=1e-12)
    written = [json.loads(line) for line in open(os.path.join(root, "s.jsonl"))]
    assert [r["basename"] for r in written] == ["u0", "u1", "u2"] and written[0]["cwt_corr"] == rows[0]["cwt_corr"]
    with pytest.raises(SystemExit):
        score.main(argv + ["--wavelet", "--no_f0"])
