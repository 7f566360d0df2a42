"""Each kernel of csrc/fs2_f0.hip alone against fp64, on the inputs of tests/f0_stage_cases.py (whose exactness and conditions
tests/test_f0_stages_cpu.py shows without a GPU).  Every batch is ragged with a row of length 0, every input is poisoned beyond a
row's extent (NaN, or a sentinel for integers), every output is filled with a sentinel first and must keep it outside the row's
extent, and every leading dimension is larger than it has to be.

    entry point          called directly by
    fs2_f0_dc            test_dc, test_lowcut_real
    fs2_f0_lowcut        test_lowcut_exact, test_lowcut_real, test_lowcut_refuses_oversized_taps
    fs2_f0_events        test_events
    fs2_f0_scan          test_events, test_scan
    fs2_f0_candidates    test_candidates_exact, test_candidates_real
    fs2_f0_fix           test_fix
    fs2_f0_stonemask     test_stonemask
    (pitch.dio / pitch.stonemask at 16 kHz, 48 kHz and with other band settings: test_chain_other_rates_and_settings)
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib, ops, pitch
from tests import f0_ref as R
from tests import f0_stage_cases as C
from tests.f0_signals import FRAME_PERIOD, FS, tone
from tests.test_f0_gpu import RTOL, _agree, _batch

pytestmark = pytest.mark.gpu
SENT, ISENT = -7777.25, -77777                   # what every output holds before a call
NAN = float("nan")


def _rows(rows, ld, fill, dtype, dev, extra=0):
    """(len(rows) + extra, ld) device tensor holding `fill`, row b starting with rows[b]"""
    a = np.full((len(rows) + extra, ld), fill, dtype=dtype)
    for b, r in enumerate(rows):
        a[b, :len(r)] = r
    return torch.from_numpy(a).to(dev)


def _vec(v, fill, dtype, dev, extra=3):
    """v followed by `extra` poisoned entries"""
    return torch.from_numpy(np.concatenate([np.asarray(v, dtype), np.full(extra, fill, dtype)])).to(dev)


def _kept(a, fill=SENT):
    return a.size == 0 or bool(np.all(a == fill))


def _dc(rows, dev):
    B, Nmax = len(rows), max(len(r) for r in rows)
    ldx = Nmax + 7
    x = _rows(rows, ldx, NAN, np.float32, dev)
    lens = _vec([len(r) for r in rows], 1 << 30, np.int32, dev)
    stats = torch.full((B + 1, 2), SENT, dtype=torch.float64, device=dev)
    _lib.call("fs2_f0_dc", x.data_ptr(), ldx, lens.data_ptr(), stats.data_ptr(), B, Nmax, ops._stream())
    return x, ldx, lens, stats, B, Nmax


def test_dc(dev):
    rows = C.dc_rows()
    _, _, _, stats, B, _ = _dc(rows, dev)
    got = stats.cpu().numpy()
    assert _kept(got[B])
    worst_m = worst_t = 0.0
    for b, x in enumerate(rows):
        mean, bound, tau = C.dc_ref(x)
        dm = abs(got[b, 0] - mean)
        tb = C.dc_tau_bound(tau, dm)
        dt = abs(Fraction(got[b, 1]) - tau)
        print("dc row", b, "N", len(x), "|dmean|", dm, "bound", bound, "|dtau|", float(dt), "bound", float(tb))
        assert dm <= bound and dt <= tb, (b, dm, bound, float(dt), float(tb))
        worst_m, worst_t = max(worst_m, dm / bound if bound else 0.0), max(worst_t, float(dt / tb) if tb else 0.0)
    print("dc: largest |dmean| / bound", worst_m, "largest |dtau| / bound", worst_t)
    assert got[0, 0] == 0 and got[0, 1] == 0 and got[8, 0] == 0 and got[8, 1] == 0


def _lowcut(x, ldx, lens, stats, taps, Rr, H, B, Nmax, dev):
    ldl = Nmax + 2 * H + 1 + 5
    lc = torch.full((B + 1, ldl), SENT, dtype=torch.float64, device=dev)
    g = _vec(taps, NAN, np.float64, dev)
    _lib.call("fs2_f0_lowcut", x.data_ptr(), ldx, lens.data_ptr(), stats.data_ptr(), g.data_ptr(), Rr, lc.data_ptr(), ldl, H, B, Nmax,
              ops._stream())
    return lc.cpu().numpy()


@pytest.mark.parametrize("Rr,H", [(3, 4), (5, 12)])
def test_lowcut_exact(dev, Rr, H):
    """integers, dyadic means and taps: lc equals np.convolve as numbers, element for element (-0 counts as 0)"""
    rows, means, taps = C.lowcut_exact_case(Rr, H, 20 + Rr)
    B, Nmax = len(rows), max(len(r) for r in rows)
    ldx = Nmax + 7
    x = _rows(rows, ldx, NAN, np.float32, dev)
    lens = _vec([len(r) for r in rows], 1 << 30, np.int32, dev)
    stats = torch.from_numpy(np.stack([means, np.full(B, NAN)], axis=1)).to(dev)
    got = _lowcut(x, ldx, lens, stats, taps, Rr, H, B, Nmax, dev)
    assert _kept(got[B])
    for b, r in enumerate(rows):
        n = len(r) + 2 * H + 1
        want = C.lowcut_ref(r, means[b], taps, H)
        assert np.array_equal(got[b, :n], want), (b, len(r), np.nonzero(got[b, :n] != want)[0][:8])
        assert _kept(got[b, n:]), (b, len(r))


@pytest.mark.parametrize("fs", [16000, 22050, 48000])
def test_lowcut_real(dev, fs):
    """the preprocessor's own taps (R = 320, 441, 960) on noise, against the direct fp64 sum with the error bound of a sum of
    2R + 2 terms in any order, plus what the DC kernel's own mean moves the result by"""
    rows = C.lowcut_real_rows()
    taps = pitch.lowcut_taps(fs)
    Rr, H = (len(taps) - 1) // 2, C.rate_half_width(fs)
    x, ldx, lens, stats, B, Nmax = _dc(rows, dev)
    means = stats.cpu().numpy()[:, 0]
    got = _lowcut(x, ldx, lens, stats, taps, Rr, H, B, Nmax, dev)
    assert _kept(got[B])
    worst = 0.0
    for b, r in enumerate(rows):
        n = len(r) + 2 * H + 1
        mean, mbound, _ = C.dc_ref(r)
        assert abs(means[b] - mean) <= mbound
        want, mag, gs = C.lowcut_real_ref(r, mean, taps, H)
        bound = (2 * Rr + 2) * C.U * mag + abs(means[b] - mean) * gs
        err = np.abs(got[b, :n] - want)
        assert np.all(err <= bound), (fs, b, float((err - bound).max()))
        assert _kept(got[b, n:]), (fs, b)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if len(r) else 0.0)
    print("lowcut fs", fs, "R", Rr, "H", H, "largest err / bound", worst)


def test_lowcut_refuses_oversized_taps(dev):
    Rr = 1984                                                          # (4R + 1 + 256) * 8 = 65544 bytes of LDS
    x = torch.zeros(1, 64, dtype=torch.float32, device=dev)
    lens = torch.tensor([64], dtype=torch.int32, device=dev)
    stats = torch.zeros(1, 2, dtype=torch.float64, device=dev)
    taps = torch.zeros(2 * Rr + 1, dtype=torch.float64, device=dev)
    lc = torch.full((1, 64 + 2 * 4 + 1), SENT, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        _lib.call("fs2_f0_lowcut", x.data_ptr(), 64, lens.data_ptr(), stats.data_ptr(), taps.data_ptr(), Rr, lc.data_ptr(), lc.shape[1], 4,
                  1, 64, ops._stream())
    assert _kept(lc.cpu().numpy())


@pytest.mark.parametrize("H", [2 * max(C.BAND_H), 2 * max(C.BAND_H) + 3])
@pytest.mark.parametrize("kind", ["dense", "sparse", "tau", "seam"])
def test_events(dev, kind, H):
    """counting pass, scan and emitting pass as pitch.dio runs them, on exact inputs: counts per tile, offsets, totals and every
    event position equal the reference's bits"""
    rows, tk = C.event_rows(kind, H)
    taps = C.band_taps(tk)
    nb, max_h = len(taps), max(C.BAND_H)
    B, Nmax = len(rows), max(N for N, _, _ in rows)
    ldl, ntile, cap = Nmax + 2 * H + 1 + 3, -(-Nmax // 256), Nmax // 2 + 2 + 5
    lc = _rows([r for _, r, _ in rows], ldl, NAN, np.float64, dev)
    lens = _vec([N for N, _, _ in rows], 1 << 30, np.int32, dev)
    stats = torch.from_numpy(np.array([[NAN, tau] for _, _, tau in rows])).to(dev)
    nut = _vec(np.concatenate(taps), NAN, np.float64, dev)
    band_h = _vec(C.BAND_H, 1 << 20, np.int32, dev)
    counts = torch.full((B + 1, nb, 4, ntile), ISENT, dtype=torch.int32, device=dev)
    offs = torch.full_like(counts, ISENT)
    totals = torch.full((B + 1, nb, 4), ISENT, dtype=torch.int32, device=dev)
    events = torch.full((B + 1, nb, 4, cap), SENT, dtype=torch.float64, device=dev)
    st = ops._stream()
    for emit in (0, 1):
        _lib.call("fs2_f0_events", lc.data_ptr(), ldl, H, lens.data_ptr(), stats.data_ptr(), nut.data_ptr(), band_h.data_ptr(), nb, max_h,
                  counts.data_ptr(), offs.data_ptr(), events.data_ptr(), cap, B, Nmax, emit, st)
        if not emit:
            assert _kept(events.cpu().numpy())                         # the counting pass writes no event
            _lib.call("fs2_f0_scan", counts.data_ptr(), offs.data_ptr(), totals.data_ptr(), B, nb, Nmax, st)
    counts, offs, totals, events = (a.cpu().numpy() for a in (counts, offs, totals, events))
    assert _kept(counts[B], ISENT) and _kept(offs[B], ISENT) and _kept(totals[B], ISENT) and _kept(events[B])
    for b, (N, r, tau) in enumerate(rows):
        _, streams, wc, wo, wt = C.events_ref(r, N, H, taps, tau, -(-N // 256))
        k = wc.shape[2] if N else 0
        assert np.array_equal(counts[b, :, :, :k], wc[:, :, :k]) and np.all(counts[b, :, :, k:] == 0), (kind, N, b)
        assert np.array_equal(offs[b, :, :, :k], wo[:, :, :k]) and np.array_equal(totals[b], wt), (kind, N, b)
        assert np.all(offs[b, :, :, k:] == wt[:, :, None])
        for j in range(nb):
            for e in range(4):
                pos = streams[j][e][1]
                assert np.array_equal(events[b, j, e, :len(pos)], pos), (kind, N, b, j, e)
                assert _kept(events[b, j, e, len(pos):]), (kind, N, b, j, e)


def test_scan(dev):
    for B, nb, Nmax, c in C.scan_cases():
        n, ntile = c.shape
        counts = torch.from_numpy(np.concatenate([c, np.full((2, ntile), ISENT, np.int32)])).to(dev)
        offs = torch.full((n + 2, ntile), ISENT, dtype=torch.int32, device=dev)
        totals = torch.full((n + 2,), ISENT, dtype=torch.int32, device=dev)
        _lib.call("fs2_f0_scan", counts.data_ptr(), offs.data_ptr(), totals.data_ptr(), B, nb, Nmax, ops._stream())
        offs, totals = offs.cpu().numpy(), totals.cpu().numpy()
        cs = np.cumsum(c, axis=1)
        assert np.array_equal(offs[:n], cs - c) and np.array_equal(totals[:n], cs[:, -1]), (B, nb, Nmax)
        assert _kept(offs[n:], ISENT) and _kept(totals[n:], ISENT)


def _candidates(dev, lists, frames, Fmax, band_f0, fs, frame_period, f0_floor, f0_ceil):
    """lists[b][j] are the four event lists of band j of row b -> (cand, score), each (B, nb, Fmax)"""
    B, nb = len(lists), len(band_f0)
    cap = max([len(e) for row in lists for band in row for e in band] + [1]) + 4
    ev = np.full((B, nb, 4, cap), NAN)
    tot = np.zeros((B, nb, 4), np.int32)
    for b, row in enumerate(lists):
        for j, band in enumerate(row):
            for e, l in enumerate(band):
                ev[b, j, e, :len(l)], tot[b, j, e] = l, len(l)
    ev, tot = torch.from_numpy(ev).to(dev), torch.from_numpy(tot).to(dev)
    fr = _vec(frames, 1 << 30, np.int32, dev)
    bf = _vec(band_f0, NAN, np.float64, dev)
    cand = torch.full((B + 1, nb, Fmax), SENT, dtype=torch.float64, device=dev)
    score = torch.full_like(cand, SENT)
    _lib.call("fs2_f0_candidates", ev.data_ptr(), cap, tot.data_ptr(), fr.data_ptr(), bf.data_ptr(), nb, float(fs), float(frame_period),
              float(f0_floor), float(f0_ceil), cand.data_ptr(), score.data_ptr(), B, Fmax, ops._stream())
    cand, score = cand.cpu().numpy(), score.cpu().numpy()
    assert _kept(cand[B]) and _kept(score[B])
    return cand[:B], score[:B]


@pytest.mark.parametrize("Fmax", [1, 63, 64, 65, 130])
def test_candidates_exact(dev, Fmax):
    """fs = 1024, t_f = f / 16, events on integers and halves, four equal streams: candidates and scores equal the reference's
    bits at both inclusive ends of the location range, at the floor, at band_f0 and band_f0 / 2, and with 3 and 4 events"""
    rows = C.cand_exact_rows(Fmax)
    nb = len(C.CAND_BANDS)
    cand, score = _candidates(dev, [[[ev] * 4] * nb for ev, _ in rows], [f for _, f in rows], Fmax, C.CAND_BANDS, C.CAND_FS, C.CAND_PERIOD,
                              C.CAND_FLOOR, C.CAND_CEIL)
    for b, (ev, frames) in enumerate(rows):
        wc, ws = C.cand_expected(ev, frames, Fmax, C.CAND_FS, C.CAND_PERIOD, C.CAND_BANDS, C.CAND_FLOOR, C.CAND_CEIL)
        assert np.array_equal(cand[b], wc), (b, np.nonzero(cand[b] != wc))
        assert np.array_equal(score[b], ws), (b, np.nonzero(score[b] != ws))


@pytest.mark.parametrize("ki", [0, 1])
def test_candidates_real(dev, ki):
    """the oracle's event lists of a tone and a glide, default bands and floor 50 / ceil 400 / 4 channels per octave"""
    cases = [C.cand_real_case(si, ki) for si in (0, 1)]
    band_f0, floor, ceil = cases[0][0], cases[0][3], cases[0][4]
    nb, Fmax = len(band_f0), 40
    lists = [cases[0][1], cases[1][1], cases[0][1], [[np.zeros(0)] * 4] * nb]
    frames = [cases[0][2], cases[1][2], 10, Fmax]
    cand, score = _candidates(dev, lists, frames, Fmax, band_f0, FS, FRAME_PERIOD, floor, ceil)
    worst_c = worst_s = worst_a = 0.0
    for b in range(4):
        wc, ws = C.cand_expected(lists[b], frames[b], Fmax, FS, FRAME_PERIOD, band_f0, floor, ceil)
        assert np.array_equal(cand[b] > 0, wc > 0), (b, np.nonzero((cand[b] > 0) != (wc > 0)))
        v = wc > 0
        assert np.all(cand[b][~v] == 0) and np.all(score[b][~v] == C.REJECTED)
        if b < 3:
            assert v.sum() >= 10
        if not v.any():
            continue
        worst_c = max(worst_c, float(np.abs(cand[b][v] / wc[v] - 1).max()))
        well = v & (ws >= 1e-6)
        flat = v & (ws < 1e-6)                                         # the tone's period is 147 samples exactly: no spread at all
        if well.any():
            worst_s = max(worst_s, float(np.abs(score[b][well] / ws[well] - 1).max()))
        if flat.any():
            worst_a = max(worst_a, float(np.abs(score[b][flat] - ws[flat]).max()))
    print("candidates setting", ki, "largest rel err of a candidate", worst_c, "of a normalised score", worst_s, "bound", RTOL,
          "; largest abs err of a score without spread", worst_a, "bound", 16 * C.U)
    assert worst_c <= RTOL and worst_s <= 1e-6 and worst_a <= 16 * C.U


@pytest.mark.parametrize("B", [1, 64, 65])
@pytest.mark.parametrize("vrm", [3, 7])
def test_fix(dev, vrm, B):
    """integer candidates and dyadic scores: the fixed contour equals R.fix_contour's bits, the tail beyond a row's frames is 0"""
    rows = C.fix_case(vrm, B)
    nb, Fmax = rows[0][0].shape[0], 205
    cand = np.full((B, nb, Fmax), NAN)
    score = np.full((B, nb, Fmax), NAN)
    for b, (c, s) in enumerate(rows):
        cand[b, :, :c.shape[1]], score[b, :, :c.shape[1]] = c, s
    cand, score = torch.from_numpy(cand).to(dev), torch.from_numpy(score).to(dev)
    frames = _vec([c.shape[1] for c, _ in rows], 1 << 30, np.int32, dev)
    tmp = torch.full((B, 2, Fmax), SENT, dtype=torch.float64, device=dev)
    f0 = torch.full((B + 1, Fmax), SENT, dtype=torch.float64, device=dev)
    _lib.call("fs2_f0_fix", cand.data_ptr(), score.data_ptr(), frames.data_ptr(), nb, vrm, float(pitch.ALLOWED_RANGE), tmp.data_ptr(),
              f0.data_ptr(), B, Fmax, ops._stream())
    f0 = f0.cpu().numpy()
    assert _kept(f0[B])
    for b, (c, s) in enumerate(rows):
        F = c.shape[1]
        want = R.fix_contour(c, s, C.FIX_PERIODS[vrm])
        assert np.array_equal(f0[b, :F], want), (b, F, np.nonzero(f0[b, :F] != want)[0])
        assert np.all(f0[b, F:] == 0)


@pytest.mark.parametrize("fs", C.STONE_RATES)
def test_stonemask(dev, fs):
    """hand-made contours on tones of two lengths (and speech at 22050 Hz): frames 0 and last, true and 15 % off values, 40 and
    fs / 12 from both sides, 0, NaN, frames at or beyond frames[b], and a row of length 0 whose one frame holds a fine f0"""
    rows, _ = C.stone_case(fs)
    B, Nmax = len(rows), max(len(x) for x, _, _, _ in rows)
    ldx, Fmax = Nmax + 9, max(F for _, _, F, _ in rows) + 3
    x = _rows([r[0] for r in rows], ldx, NAN, np.float32, dev)
    lens = _vec([len(r[0]) for r in rows], 1 << 30, np.int32, dev)
    frames = _vec([r[2] for r in rows], 1 << 30, np.int32, dev)
    f0 = _rows([r[1] for r in rows], Fmax, 200.0, np.float64, dev)      # a fine value at and beyond frames[b]: still 0 there
    out = torch.full((B + 1, Fmax), SENT, dtype=torch.float64, device=dev)
    _lib.call("fs2_f0_stonemask", x.data_ptr(), ldx, lens.data_ptr(), f0.data_ptr(), frames.data_ptr(), float(fs), 256 / fs * 1000,
              out.data_ptr(), B, Fmax, Nmax, ops._stream())
    out = out.cpu().numpy()
    assert _kept(out[B])
    worst = 0.0
    for b, (_, _, F, want) in enumerate(rows):
        assert np.array_equal(out[b, :F] != 0, want != 0), (fs, b, np.nonzero((out[b, :F] != 0) != (want != 0))[0])
        assert np.all(out[b, F:] == 0)
        v = want != 0
        if v.any():
            worst = max(worst, float(np.abs(out[b, :F][v] / want[v] - 1).max()))
    print("stonemask fs", fs, "largest rel err", worst, "bound", RTOL)
    assert worst <= RTOL


@pytest.mark.parametrize("ci", range(len(C.CHAIN_CASES)))
def test_chain_other_rates_and_settings(dev, ci):
    """pitch.dio and pitch.stonemask against R.dio and R.stonemask on a ragged batch of tones with a row of length 0.  The 130 and
    310 Hz rows are held to the oracle's whole chain at every frame.  For the 120 and 300 Hz rows that will not do at 16 and
    48 kHz: 1.5 fs / f0 is an integer there, so StoneMask's window half-width int(1.5 fs / f0 + 1) turns on the last bit of a DIO
    value that is 120 or 300 up to rounding.  Those rows are compared in two steps, pitch.dio with R.dio and pitch.stonemask with
    R.stonemask of the contour pitch.dio returned, and with the whole chain where the oracle's contour leaves the truncation
    alone."""
    fs, kw = C.CHAIN_CASES[ci]
    fp = 256 / fs * 1000
    rows = C.chain_case(ci)
    y, lens = _batch([r[0] for r in rows], dev, poison=NAN)
    f0, t, frames = pitch.dio(y, lens, fs, fp, **kw)
    sm = pitch.stonemask(y, lens, f0, frames, fs, fp).cpu().numpy()
    f0 = f0.cpu().numpy()
    for b, (x, plain, want_sm, want_dio, tt) in enumerate(rows):
        F = frames[b]
        assert len(tt) == F and np.all(f0[b, F:] == 0) and np.all(sm[b, F:] == 0)
        _agree(f0[b, :F], want_dio, ("dio", fs, b))
        _agree(sm[b, :F], R.stonemask(x, f0[b, :F], tt, fs), ("stonemask of the dio contour", fs, b))
        firm = np.full(F, True) if plain else C.chain_firm(fs, want_dio)
        _agree(np.where(firm, sm[b, :F], 0.0), np.where(firm, want_sm, 0.0), ("dio+stonemask", fs, b))


def test_chain_refuses_a_ceiling_above_the_rate(dev):
    y, lens = _batch([tone(200, dur=0.1, fs=16000)], dev)
    with pytest.raises(ValueError, match="too high"):
        pitch.dio(y, lens, 16000, 16.0, f0_ceil=40000.0)
