"""The inputs of the F0 stage tests (tests/f0_stage_cases.py) on the references alone: the exact cases are exact, the builders hold
the features they claim, the restated stages equal tests/f0_ref.py, and no decision of a conditioned case sits near a threshold."""
from fractions import Fraction

import numpy as np
import pytest

from fastspeech2_amd import pitch
from tests import f0_ref as R
from tests import f0_stage_cases as C
from tests.f0_signals import FRAME_PERIOD, FS


def _dyadic(a, bits):
    a = np.asarray(a, np.float64)
    return np.all(a * 2.0 ** bits == np.round(a * 2.0 ** bits)) and np.all(np.abs(a) < 2.0 ** 20)


def test_dc_rows_and_reference():
    rows = C.dc_rows()
    assert [len(r) for r in rows[:7]] == [0, 1, 2, 255, 256, 257, 1000]
    for x in rows:
        mean, bound, tau = C.dc_ref(x)
        y = np.concatenate([x.astype(np.float64), [0.0]])
        assert abs(mean - y.sum() / len(y)) <= bound + 2.0 ** -53 * abs(mean)       # the oracle's own mean obeys the bound
        assert abs(float(tau) - 1e-9 * np.abs(y - mean).max()) <= 2 * C.U * float(tau)
    assert C.dc_ref(rows[0])[0] == 0 and C.dc_ref(rows[0])[2] == 0
    x = rows[7]
    mean, _, tau = C.dc_ref(x)
    assert np.all(x == x[0]) and tau == Fraction(1e-9) * abs(Fraction(mean))        # the appended zero alone sets tau
    assert C.dc_ref(rows[8])[0] == 0 and C.dc_ref(rows[8])[2] == 0


@pytest.mark.parametrize("Rr,H", [(3, 4), (5, 12)])
def test_lowcut_exact_inputs(Rr, H):
    rows, means, taps = C.lowcut_exact_case(Rr, H, 20 + Rr)
    assert sorted({len(r) + 2 * H + 1 for r in rows} & {255, 256, 257}) == [255, 256, 257]
    assert {0, 1} <= {len(r) for r in rows} and max(len(r) for r in rows) + 2 * H + 1 > 512
    assert _dyadic(taps, 3) and _dyadic(means, 3) and taps[0] != 0 and taps[-1] != 0
    for x, mean in zip(rows, means):
        assert _dyadic(x, 0) and np.abs(x).max(initial=0) <= 8
        N = len(x)
        lc = C.lowcut_ref(x, mean, taps, H)
        assert _dyadic(lc, 6)                                          # products of two k / 8: exact, whatever is fused
        m = np.arange(-H, N + H + 1)
        assert np.all(lc[(m < -Rr) | (m > N + Rr)] == 0)
        # the direct definition, element by element, in exact rational arithmetic
        y = {n: Fraction(float(x[n])) - Fraction(mean) for n in range(N)}
        y[N] = -Fraction(mean)
        for mm in (-H, -Rr, 0, N - 1, N, N + 1, N + Rr, N + H):
            want = sum(Fraction(taps[j + Rr]) * y.get(mm - j, 0) for j in range(-Rr, Rr + 1))
            assert Fraction(lc[mm + H]) == want, mm
        assert lc[N + Rr + H] == taps[-1] * -mean                      # the -mean sample reaches position N + R through the last tap


def test_lowcut_real_reference():
    for fs in (16000, 22050, 48000):
        g = pitch.lowcut_taps(fs)
        assert (len(g) - 1) // 2 == {16000: 320, 22050: 441, 48000: 960}[fs]
        assert (4 * ((len(g) - 1) // 2) + 1 + 256) * 8 <= 65536
    assert (4 * 1984 + 1 + 256) * 8 > 65536 >= (4 * 1983 + 1 + 256) * 8
    x = C.lowcut_real_rows()[0][:90]
    g = pitch.lowcut_taps(16000)[300:341]
    lc, mag, gs = C.lowcut_real_ref(x, 0.05, g, 7)
    y = np.concatenate([x.astype(np.float64) - 0.05, [0.05 * -1]])
    for m in (-7, 0, 45, 90, 97):
        terms = [g[j + 20] * y[m - j] for j in range(-20, 21) if 0 <= m - j <= 90]
        assert abs(lc[m + 7] - sum(terms)) <= 42 * C.U * sum(abs(v) for v in terms) + 1e-300
        assert abs(mag[m + 7] - sum(abs(v) for v in terms)) <= 1e-12 * mag[m + 7] + 1e-300
        assert abs(gs[m + 7] - sum(abs(g[j + 20]) for j in range(-20, 21) if 0 <= m - j <= 90)) <= 1e-12


@pytest.mark.parametrize("H", [6, 9])
@pytest.mark.parametrize("kind", ["dense", "sparse", "tau", "seam"])
def test_event_inputs(kind, H):
    rows, tk = C.event_rows(kind, H)
    taps = C.band_taps(tk)
    assert [len(v) for v in taps] == [4, 12, 8] and all(_dyadic(v, 3) for v in taps) and H >= 2 * max(C.BAND_H)
    assert sorted({N for N, _, _ in rows}) == sorted(C.EVENT_LENS + (0,))
    seen = {}
    for N, lc, tau in rows:
        assert len(lc) == N + 2 * H + 1 and _dyadic(lc, 0) and _dyadic([tau], 3)
        if N == 0:
            continue
        ntile = -(-N // 256)
        sig, streams, counts, offs, totals = C.events_ref(lc, N, H, taps, tau, ntile)
        for j, st in enumerate(sig):
            assert _dyadic(st, 3)                                      # every band sample is exact
            want = R.events(st)
            for e in range(4):
                i, pos = streams[j][e]
                assert np.array_equal(pos, want[e]) and np.all(np.diff(pos) > 0)
                assert len(pos) <= N // 2 + 2 and totals[j, e] == len(pos)
                assert np.all((e < 2) | (i < N - 1))
                for q in i:
                    seen.setdefault((N, j, e), set()).add(int(q))
            s = C.band_signal_ref(lc, N, H, taps[j])
            if kind == "dense":
                assert np.all(s[1:] * s[:-1] < 0) and np.all(np.abs(s) > tau)
                assert max(len(streams[j][0][0]), len(streams[j][1][0])) >= N // 2
            if kind == "sparse":
                seen.setdefault("zero", [0, 0, 0, 0])
                d = st[1:] - st[:-1]
                for e, u in enumerate((st, -st, d, -d)):
                    i = streams[j][e][0]
                    seen["zero"][e] += int(np.sum(u[i + 1] == 0))
            if kind == "tau":
                seen.setdefault("tau", [0, 0, 0])
                seen["tau"][0] += int(np.sum(np.abs(s) == tau))
                seen["tau"][1] += int(np.sum((np.abs(s) == tau) & (st == 0)))
                seen["tau"][2] += int(np.sum((np.abs(s) == 4) & (st != 0)))
            if kind in ("dense", "seam"):
                dl = st[N] - st[N - 1]
                seen.setdefault(("spur", N, j), set()).update({2} if dl > 0 and st[N] > 0 else {3} if dl < 0 and st[N] < 0 else set())
    if kind == "sparse":
        assert min(seen["zero"]) > 0, seen["zero"]                      # u[i + 1] == 0 ends an event in every stream
    if kind == "tau":
        assert seen["tau"][0] > 20 and seen["tau"][0] == seen["tau"][1] and seen["tau"][2] > 20
    if kind in ("dense", "seam"):
        for N in (257, 258, 513, 700):
            for j in range(3):
                for e in (0, 1):
                    assert {255, 256, N - 1} <= seen[(N, j, e)], (N, j, e)      # either polarity's row has it
                for e in (2, 3):
                    assert {255, min(256, N - 2), N - 2} <= seen[(N, j, e)] and N - 1 not in seen[(N, j, e)]
                assert seen[("spur", N, j)] == {2, 3}                  # d[N-1] would fire with s~[N+1] = 0, were i = N - 1 allowed


def test_scan_cases():
    cs = C.scan_cases()
    assert sorted({B * nb * 4 for B, nb, _, _ in cs}) == [4, 60, 64, 68]
    assert sorted({c.shape[1] for _, _, _, c in cs}) == [1, 3]


@pytest.mark.parametrize("Fmax", [1, 63, 64, 65, 130])
def test_candidate_exact_inputs(Fmax):
    rows = C.cand_exact_rows(Fmax)
    t = np.arange(Fmax) * C.CAND_PERIOD / 1000.0
    assert np.array_equal(t * 16, np.arange(Fmax))
    seen = set()
    for ev, frames in rows:
        assert _dyadic(ev, 1) and np.all(np.diff(ev) > 0)
        cand, score = C.cand_expected(ev, frames, Fmax, C.CAND_FS, C.CAND_PERIOD, C.CAND_BANDS, C.CAND_FLOOR, C.CAND_CEIL)
        assert _dyadic(cand, 10) and np.all((score == 0) | (score == C.REJECTED)) and np.all((score == 0) == (cand > 0))
        assert np.all(cand[:, frames:] == 0)
        if len(ev) == 3:
            assert np.all(cand == 0)
        if len(ev) == 4 and Fmax > 1:
            assert np.array_equal(cand[:, 1], [128.0, 0, 128.0, 0, 0]) and np.all(cand[:, 2:] == 0)
        if len(ev) > 4 and frames == Fmax:
            loc = (ev[:-1] + ev[1:]) / 2.0 / C.CAND_FS
            f0i = C.CAND_FS / np.diff(ev)
            assert t[1] == loc[0] and t[Fmax - 1] == loc[-1] and cand[0, 1] == 128 and cand[0, Fmax - 1] == 128
            k = np.clip(np.searchsorted(loc, t[1:], side="right"), 1, len(loc) - 1)
            assert C.CAND_FLOOR in f0i[k] and np.any(f0i[k] < C.CAND_FLOOR)          # a bracket at the floor, one below it
            seen |= set(cand[0][cand[0] > 0])
            # 128 == band_f0 is accepted, just above band_f0 or just below band_f0 / 2 it is not
            at = cand[0] == 128
            assert at.sum() >= 2 and np.all(cand[1][at] == 0) and np.all(cand[2][at] == 128) and np.all(cand[3][at] == 0)
            assert np.all(score[1][at] == C.REJECTED)
    if Fmax >= 63:
        assert {64.0, 80.0, 112.0, 128.0} <= seen


@pytest.mark.parametrize("si", [0, 1])
@pytest.mark.parametrize("ki", [0, 1])
def test_candidate_real_conditions(si, ki):
    band_f0, lists, frames, floor, ceil = C.cand_real_case(si, ki)
    assert len(band_f0) == (7, 13)[ki]
    t = np.arange(frames) * FRAME_PERIOD / 1000.0
    accepted = 0
    for b, ls in zip(band_f0, lists):
        edge, loc_d, floor_d, spread = C.cand_margins(ls, t, FS, b, floor, ceil)
        assert edge > 1e-6 and loc_d > 1e-9 and floor_d > 1e-6, (b, edge, loc_d, floor_d)
        c, s = R.band_candidates(ls, t, FS, b, floor, ceil)
        accepted += int(np.sum(c > 0))
        if si == 1:
            assert spread >= 1e-6, (b, spread)
        else:
            # the 150 Hz tone's period is 147 samples exactly, so its four streams agree to the last bits and no shift or cut
            # gives its scores a spread: they are either well conditioned or rounding residue, which the GPU test bounds
            # absolutely (four values each within a rounding of the oracle's have a spread within 16 roundings of its own)
            assert np.all((s[c > 0] >= 1e-6) | (s[c > 0] <= 16 * C.U)), (b, s[c > 0])
    assert accepted >= frames // 2


@pytest.mark.parametrize("vrm", [3, 7])
def test_fix_inputs(vrm):
    assert pitch.voice_range_minimum(C.FIX_PERIODS[vrm]) == vrm
    changed3 = changed4 = tb = ts = 0
    feats = set()
    for B in (1, 64, 65):
        rows = C.fix_case(vrm, B)
        assert len(rows) == B and {c.shape[1] for c, _ in rows} >= ({200} if B == 1 else {0, vrm, vrm + 1, 40, 200})
        for cand, score in rows:
            F = cand.shape[1]
            assert _dyadic(cand, 0) and np.all((cand == 0) | ((cand >= 72) & (cand <= 790))) and _dyadic(score, 5)
            f2, f3, f4, t_best, t_sel = C.fix_stages(cand, score, vrm)
            want = R.fix_contour(cand, score, C.FIX_PERIODS[vrm])
            assert np.array_equal(f4, want)
            assert _dyadic(want, 0)
            if F <= vrm + 1:
                assert np.all(want == 0)
                continue
            changed3 += int(np.any(f3 != f2))
            changed4 += int(np.any(f4 != f3))
            tb, ts = tb + t_best, ts + t_sel
            best = cand[np.argmin(score, axis=0), np.arange(F)]
            feats |= {"starts at vrm"} if best[vrm] != 0 and f4[vrm] != 0 else set()
            feats |= {"ends vrm before the end"} if best[F - vrm - 1] != 0 else set()
            inner = best[vrm:F - vrm]
            feats |= {"one frame apart"} if np.any((inner[1:-1] == 0) & (inner[:-2] != 0) & (inner[2:] != 0)) else set()
            feats |= {"extends past the best band"} if np.any((f3 != 0) & (best == 0)) else set()
            nz = (f3[1:] == 0) & (f3[:-1] != 0) & (f2[:-1] == 0)
            feats |= {"a jump stops an extension"} if np.any(nz & (np.abs(cand[:, 1:]).max(axis=0) > 0)) else set()
    assert changed3 >= 2 and changed4 >= 2 and tb >= 2 and ts >= 2, (changed3, changed4, tb, ts)
    assert feats == {"starts at vrm", "ends vrm before the end", "one frame apart", "extends past the best band",
                     "a jump stops an extension"}, feats


@pytest.mark.parametrize("fs", C.STONE_RATES)
def test_stonemask_conditions(fs):
    rows, share = C.stone_case(fs)
    assert len(rows) == (6 if fs == FS else 5) and share >= 0.9, share
    assert len({len(x) for x, _, _, _ in rows}) >= 3 and len({F for _, _, F, _ in rows}) >= 3        # ragged in lens and in frames
    fp = 256 / fs * 1000
    kinds = set()
    for x, f0, F, want in rows:
        if len(x) == 0:
            # a frame with a fine f0 on a row without samples: only the kernel's own length guard keeps it from reading x[-1]
            assert F == 1 and f0[0] == 200.0 and want[0] == 0 and C.stone_trace(x, fs, 0.0, 200.0)[0] == 0
            kinds.add("empty row")
            continue
        assert F == len(f0) == len(want) >= 8
        t = np.arange(F) * fp / 1000.0
        assert f0[0] > 40 and f0[-1] > 40 and want[0] > 0 and want[-1] > 0           # both clamping ends are refined frames
        for i in range(F):
            res, f1, f2, half = C.stone_trace(x, fs, t[i], f0[i])
            assert res == want[i] == R.stonemask_frame(x, fs, t[i], f0[i])
            assert f1 is None or C.stone_conditioned(f0[i], f1, f2, half)
            if f1 is not None and abs(res / f0[i] - 1) > 0.1:
                kinds.add("pulled back")
        kinds |= {"40" for v, w in zip(f0, want) if v == 40.0 and w == 0}
        kinds |= {"above 40" for v, w in zip(f0, want) if v == np.nextafter(40.0, np.inf) and w > 0}
        kinds |= {"fs/12" for v, w in zip(f0, want) if v == fs / 12.0 and w > 0}
        kinds |= {"above fs/12" for v, w in zip(f0, want) if v == np.nextafter(fs / 12.0, np.inf) and w == 0}
        kinds |= {"nan" for v, w in zip(f0, want) if np.isnan(v) and w == 0}
    assert kinds == {"pulled back", "40", "above 40", "fs/12", "above fs/12", "nan", "empty row"}, kinds


@pytest.mark.parametrize("ci", range(len(C.CHAIN_CASES)))
def test_chain_conditions(ci):
    """the rows that the GPU test compares with the oracle's whole chain at every frame: no voiced frame of the oracle's DIO
    contour has its StoneMask window on an integer edge, and no decision of its StoneMask sits near a threshold"""
    fs, _ = C.CHAIN_CASES[ci]
    rows = C.chain_case(ci)
    assert len({len(x) for x, _, _, _, _ in rows}) == 4 and min(len(x) for x, _, _, _, _ in rows) == 0
    on_edge = 0
    for x, plain, want_sm, want_dio, tt in rows:
        if len(x) == 0:
            assert len(tt) == 1 and want_dio[0] == 0 and want_sm[0] == 0
            continue
        assert np.mean(want_sm > 0) > 0.5
        firm = C.chain_firm(fs, want_dio)
        on_edge += int(np.sum((want_dio > 0) & ~firm))
        if plain:
            assert np.array_equal(firm, want_dio > 0)
            for i in np.nonzero(want_dio > 0)[0]:
                res, f1, f2, half = C.stone_trace(x, fs, tt[i], want_dio[i])
                assert res == want_sm[i] and C.stone_conditioned(want_dio[i], f1, f2, half), (ci, i, want_dio[i], f1, f2, half)
    assert on_edge > 0 or fs != 48000                                  # why the 120 and 300 Hz rows are compared in two steps


def test_chain_settings_are_new():
    assert pitch.matlab_round(16000 / 50.0) == 320 and pitch.matlab_round(48000 / 50.0) == 960
    assert len(pitch.bands(50.0, 400.0, 4.0)) == 13
    assert min(pitch.matlab_round(16000 / b / 2.0) for b in pitch.bands(71.0, 40000.0, 2.0)) < 1
