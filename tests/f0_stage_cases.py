"""Inputs and small plain-numpy references for the stage tests of the F0 kernels (tests/test_f0_stages_cpu.py checks the builders
and their conditions without a GPU, tests/test_f0_stages_gpu.py runs the kernels of csrc/fs2_f0.hip on them one at a time).

Every comparison is one of two kinds.  Exact: the inputs are small integers and dyadic fractions, so every product and sum of the
stage is exact in fp64 whatever the compiler fuses, and the kernel must return the reference's bits.  Conditioned: the inputs are
real-valued and the CPU test shows, on the reference alone, that no decision of the stage sits near its threshold.

What tests/f0_ref.py lacks is restated here as direct sums (no FFT): the DC statistics, the low-cut, the band signal, the events
with their sample indices, the fixing steps one by one and StoneMask's two passes."""
import math
from fractions import Fraction

import numpy as np

from fastspeech2_amd import pitch
from tests import f0_ref as R
from tests.f0_signals import FRAME_PERIOD, FS, glide, speech, tone

U = 2.0 ** -52                                   # one rounding (one unit in the last place, relative)
REJECTED = R.NO_SCORE / R.SAFE                   # normalised score of a frame without a candidate


# ---------------------------------------------------------------------------------------------- 1. DC
def dc_rows():
    rng = np.random.RandomState(11)
    rows = [(0.3 * rng.randn(n) + 0.2).astype(np.float32) for n in (0, 1, 2, 255, 256, 257, 1000)]
    rows.append(np.full(300, 0.75, np.float32))                       # constant: tau comes from the appended zero alone
    rows.append(np.zeros(500, np.float32))
    return rows


def dc_ref(x):
    """(mean by math.fsum over the N + 1 samples, its bound N 2^-52 sum|x| / (N + 1): the worst case of any summation order
    with both divisions' roundings, and tau exactly, as a Fraction, from that mean)"""
    v = [float(a) for a in x] + [0.0]
    N = len(x)
    mean = math.fsum(v) / (N + 1)
    bound = N * U * math.fsum(abs(a) for a in v) / (N + 1)
    tau = Fraction(1e-9) * max(abs(Fraction(a) - Fraction(mean)) for a in v)
    return mean, bound, tau


def dc_tau_bound(tau, dmean):
    """|tau_gpu - tau| <= 1e-9 |dmean| (the kernel's own mean moves every |x - mean| by that much) plus one rounding: the
    subtraction and the product by 1e-9 round once each, half a unit each"""
    return Fraction(1e-9) * Fraction(dmean) + Fraction(U) * (1 + Fraction(U)) * (tau + Fraction(1e-9) * Fraction(dmean))


# ---------------------------------------------------------------------------------------------- 2. low-cut
def lowcut_ref(x, mean, taps, H):
    """lc[m], m in [-H, N + H], as a direct sum (np.convolve never uses an FFT)"""
    x = np.asarray(x, np.float64)
    N, Rr = len(x), (len(taps) - 1) // 2
    y = np.empty(N + 1)
    y[:N] = x - mean
    y[N] = -mean
    full = np.convolve(y, np.asarray(taps, np.float64))               # full[q] is lc[q - R], q < N + 1 + 2R
    out = np.zeros(N + 2 * H + 1)
    m = np.arange(-H, N + H + 1)
    q = m + Rr
    ok = (q >= 0) & (q < len(full))
    out[ok] = full[q[ok]]
    return out


def lowcut_exact_case(Rr, H, seed):
    """small-integer rows, dyadic taps, dyadic means written into `stats` by hand; N + 2H + 1 lands on 255, 256, 257 and the third
    tile"""
    rng = np.random.RandomState(seed)
    edge = 255 - 2 * H - 1
    lens = (0, 1, edge, edge + 1, edge + 2, 600)
    rows = [rng.randint(-8, 9, n).astype(np.float32) for n in lens]
    means = rng.randint(-12, 13, len(lens)) / 8.0
    means[0] = 0.625                                                   # the empty row is its appended sample alone
    taps = rng.randint(-8, 9, 2 * Rr + 1) / 8.0
    taps[0], taps[-1] = 0.125, -0.375                                  # both ends of the tap array must count
    return rows, means, taps


def lowcut_real_rows():
    rng = np.random.RandomState(23)
    return [(0.25 * rng.randn(n) + 0.05).astype(np.float32) for n in (700, 0, 1500)]


def lowcut_real_ref(x, mean, taps, H):
    """(lc, sum_j |g_j| |y_{m-j}|, sum of |g_j| over the taps that meet the row: what an error of the mean is multiplied by)"""
    N = len(x)
    ya = np.abs(np.concatenate([np.asarray(x, np.float64) - mean, [-mean]]))
    return lowcut_ref(x, mean, taps, H), _abs_conv(ya, taps, H), _abs_conv(np.ones(N + 1), taps, H)


def _abs_conv(ya, taps, H):
    """sum_j |g_j| ya[m - j] for m in [-H, N + H], ya given on [0, N]"""
    N, Rr = len(ya) - 1, (len(taps) - 1) // 2
    full = np.convolve(ya, np.abs(taps))
    out = np.zeros(N + 2 * H + 1)
    q = np.arange(-H, N + H + 1) + Rr
    ok = (q >= 0) & (q < len(full))
    out[ok] = full[q[ok]]
    return out


def rate_half_width(fs):
    """H as pitch.dio chooses it for the default bands"""
    return 2 * max(pitch.matlab_round(fs / b / 2.0) for b in pitch.bands())


# ---------------------------------------------------------------------------------------------- 3. band signal and events
BAND_H = [1, 3, 2]
EVENT_LENS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 258, 513, 700)


def band_taps(kind, seed=5):
    """dyadic taps of 4h each.  "alt": (-1)^k c_k with c_k in {1/4, 1/2, 1}, so that lc = (-1)^m a_m (a_m >= 0) gives
    s[i] = (-1)^i sum_k c_k a_{i + 2h - k}: every term has one sign.  "gen": k / 8 in [-1, 1], both ends non-zero."""
    rng = np.random.RandomState(seed)
    out = []
    for h in BAND_H:
        if kind == "alt":
            v = (-1.0) ** np.arange(4 * h) * rng.choice([0.25, 0.5, 1.0], 4 * h)
            v[:3] = np.array([0.25, -0.5, 1.0])                        # every band has all three magnitudes
        else:
            v = rng.randint(-8, 9, 4 * h) / 8.0
            v[0], v[-1] = -0.375, 0.625
        out.append(v)
    return out


def band_signal_ref(lc, N, H, v):
    """s[i] = sum_k v[k] lc[i + 2h - k], i in [0, N], lc given on [-H, N + H]; a direct sum"""
    L = len(v)
    h = L // 4
    idx = H + np.arange(N + 1)[:, None] + 2 * h - np.arange(L)[None, :]
    return (np.asarray(lc, np.float64)[idx] * v[None, :]).sum(axis=1)


def events_indexed(st):
    """R.events with the sample index of every event kept: [(i, position)] for the four streams"""
    st = np.asarray(st, np.float64)
    d = st[1:] - st[:-1]
    out = []
    for u in (st, -st, d, -d):
        i = np.nonzero((u[:-1] > 0) & (u[1:] <= 0))[0]
        out.append((i, (i + 1) - u[i] / (u[i + 1] - u[i])))
    return out


def events_ref(lc, N, H, taps, tau, ntile):
    """per band: s~ and its four (indices, positions); counts (nb, 4, ntile), offsets, totals"""
    nb = len(taps)
    counts = np.zeros((nb, 4, max(ntile, 1)), np.int32)
    streams, sig = [], []
    for j, v in enumerate(taps):
        if N == 0:
            sig.append(np.zeros(1))
            streams.append([(np.zeros(0, np.int64), np.zeros(0))] * 4)
            continue
        s = band_signal_ref(lc, N, H, v)
        st = np.where(np.abs(s) > tau, s, 0.0)
        ev = events_indexed(st)
        for e, (i, _) in enumerate(ev):
            counts[j, e] += np.bincount(i // 256, minlength=max(ntile, 1)).astype(np.int32)
        sig.append(st)
        streams.append(ev)
    offs = np.cumsum(counts, axis=2) - counts
    return sig, streams, counts, offs.astype(np.int32), counts.sum(axis=2).astype(np.int32)


def event_rows(kind, H):
    """[(lc over [-H, N + H] as integers, tau)] and the taps' kind; rows of every length of EVENT_LENS and one of length 0"""
    rng = np.random.RandomState({"dense": 31, "sparse": 32, "tau": 33, "seam": 34}[kind] + H)
    rows = []
    for N in EVENT_LENS + (0,):
        W = N + 2 * H + 1
        m = np.arange(-H, N + H + 1)
        for pol in ((1.0, -1.0) if kind in ("dense", "seam") else (1.0,)):
            if kind == "dense":                                       # s alternates in sign every sample
                lc, tau = pol * (-1.0) ** (m % 2) * rng.randint(1, 9, W), (0.0, 0.125)[N % 2]
            elif kind == "sparse":                                    # seeded integers, runs of exact zeros longer than the taps
                lc = rng.randint(-8, 9, W).astype(np.float64)
                p = 0
                while p < W:
                    p += rng.randint(5, 40)
                    z = rng.randint(14, 40)
                    lc[p:p + z] = 0.0
                    p += z
                tau = 0.0
            elif kind == "tau":                                       # lone impulses: s = a v[k], so |s| takes 1/2 ... 8; tau = 2
                lc = np.zeros(W)
                p = rng.randint(0, 6)
                while p < W:
                    lc[p] = rng.choice([-8.0, -4.0, -2.0, 2.0, 4.0, 8.0])
                    p += rng.randint(1, 4) if rng.rand() < 0.3 else rng.randint(13, 30)
                tau = 2.0
            else:                                                     # alternating only next to the tile seam and the row's end
                on = ((m >= 240) & (m <= 275)) | (m >= N - 20)
                lc, tau = np.where(on, pol * (-1.0) ** (m % 2) * rng.randint(1, 9, W), 0.0), 0.0
            rows.append((N, lc, tau))
    return rows, ("gen" if kind == "sparse" else "alt")


def scan_cases():
    rng = np.random.RandomState(41)
    out = []
    for B, nb in ((1, 1), (5, 3), (4, 4), (17, 1)):                    # B nb 4 = 4, 60, 64, 68
        for Nmax in (256, 700):                                        # 1 and 3 tiles
            out.append((B, nb, Nmax, rng.randint(0, 130, (B * nb * 4, -(-Nmax // 256))).astype(np.int32)))
    return out


# ---------------------------------------------------------------------------------------------- 4. candidates
CAND_FS, CAND_PERIOD, CAND_FLOOR, CAND_CEIL = 1024.0, 62.5, 64.0, 256.0          # t_f = f / 16 s = 64 f samples, exactly
CAND_BANDS = np.array([128.0, np.nextafter(128.0, 0.0), 256.0, np.nextafter(256.0, np.inf), 100.0])
# events around frame time 64 f (offsets in samples) -> the value interpolated there.  Interval F0s are 1024 / 4, 8, 16 or 32 and
# the interpolation weight is 0, 1/4, 1/2, 9/16 or 1, so every value is a short dyadic number on both sides.
CAND_CELLS = {
    "c8": ((-8, 0, 8), 128.0), "c16": ((-16, 0, 16), 64.0), "c4": ((-4, 0, 4), 256.0), "down": ((-7, 1, 17), 112.0),
    "up": ((-11, 5, 13), 80.0), "half": ((-8.5, -0.5, 7.5), 128.0), "at_loc": ((-4, 4, 12), 128.0), "low": ((-8, 0, 32), None),
}


def cand_exact_rows(Fmax):
    """[(four equal event lists, frames)] for fs = 1024, frame_period = 62.5"""
    rng = np.random.RandomState(50 + Fmax)
    kinds = sorted(CAND_CELLS)
    ev = []
    for f in range(1, Fmax):
        k = kinds[(f - 1) % len(kinds)] if f <= len(kinds) else kinds[rng.randint(len(kinds))]
        if f == 1:
            k = "at_loc"                                               # t_1 is the first location of the row
        off = CAND_CELLS[k][0]
        if f == Fmax - 1 and f > 1:
            off = (-12, -4, 4)                                         # t is the last location
        ev += [64.0 * f + o for o in off]
    full = np.array(ev)
    rows = [(full, Fmax), (full, Fmax // 2), (np.zeros(0), Fmax), (np.array([56.0, 64.0, 72.0]), Fmax),
            (np.array([56.0, 64.0, 72.0, 80.0]), Fmax), (full, 0)]
    return rows


def cand_expected(ev4, frames, Fmax, fs, frame_period, band_f0, f0_floor, f0_ceil):
    """(cand, normalised score), each (nb, Fmax), by R.band_candidates; frames at or beyond `frames` hold no candidate"""
    t = np.arange(frames) * frame_period / 1000.0
    cand = np.zeros((len(band_f0), Fmax))
    score = np.full((len(band_f0), Fmax), REJECTED)
    for j, b in enumerate(band_f0):
        lists = ev4[j] if isinstance(ev4, list) else [ev4] * 4
        c, s = R.band_candidates(lists, t, fs, b, f0_floor, f0_ceil)
        cand[j, :frames], score[j, :frames] = c, s
    return cand, score


REAL_SETTINGS = (dict(), dict(f0_floor=50.0, f0_ceil=400.0, channels_in_octave=4.0))


def cand_real_signals():
    return [tone(150)[:6000], glide()[0][:9000]]


_real = {}


def cand_real_case(si, ki):
    """event lists of signal si under settings ki by the oracle: (band_f0, [four lists per band], frames, f0_floor, f0_ceil)"""
    if (si, ki) not in _real:
        x, kw = cand_real_signals()[si], REAL_SETTINGS[ki]
        sig, _ = R.band_signals(x, FS, **kw)
        _real[si, ki] = (np.array([b for b, _ in sig]), [R.events(st) for _, st in sig], pitch.frame_count(len(x), FS, FRAME_PERIOD),
                         kw.get("f0_floor", pitch.F0_FLOOR), kw.get("f0_ceil", pitch.F0_CEIL))
    return _real[si, ki]


def cand_margins(lists, t, fs, b, f0_floor, f0_ceil):
    """how far the oracle's decisions for one band are from their thresholds: smallest relative distance of an accepted candidate
    from b, b / 2, floor, ceil; smallest |t_f - first or last location| in seconds; smallest relative distance of a bracketing
    F0 from the floor; smallest normalised spread of an accepted candidate"""
    c, s = R.band_candidates(lists, t, fs, b, f0_floor, f0_ceil)
    edge = loc_d = floor_d = np.inf
    if all(len(e) >= 4 for e in lists):
        ok, vals = np.ones(len(t), dtype=bool), []
        for e in lists:
            n = len(e) - 1
            loc = (e[:-1] + e[1:]) / 2.0 / fs
            f0i = fs / (e[1:] - e[:-1])
            loc_d = min(loc_d, np.abs(t - loc[0]).min(), np.abs(t - loc[-1]).min())
            k = np.clip(np.searchsorted(loc, t, side="right"), 1, n - 1)
            inside = (t >= loc[0]) & (t <= loc[-1])
            if inside.any():
                floor_d = min(floor_d, np.abs(f0i[k - 1][inside] / f0_floor - 1).min(), np.abs(f0i[k][inside] / f0_floor - 1).min())
            ok &= inside & (f0i[k - 1] >= f0_floor) & (f0i[k] >= f0_floor)
            vals.append(f0i[k - 1] + (t - loc[k - 1]) / (loc[k] - loc[k - 1]) * (f0i[k] - f0i[k - 1]))
        v = ((vals[0] + vals[1] + vals[2] + vals[3]) / 4.0)[ok]        # the value before the band test
        if len(v):
            edge = min(np.abs(v / th - 1).min() for th in (b, b / 2.0, f0_floor, f0_ceil))
    spread = s[c > 0].min() if (c > 0).any() else np.inf
    return edge, loc_d, floor_d, spread


# ---------------------------------------------------------------------------------------------- 5. fixing
FIX_PERIODS = {3: 14.0, 7: 4.7}                  # pitch.voice_range_minimum gives 3 and 7 at the default floor


def fix_row(F, vrm, rng, nb=4):
    """integer candidates (0 or [72, 790]) and dyadic scores of one row: voiced runs that drift slowly, with constant ends, jumps
    inside, equal best scores in two bands, and after a run frames whose best band is unvoiced while another band carries on
    (first two candidates equally far from the extrapolation)"""
    cand = np.zeros((nb, F))
    score = np.full((nb, F), 8.0)
    if F <= vrm + 1:
        cand[:] = rng.randint(72, 791, (nb, F))
        score[:] = rng.choice([0.0625, 0.25], (nb, F))
        return cand, score
    c = (vrm - 1) // 2
    pos = vrm if rng.rand() < 0.6 else vrm + rng.randint(1, 4)
    while pos < F - vrm:
        end = pos + 2 * c + 6 + rng.randint(0, 12)
        if end > F - vrm - (2 * c + 6):
            end = F - vrm                                              # the last run ends vrm frames before the end
        v = int(rng.randint(110, 560))
        jump = pos + c + 3 + rng.randint(0, 3) if (end - pos > 4 * c + 12 and rng.rand() < 0.5) else -1
        for i in range(pos, end):
            if i == jump:
                v = int(v * 1.3)
            elif c + 2 <= i - pos < end - pos - (c + 2):
                v += int(rng.randint(-3, 4))
            j = int(rng.randint(nb))
            for jj in range(nb):
                cand[jj, i] = min(max(v + int(rng.choice([-60, 45, 90, 150])), 72), 790)
                score[jj, i] = float(rng.choice([0.25, 0.5]))
            cand[j, i], score[j, i] = v, 0.0625
            if j + 1 < nb and rng.rand() < 0.3:                        # a later band ties the best score: the first wins
                cand[j + 1, i], score[j + 1, i] = min(v + 40, 790), 0.0625
        gap = 1 if rng.rand() < 0.3 else int(rng.randint(2 * c + 2, 2 * c + 9))
        nxt = end + gap
        ext = min(int(rng.randint(0, 5)), gap - 1, F - 1 - end) if gap > 1 else 0
        sgn = int(rng.choice([-1, 1]))
        val = [v + 2 * sgn, v + 3 * sgn, v + 4 * sgn, v + 4 * sgn][:max(ext, 0)]
        for q, i in enumerate(range(end, end + max(ext, 0))):
            cand[:, i], score[:, i] = 0.0, 8.0
            score[0, i] = 0.03125                                      # the best band is unvoiced here
            j = 1 + int(rng.randint(nb - 2))
            cand[j, i], score[j, i] = val[q], 0.5
            if q == 0:
                cand[j + 1, i], score[j + 1, i] = v - 2 * sgn, 0.5     # as far from the extrapolation v as band j: j wins
        pos = nxt
    return cand, score


def fix_case(vrm, B):
    """[(cand (nb, F), score (nb, F))] for B rows; F cycles through vrm, vrm + 1, 40, 200 and 0"""
    rng = np.random.RandomState(60 + 10 * vrm + B)
    Fs = [200, 40, vrm, vrm + 1, 0, 40, 200, 40]
    return [fix_row(Fs[b % len(Fs)] if B > 1 else 200, vrm, rng) for b in range(B)]


def fix_stages(cands, scores, vrm, allowed=pitch.ALLOWED_RANGE):
    """the docstring's steps one by one: (f2, f3, f4, ties of the best score, ties of the distance to the extrapolation between two
    distinct non-zero candidates)"""
    nb, F = cands.shape
    if F <= vrm:
        z = np.zeros(F)
        return z, z, z, 0, 0
    ties_best = ties_sel = 0
    best = np.zeros(F)
    for i in range(F):
        j = int(np.argmin(scores[:, i]))
        ties_best += int(vrm <= i < F - vrm and np.sum(scores[:, i] == scores[j, i]) > 1)
        best[i] = cands[j, i]
    base = best.copy()
    base[:vrm] = 0.0
    base[F - vrm:] = 0.0
    f1 = np.zeros(F)
    for i in range(vrm, F):
        f1[i] = base[i] if abs((base[i] - base[i - 1]) / (R.SAFE + base[i])) < allowed else 0.0
    c = (vrm - 1) // 2
    f2 = f1.copy()
    for i in range(c, F - c):
        if np.any(f1[i - c:i + c + 1] == 0):
            f2[i] = 0.0

    def select(cur, past, i):
        nonlocal ties_sel
        r = (3.0 * cur - past) / 2.0
        err = np.abs(r - cands[:, i])
        j = int(np.argmin(err))
        tied = cands[err == err[j], i]
        ties_sel += int(len(set(tied[tied != 0])) > 1)                 # two distinct candidates, not a frame of zeros
        return 0.0 if abs(1.0 - cands[j, i] / r) > allowed else cands[j, i]

    ends = [i - 1 for i in range(1, F) if f2[i] == 0 and f2[i - 1] != 0]
    starts = [i for i in range(1, F) if f2[i - 1] == 0 and f2[i] != 0]
    f3 = f2.copy()
    for q, e in enumerate(ends):
        for j in range(e, ends[q + 1] if q + 1 < len(ends) else F - 1):
            f3[j + 1] = select(f3[j], f3[j - 1], j + 1)
            if f3[j + 1] == 0:
                break
    f4 = f3.copy()
    for q in range(len(starts) - 1, -1, -1):
        for j in range(starts[q], starts[q - 1] if q > 0 else 1, -1):
            f4[j - 1] = select(f4[j], f4[j + 1], j - 1)
            if f4[j - 1] == 0:
                break
    return f2, f3, f4, ties_best, ties_sel


# ---------------------------------------------------------------------------------------------- 6. StoneMask
STONE_RATES = (16000, 22050, 48000)


def stone_rows(fs):
    """(signal, its F0): the three tones of 0.15 s, speech at 22050 Hz, a shorter tone (so that lens and frames differ within
    the batch at every rate and poison follows a row's own last sample) and a row of length 0, which still has one frame"""
    rows = [(tone(f, dur=0.15, fs=fs), float(f)) for f in (80, 200, 600)]
    if fs == FS:
        rows.append((speech()[0][:int(0.2 * FS)], 210.0))
    rows.append((tone(130, dur=0.12, fs=fs), 130.0))
    rows.append((np.zeros(0, np.float32), 200.0))
    return rows


def stone_contour(fs, true, F, row):
    """hand-made f0 per frame: the true F0, 15 % off either way, and the values next to the kernel's input thresholds (which of
    them a short row holds turns with the row's number)"""
    if F == 1:
        return np.array([true])                                        # the empty row: a fine value, and no sample to read
    vals = [40.0, np.nextafter(40.0, np.inf), true * 1.15, fs / 12.0, np.nextafter(fs / 12.0, np.inf), true * 0.85, 0.0, float("nan"), true]
    f0 = np.array([vals[(i + 3 * row) % len(vals)] for i in range(F)])
    f0[0], f0[-1] = true, true * 1.15                                  # both ends clamp their sample indices
    f0[1], f0[-2] = true * 0.85, true
    return f0


def stone_trace(x, fs, t, f0):
    """R.stonemask_frame with its two passes kept: (result, f', f'', smallest distance of a harmonic's bin position from a half)"""
    N = len(x)
    if not f0 > 40.0 or f0 > fs / 12.0 or N == 0:
        return 0.0, None, None, None
    hw = int(1.5 * fs / f0 + 1.0)
    n = np.arange(2 * hw + 1)
    r = np.array([pitch.matlab_round(v) for v in (t + (n - hw) / fs) * fs])
    xs = np.asarray(x, dtype=np.float64)[np.clip(r - 1, 0, N - 1)]
    wl = (2.0 * hw + 1.0) / fs
    tm = (r - 1.0) / fs - t
    w = 0.42 + 0.5 * np.cos(2.0 * np.pi * tm / wl) + 0.08 * np.cos(4.0 * np.pi * tm / wl)
    dw = np.empty_like(w)
    dw[0], dw[-1] = -w[1] / 2.0, w[-2] / 2.0
    dw[1:-1] = -(w[2:] - w[:-2]) / 2.0
    L = 4 * 2 ** int(np.floor(np.log2(2 * hw + 1)))
    M, D = np.fft.fft(xs * w, L), np.fft.fft(xs * dw, L)
    f1 = R._if(M, D, L, fs, f0, 2)
    half = min(abs((f0 * L / fs * h) % 1.0 - 0.5) for h in (1, 2))
    f2 = 0.0
    if not (f1 <= 0.0 or f1 > f0 * 2):
        f2 = R._if(M, D, L, fs, f1, 6)
        half = min([half] + [abs((f1 * L / fs * h) % 1.0 - 0.5) for h in range(1, 7)])
    return (f0 if abs(f2 - f0) > f0 * 0.2 else f2), f1, f2, half


def stone_conditioned(f0, f1, f2, half):
    """no decision of the frame near its threshold: f' away from 0 and 2 f0, |f'' - f0| away from 0.2 f0, and (not in the
    kernel's list of thresholds, but a rounding of a bin index all the same) no harmonic within 1e-6 of half a bin"""
    return abs(f1) > 1e-3 * f0 and abs(f1 - 2 * f0) > 1e-3 * f0 and abs(abs(f2 - f0) - 0.2 * f0) > 1e-3 * f0 and half > 1e-6


_stone = {}


def stone_case(fs):
    """[(x, f0 in, frames, expected out)] of one rate; frames that miss a condition get f0 = 0 (their share is returned too)"""
    if fs not in _stone:
        fp = 256 / fs * 1000
        out, kept, total = [], 0, 0
        for row, (x, true) in enumerate(stone_rows(fs)):
            F = pitch.frame_count(len(x), fs, fp)
            t = np.arange(F) * fp / 1000.0
            f0 = stone_contour(fs, true, F, row)
            for i in range(F):
                res, f1, f2, half = stone_trace(x, fs, t[i], f0[i])
                if f1 is not None:
                    total += 1
                    if stone_conditioned(f0[i], f1, f2, half):
                        kept += 1
                    else:
                        f0[i] = 0.0
            out.append((x, f0, F, R.stonemask(x, f0, t, fs)))
        _stone[fs] = (out, kept / max(total, 1))
    return _stone[fs]


# ---------------------------------------------------------------------------------------------- 7. the chain
CHAIN_CASES = ((16000, {}), (48000, {}), (FS, dict(f0_floor=50.0, f0_ceil=400.0, channels_in_octave=4.0)))
_chain = {}


def chain_case(ci):
    """[(x, plain, StoneMask of the oracle's DIO contour, that contour, frame times)] of CHAIN_CASES[ci].  At 16 and 48 kHz
    1.5 fs / f0 is an integer for the 120 and 300 Hz tones, so StoneMask's window half-width int(1.5 fs / f0 + 1) turns on the last
    bit of DIO's value there; the 130 and 310 Hz tones sit on no such edge (`plain`: the CPU test shows it), and with the row of
    length 0 they make the batch ragged."""
    if ci not in _chain:
        fs, kw = CHAIN_CASES[ci]
        xs = [(tone(120, dur=0.4, fs=fs), False), (tone(130, dur=0.3, fs=fs), True), (np.zeros(0, np.float32), True),
              (tone(300, dur=0.4, fs=fs), False), (tone(310, dur=0.35, fs=fs), True)]
        _chain[ci] = [(x, plain) + R.dio_stonemask(x, fs, 256 / fs * 1000, **kw) for x, plain in xs]
    return _chain[ci]


def chain_firm(fs, f0):
    """frames of a DIO contour whose StoneMask window half-width no rounding of the contour can change"""
    hw = 1.5 * fs / np.where(f0 > 0, f0, 1.0) + 1.0
    return (f0 > 0) & (np.abs(hw - np.round(hw)) > 1e-6)
