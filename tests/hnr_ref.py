"""An independent numpy restatement of the harmonics-to-noise ratio as the docstring of fastspeech2_amd/hnr.py specifies it: the
frame by explicit indexing, the lag sums through np.correlate (another algorithm and another order than the kernel's direct,
compensated sums), the window sizes from integer arithmetic, the moments and path sums with numpy's own sums.  Written from the
specification, not from the kernels; it imports nothing of the package.  `dtype=np.longdouble` runs the same chain, its tables
included, in extended precision, the lag sums then as dot products (np.correlate is double only): tests/golden/make_hnr_bars.py
measures the fp64 chain's own rounding with it.  Also the test inputs of tests/test_hnr_cpu.py and tests/test_hnr_gpu.py."""
import functools
import math

import numpy as np

F0_FLOOR, F0_CEIL = 71.0, 800.0
SEARCH = 1.2
R_LO, R_HI = 1e-3, 1 - 1e-6
SILENT = 1e-20
CORR_FLOOR = 1e-24
RATES = ((4000, 50), (22050, 256))
KEYS = ("hnr_mean_db_ref", "hnr_mean_db_syn", "hnr_std_db_ref", "hnr_std_db_syn", "hnr_frames_ref", "hnr_frames_syn", "hnr_cells",
        "hnr_diff_db", "hnr_rmse_db", "hnr_corr")


# ------------------------------------------------------------------------------------------------ the chain
def window(fs):
    """-> (h, N, LMAX): 4.5 periods of 71 Hz, h = floor(4.5 fs / 142) = floor(9 fs / 284)"""
    h = (9 * fs) // 284
    return h, 2 * h + 1, fs // 71 + 2


@functools.lru_cache(maxsize=None)
def tables(fs, dtype=np.float64):
    """-> (w (N,), rw (LMAX + 1,)) in `dtype`"""
    _, N, lmax = window(fs)
    pi = 4 * np.arctan(dtype(1))
    w = np.array([dtype(0.5) - dtype(0.5) * np.cos(2 * pi * dtype(k + 1) / dtype(N + 1)) for k in range(N)], dtype)
    if dtype == np.float64:
        full = np.correlate(w, w, "full")                                   # lag tau at N - 1 + tau
        return w, full[N - 1:N + lmax] / full[N - 1]
    return w, np.array([np.dot(w[:N - tau], w[tau:]) for tau in range(lmax + 1)], dtype) / np.dot(w, w)


def frame(y, t, f0, fs, hop, dtype=np.float64, lag=None):
    """Frame t of the audio y (its n samples) at the track value f0 -> dict r, hnr, valid, lag and, for a valid frame, rprime (the
    three r' the peak is taken from) and margin (how far the best lag leads the runner-up in [l0, l1]; inf when it is alone).
    With `lag` the peak is taken at that lag instead of the best one (it must lie in [l0, l1])."""
    h, N, lmax = window(fs)
    w, rw = tables(fs, dtype)
    n, c = len(y), t * hop
    x = np.zeros(N, dtype)
    for k in range(max(0, h - c), min(N, n - c + h)):
        x[k] = y[c - h + k]
    a = (x - x.sum() / dtype(N)) * w
    r0 = (a * a).sum()
    invalid = {"r": dtype(0), "hnr": dtype(0), "valid": 0, "lag": 0}
    if not f0 > 0 or not r0 > dtype(SILENT) * N:
        return invalid
    tau0 = fs / float(f0)                                                   # the placement of the search is float64 in every chain
    if not tau0 < 1e9:
        return invalid
    l0, l1 = max(2, math.ceil(tau0 / SEARCH)), min(lmax - 1, math.floor(tau0 * SEARCH))
    if l1 < l0:
        return invalid
    if dtype == np.float64:
        ac = np.correlate(a, a, "full")[N - 1 + l0 - 1:N - 1 + l1 + 2]
    else:
        ac = np.array([np.dot(a[:N - tau], a[tau:]) for tau in range(l0 - 1, l1 + 2)], dtype)
    rp = ac / (r0 * rw[l0 - 1:l1 + 2])                                      # rp[i] is lag l0 - 1 + i
    inner = rp[1:-1]
    best = int(np.argmax(inner)) + 1 if lag is None else lag - l0 + 1       # np.argmax: the first maximum
    assert 1 <= best <= len(rp) - 2
    others = np.delete(inner, best - 1)
    margin = float(rp[best] - others.max()) if len(others) else math.inf
    rm, rc, rn = rp[best - 1], rp[best], rp[best + 1]
    d = rm - 2 * rc + rn
    peak = rc - (rn - rm) * (rn - rm) / (8 * d) if d < 0 else rc
    r = min(max(peak, dtype(R_LO)), dtype(R_HI))
    return {"r": r, "hnr": 10 * np.log10(r / (1 - r)), "valid": 1, "lag": l0 - 1 + best, "rprime": np.array([rm, rc, rn], dtype),
            "margin": margin}


def frames(y, f0, fs, hop, dtype=np.float64, lags=None):
    """every frame of a row -> (fr (T, 3) = r, hnr, valid in `dtype`, lag (T,) int, rprime (T, 3) (NaN where invalid), margin (T,))"""
    T = len(f0)
    fr, lag = np.zeros((T, 3), dtype), np.zeros(T, np.int64)
    rprime, margin = np.full((T, 3), np.nan, dtype), np.full(T, np.inf)
    for t in range(T):
        q = frame(y, t, f0[t], fs, hop, dtype, None if lags is None or not lags[t] else int(lags[t]))
        fr[t], lag[t] = (q["r"], q["hnr"], q["valid"]), q["lag"]
        if q["valid"]:
            rprime[t], margin[t] = q["rprime"], q["margin"]
    return fr, lag, rprime, margin


def side(fr, dtype=np.float64):
    """(T, >= 3) frames -> (n_valid, mean, M2) of hnr over the valid frames; zeros without one"""
    v = np.asarray(fr)[:, 1][np.asarray(fr)[:, 2] != 0].astype(dtype)
    if not len(v):
        return np.zeros(3, dtype)
    m = v.sum() / dtype(len(v))
    return np.array([len(v), m, ((v - m) ** 2).sum()], dtype)


def path_sums(pi, pj, fr_ref, fr_syn, dtype=np.float64):
    """-> (7,): P_v, mean x, mean y, Sxx, Syy, Sxy, Sd2 over the cells valid on both sides; zeros without one"""
    fa, fb = np.asarray(fr_ref), np.asarray(fr_syn)
    pi, pj = np.asarray(pi, np.int64), np.asarray(pj, np.int64)
    keep = (fa[pi, 2] != 0) & (fb[pj, 2] != 0) if len(pi) else np.zeros(0, bool)
    x, y = fa[pi[keep], 1].astype(dtype), fb[pj[keep], 1].astype(dtype)
    if not len(x):
        return np.zeros(7, dtype)
    P = dtype(len(x))
    xm, ym = x.sum() / P, y.sum() / P
    dx, dy = x - xm, y - ym
    return np.array([P, xm, ym, (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum(), ((x - y) ** 2).sum()], dtype)


def row_scores(fr_ref, fr_syn, pi, pj, dtype=np.float64):
    """the HNR keys of a pair from its two sides' frames and its path"""
    nan = dtype("nan")
    row = {}
    for name, fr in (("ref", fr_ref), ("syn", fr_syn)):
        n, m, m2 = side(fr, dtype)
        row["hnr_frames_" + name] = int(n)
        row["hnr_mean_db_" + name] = m if n else nan
        row["hnr_std_db_" + name] = np.sqrt(m2 / n) if n else nan
    P, xm, ym, sxx, syy, sxy, sd2 = path_sums(pi, pj, fr_ref, fr_syn, dtype)
    ok = P >= 2 and sxx > CORR_FLOOR * P and syy > CORR_FLOOR * P
    row["hnr_cells"] = int(P)
    row["hnr_diff_db"] = ym - xm if P else nan
    row["hnr_rmse_db"] = np.sqrt(sd2 / P) if P else nan
    row["hnr_corr"] = sxy / np.sqrt(sxx * syy) if ok else nan
    return {k: row[k] for k in KEYS}


def pair_scores(ref_y, ref_f0, syn_y, syn_f0, fs, hop, dtype=np.float64):
    """a time-aligned pair along the diagonal of its shorter side: the whole chain"""
    fa, fb = frames(ref_y, ref_f0, fs, hop, dtype)[0], frames(syn_y, syn_f0, fs, hop, dtype)[0]
    k = np.arange(min(len(fa), len(fb)))
    return row_scores(fa, fb, k, k, dtype)


# ------------------------------------------------------------------------------------------------ inputs
def tone(f0, n, fs, rng=None, snr_db=None, amp=0.3):
    """n float32 samples of a tone of up to ten harmonics of amplitude 1 / k below 0.45 fs with fixed phases, plus white Gaussian
    noise at `snr_db` (the ratio of the tone's power to the noise's) from `rng`"""
    t = np.arange(n, dtype=np.float64) / fs
    K = max(1, min(10, int(0.45 * fs / f0)))
    x = sum(np.sin(2 * np.pi * f0 * k * t + 0.7 * k * k) / k for k in range(1, K + 1))
    x *= amp / np.sqrt(np.mean(x ** 2) * 2)
    if snr_db is not None:
        x = x + rng.standard_normal(n) * np.sqrt(np.mean(x ** 2) / 10 ** (snr_db / 10))
    return x.astype(np.float32)


def noisier(y, rng, snr_db):
    """y plus white noise at snr_db below y's own power"""
    y = np.asarray(y, np.float64)
    return (y + rng.standard_normal(len(y)) * np.sqrt(np.mean(y ** 2) / 10 ** (snr_db / 10))).astype(np.float32)


def n_frames(n, hop):
    return n // hop + 1


# name -> (fs, hop, seed, ((samples, f0 of the tone, snr), ..)): ragged batches of three rows.  Row 0 is shorter than one window
# (every frame crosses both ends of the signal), row 1 has one frame more than a multiple of nothing in particular, row 2 is the
# long one: its first and last frames cross one end, it has an all-zero stretch, an unvoiced run and frames at F0_FLOOR and F0_CEIL
CASES = {
    "fs4000": (4000, 50, 9501, ((120, 150.0, 15.0), (777, 100.0, 5.0), (2990, 220.5, 25.0))),
    "fs22050": (22050, 256, 9502, ((700, 147.0, 20.0), (4100, 300.0, 10.0), (12100, 100.0, 30.0))),
    "one_frame": (4000, 50, 9503, ((30, 200.0, 10.0),)),
}


@functools.lru_cache(maxsize=None)
def case_input(name):
    """-> (fs, hop, [(y float32 (n,), f0 float64 (T,))])"""
    fs, hop, seed, spec = CASES[name]
    rng = np.random.default_rng(seed)
    rows = []
    for b, (n, f, snr) in enumerate(spec):
        y = tone(f, n, fs, rng, snr)
        T = n_frames(n, hop)
        f0 = np.full(T, f) * np.exp(0.02 * rng.standard_normal(T))          # a track a little off the truth, as an estimator's is
        if b == 2:
            y[n // 2:n // 2 + 6 * hop + window(fs)[1]] = 0.0                 # silent: the frames wholly inside are invalid
            f0[3:6] = 0.0                                                   # unvoiced
            f0[7], f0[8], f0[T - 2] = F0_FLOOR, F0_CEIL, F0_FLOOR           # the search clipped by LMAX, and the shortest lags
            f0[9] = -5.0                                                    # anything not above 0 is unvoiced
        rows.append((y, f0))
    return fs, hop, rows


# name -> what the hand-built path is for
PATH_CASES = ("none_shared", "one_shared", "one_side_invalid", "diagonal", "corner")


@functools.lru_cache(maxsize=None)
def path_case(name):
    """-> (fr_ref (T1, 3), fr_syn (T2, 3), pi, pj): frames with random hnr in [-10, 40] dB (r consistent with it) and hand-set validity"""
    rng = np.random.default_rng(9600 + PATH_CASES.index(name))
    T1, T2 = {"none_shared": (9, 7), "one_shared": (9, 7), "one_side_invalid": (40, 40), "diagonal": (257, 257), "corner": (40, 300)}[name]

    def fr(T, valid):
        hnr = rng.uniform(-10, 40, T)
        out = np.stack([1 / (1 + 10 ** (-hnr / 10)), hnr, np.ones(T)], axis=1)
        out[~valid] = 0.0
        return out

    va, vb = np.ones(T1, bool), np.ones(T2, bool)
    if name == "none_shared":
        vb[:] = False
    elif name == "one_shared":
        va[:] = False
        va[T1 - 1] = True                                                   # only the path's last cell (T1 - 1, T2 - 1) is shared
        vb[:T2 - 1] = False
    elif name == "one_side_invalid":
        vb[5:17] = False
        vb[30] = False
    else:
        va[rng.integers(0, T1, T1 // 5)] = False
        vb[rng.integers(0, T2, T2 // 5)] = False
    if name == "corner":
        pi = np.concatenate([np.zeros(T2, np.int32), np.arange(1, T1, dtype=np.int32)])
        pj = np.concatenate([np.arange(T2, dtype=np.int32), np.full(T1 - 1, T2 - 1, np.int32)])
        va[0], vb[T2 - 1] = True, True
    elif T1 == T2:
        pi = pj = np.arange(T1, dtype=np.int32)
    else:                                                                   # down the first column, then along the last row
        pi = np.concatenate([np.arange(T1, dtype=np.int32), np.full(T2 - 1, T1 - 1, np.int32)])
        pj = np.concatenate([np.zeros(T1, np.int32), np.arange(1, T2, dtype=np.int32)])
    return fr(T1, va), fr(T2, vb), pi, pj.copy()
