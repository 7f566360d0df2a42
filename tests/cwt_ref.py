"""An independent numpy restatement of the wavelet prosody scores as the docstring of fastspeech2_amd/cwt.py specifies them: the
continuous ln F0 by explicit loops over the frames, the transform as a zero-padded linear convolution with np.fft (another
algorithm than the kernel's direct sum), the scales and cut-offs from exact fractions, the path sums with numpy's own sums.  Written
from the specification, not from the kernels; it imports nothing of the package.  `dtype=np.longdouble` runs the same chain in
extended precision, the transform then as a direct sum (numpy's FFT is double only): tests/golden/make_cwt_bars.py measures the
fp64 chain's own rounding with it.  Also the test inputs of tests/test_cwt_cpu.py and tests/test_cwt_gpu.py."""
from fractions import Fraction

import numpy as np

from tests.modspec_ref import RATES  # noqa: F401  ((22050, 256), (16000, 200)): the two rate pairs of the tests

SCALES, LEVELS, COMPONENTS = 10, 5, 15
MAX_FRAMES = 2048
FLAT_SD = 1e-12
CORR_FLOOR = 1e-24

# name -> (seed, ((frames, pattern), ..)): ragged batches of F0 tracks.  `lengths` holds every T at which the kernels change what
# they do (one frame, two, one tile of 256 less or more one, the frame bound); `mixed5` the voicing patterns; `degenerate` rows that
# are flat by definition (their frame counts are powers of two so that the mean of equal values is exact in every arithmetic)
CASES = {
    "lengths": (9101, ((1, "all"), (2, "all"), (255, "runs"), (256, "runs"), (257, "runs"), (2048, "runs"))),
    "mixed5": (9102, ((300, "lead_trail"), (77, "alternating"), (513, "ends"), (64, "one"), (150, "runs"))),
    "degenerate": (9103, ((100, "none"), (256, "constant"), (64, "one"))),
}
# name -> (seed, T1, T2, path): pairs of all-voiced tracks for the path sums
PATH_CASES = {"diagonal": (9201, 257, 257, "diagonal"), "corner": (9202, 40, 300, "corner"), "long": (9203, 2048, 2048, "corner")}


# ------------------------------------------------------------------------------------------------ inputs
def track(rng, T, pattern):
    """an F0 track in Hz of T frames, 0 = unvoiced"""
    t = np.arange(T, dtype=np.float64)
    f = 120.0 * np.exp(0.25 * np.sin(2.0 * np.pi * t / 97.0 + rng.uniform(0, 6.28)) + 0.05 * rng.standard_normal(T))
    v = np.ones(T, bool)
    if pattern == "runs":
        v[:] = False
        pos, on = int(rng.integers(0, 20)), True
        while pos < T:
            n = int(rng.integers(3, 41))
            v[pos:pos + n] = on
            pos, on = pos + n, not on
        v[T // 2] = True
    elif pattern == "none":
        v[:] = False
    elif pattern == "one":
        v[:] = False
        v[T // 3] = True
    elif pattern == "ends":
        v[1:-1] = False
    elif pattern == "lead_trail":
        v[:int(0.4 * T)] = False
        v[int(0.8 * T):] = False
    elif pattern == "alternating":
        v[1::2] = False
    elif pattern == "constant":
        f[:] = 150.0
    elif pattern != "all":
        raise KeyError(pattern)
    return np.where(v, f, 0.0)


def case_input(name):
    seed, rows = CASES[name]
    rng = np.random.default_rng(seed)
    return [track(rng, T, pattern) for T, pattern in rows]


def diagonal(T):
    k = np.arange(T, dtype=np.int32)
    return k, k.copy()


def corner(T1, T2):
    """all of the synthesized side at reference frame 0, then all of the reference side at the last synthesized frame"""
    pi = np.concatenate([np.zeros(T2, np.int32), np.arange(1, T1, dtype=np.int32)])
    pj = np.concatenate([np.arange(T2, dtype=np.int32), np.full(T1 - 1, T2 - 1, np.int32)])
    return pi, pj


def path_case(name):
    """-> (f0_ref, f0_syn, pi, pj)"""
    seed, T1, T2, kind = PATH_CASES[name]
    rng = np.random.default_rng(seed)
    a, b = track(rng, T1, "runs"), track(rng, T2, "runs")
    pi, pj = diagonal(T1) if kind == "diagonal" else corner(T1, T2)
    return a, b, pi, pj


def halved(f0):
    """the track with its ln F0 excursions about the mean of the voiced frames halved, on the same voiced frames"""
    v = f0 > 0
    lf = np.log(f0[v])
    out = np.zeros_like(f0)
    out[v] = np.exp(lf.mean() + 0.5 * (lf - lf.mean()))
    return out


def moving_average(f0, n=9):
    """an all-voiced track whose ln F0 is the n-frame moving average of the input's, the end frames repeated"""
    lf = np.log(f0)
    p = np.concatenate([np.full(n // 2, lf[0]), lf, np.full(n // 2, lf[-1])])
    return np.exp(np.convolve(p, np.full(n, 1.0 / n), mode="valid"))


def wiggly(T=600, seed=9301):
    """an all-voiced track: a slow movement plus frame-to-frame noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    return 140.0 * np.exp(0.2 * np.sin(2.0 * np.pi * t / 300.0) + 0.1 * np.sin(2.0 * np.pi * t / 37.0) + 0.05 * rng.standard_normal(T))


# ------------------------------------------------------------------------------------------------ the chain
def contour(f0, dtype=np.float64):
    """f0 (T,) -> dict x (T,) (None without a voiced frame), z (T,), n_voiced, m, sd, flat"""
    f0 = np.asarray(f0, np.float64)
    T = len(f0)
    voiced = [t for t in range(T) if f0[t] > 0]
    zero = np.zeros(T, dtype)
    if not voiced:
        return {"x": None, "z": zero, "n_voiced": 0, "m": dtype(0), "sd": dtype(0), "flat": 1}
    x = np.zeros(T, dtype)
    for t in voiced:
        x[t] = np.log(dtype(f0[t]))
    for t in range(T):
        if f0[t] > 0:
            continue
        t0, t1 = t - 1, t + 1
        while t0 >= 0 and not f0[t0] > 0:
            t0 -= 1
        while t1 < T and not f0[t1] > 0:
            t1 += 1
        if t0 < 0:
            x[t] = x[t1]
        elif t1 >= T:
            x[t] = x[t0]
        else:
            x[t] = x[t0] + (x[t1] - x[t0]) * (dtype(t - t0) / dtype(t1 - t0))
    m = x.sum() / dtype(T)
    sd = np.sqrt(((x - m) ** 2).sum() / dtype(T))
    flat = int(not sd > FLAT_SD)
    return {"x": x, "z": zero if flat else (x - m) / sd, "n_voiced": len(voiced), "m": m, "sd": sd, "flat": flat}


def scale_fraction(i, sampling_rate, hop_length):
    """a_i in frames, exactly: 2^(i+1) * 5 ms * sampling_rate / hop_length"""
    return Fraction(2 ** (i + 1) * sampling_rate, 200 * hop_length)


def scales(sampling_rate, hop_length, dtype=np.float64):
    fr = [scale_fraction(i, sampling_rate, hop_length) for i in range(1, SCALES + 1)]
    if fr[0] < 1:
        raise ValueError("the smallest scale is below one frame")
    return np.array([dtype(f.numerator) / dtype(f.denominator) for f in fr], dtype)


def cutoff(i, sampling_rate, hop_length):
    """the last d of scale i's table: min(2047, floor(10 a_i))"""
    f = 10 * scale_fraction(i, sampling_rate, hop_length)
    return min(MAX_FRAMES - 1, f.numerator // f.denominator)


def scale_weight(i, dtype=np.float64):
    return (dtype(i) + dtype(2.5)) ** dtype(-2.5)


def psi(x, dtype=np.float64):
    pi = 4 * np.arctan(dtype(1))
    return dtype(2) / (np.sqrt(dtype(3)) * pi ** dtype(0.25)) * (1 - x * x) * np.exp(-(x * x) / 2)


def table(i, sampling_rate, hop_length, dtype=np.float64):
    """tab_i[d], d = 0 .. cutoff"""
    a = scales(sampling_rate, hop_length, dtype)[i - 1]
    d = np.arange(cutoff(i, sampling_rate, hop_length) + 1).astype(dtype)
    return a ** dtype(-0.5) * scale_weight(i, dtype) * psi(d / a, dtype)


def transform(z, sampling_rate, hop_length, dtype=np.float64):
    """z (T,) -> (W (10, T), power (10,)): the float64 chain by an FFT convolution, any other by the direct sum"""
    z = np.asarray(z).astype(dtype)
    T = len(z)
    W = np.zeros((SCALES, T), dtype)
    for i in range(1, SCALES + 1):
        tab = table(i, sampling_rate, hop_length, dtype)
        n = len(tab)
        if dtype == np.float64:
            full = np.concatenate([tab[:0:-1], tab])                        # d = -(n - 1) .. n - 1
            L = 1 << int(np.ceil(np.log2(T + len(full))))
            W[i - 1] = np.fft.irfft(np.fft.rfft(z, L) * np.fft.rfft(full, L), L)[n - 1:n - 1 + T]
        else:
            padded = np.zeros(max(T, n), dtype)
            padded[:n] = tab
            idx = np.abs(np.arange(T)[:, None] - np.arange(T)[None, :])
            for t0 in range(0, T, 256):                                     # a block of frames at a time bounds the matrix
                W[i - 1, t0:t0 + 256] = padded[idx[t0:t0 + 256]] @ z
    return W, (W * W).sum(axis=1)


def components(W):
    """(10, T) -> (15, T): the scales, then the levels W_(2j-1) + W_(2j)"""
    return np.concatenate([W, W[0::2] + W[1::2]])


def path_sums(pi, pj, W_ref, W_syn, dtype=np.float64):
    """-> (15, 4): Sxx, Syy, Sxy about the means over the path's cells, and Sd2"""
    x = components(np.asarray(W_ref).astype(dtype))[:, np.asarray(pi)]
    y = components(np.asarray(W_syn).astype(dtype))[:, np.asarray(pj)]
    P = dtype(x.shape[1])
    dx, dy = x - (x.sum(axis=1) / P)[:, None], y - (y.sum(axis=1) / P)[:, None]
    return np.stack([(dx * dx).sum(axis=1), (dy * dy).sum(axis=1), (dx * dy).sum(axis=1), ((x - y) ** 2).sum(axis=1)], axis=1)


KEYS = ("cwt_corr", "cwt_rmse", "cwt_level_corr", "cwt_level_rmse", "cwt_power_db_ref", "cwt_power_db_syn", "cwt_power_ratio_db",
        "lf0_mean_ref", "lf0_mean_syn", "lf0_std_ref", "lf0_std_syn")


def row_scores(f0_ref, f0_syn, pi, pj, sampling_rate, hop_length, dtype=np.float64):
    """the wavelet keys of a pair from its two F0 tracks and its path: the whole chain in `dtype`"""
    a, b = contour(f0_ref, dtype), contour(f0_syn, dtype)
    nan = dtype("nan")
    if a["flat"] or b["flat"]:
        return {k: np.full(LEVELS if "level" in k else SCALES, nan) if k.startswith("cwt") else nan for k in KEYS}
    (Wa, pa), (Wb, pb) = transform(a["z"], sampling_rate, hop_length, dtype), transform(b["z"], sampling_rate, hop_length, dtype)
    s = path_sums(pi, pj, Wa, Wb, dtype)
    P = len(pi)
    ok = (P >= 2) & (s[:, 0] > CORR_FLOOR * P) & (s[:, 1] > CORR_FLOOR * P)
    corr = np.where(ok, s[:, 2] / np.sqrt(np.where(ok, s[:, 0] * s[:, 1], 1)), nan)
    rmse = np.sqrt(s[:, 3] / dtype(P))
    dbr, dbs = 10 * np.log10(pa / dtype(len(f0_ref))), 10 * np.log10(pb / dtype(len(f0_syn)))
    return {"cwt_corr": corr[:SCALES], "cwt_rmse": rmse[:SCALES], "cwt_level_corr": corr[SCALES:], "cwt_level_rmse": rmse[SCALES:],
            "cwt_power_db_ref": dbr, "cwt_power_db_syn": dbs, "cwt_power_ratio_db": dbs - dbr, "lf0_mean_ref": a["m"], "lf0_mean_syn": b["m"],
            "lf0_std_ref": a["sd"], "lf0_std_syn": b["sd"]}
