"""An independent numpy restatement of the over-smoothing scores as the docstring of fastspeech2_amd/modspec.py specifies them:
the moments with numpy's own sums, the modulation spectrum with np.fft.rfft of the zero-padded mean-removed trajectory (another
algorithm than the kernel's direct sum), the bands from exact fractions.  Written from the specification, not from the kernels; it
imports nothing of the package.  `dtype=np.longdouble` runs the same chain in extended precision with the direct sum against
extended-precision twiddles in place of numpy's double-only FFT (tests/golden/make_modspec_bars.py measures the fp64 chain's own
rounding with it).  Also the test inputs of tests/test_modspec_gpu.py and tests/test_modspec_cpu.py."""
from fractions import Fraction

import numpy as np

N = 4096
HALF = N // 2
FLOOR = 1e-12
MIN_FRAMES = 32
EDGES_HZ = (0, Fraction(1, 2), 1, 2, 4, 8, 16, 32)
RATES = ((22050, 256), (16000, 200))                                       # the two band tables of the tests
EVERY_T = (1, 2, 31, 32, 33, 255, 256, 257, 2047, 2048)

# name -> (seed, K, frames per row): ragged batches that mix the lengths at which the kernels change what they do (one frame, the
# MIN_FRAMES rule, one lane's worth of frames more or less, the frame bound), at every K of interest
CASES = {
    "k13": (7001, 13, (33, 2048, 1, 256, 31, 2047, 2, 257, 32, 255)),
    "k1": (7002, 1, (2047, 1, 256, 2, 33, 32, 2048, 31, 257, 255)),
    "k40": (7003, 40, (257, 31, 2047, 32)),
    "k128": (7004, 128, (256, 2, 2048, 255)),
    "one_row": (7005, 13, (300,)),
}
COSINE_A, COSINE_T, COSINE_CYCLES = 0.75, 1024, 64                         # A cos(2 pi 64 t / 1024): bin 256 of the 4096 grid
CONSTANT, CONSTANT_T = 1.625, 500
SMOOTH_SEED, SMOOTH_T = 11, 1024                                            # the noise trajectory of the smoothing test


def case_input(name):
    """[(T, K) float64]: the rows of a case, noise about an offset per coefficient, as cepstra are"""
    if name == "cosine":
        t = np.arange(COSINE_T, dtype=np.float64)
        return [(COSINE_A * np.cos(2.0 * np.pi * COSINE_CYCLES * t / COSINE_T))[:, None]]
    if name == "constant":
        return [np.full((CONSTANT_T, 1), CONSTANT)]
    seed, K, frames = CASES[name]
    rng = np.random.default_rng(seed)
    offset, scale = 2.0 * rng.standard_normal(K), rng.uniform(0.1, 1.0, K)
    return [offset + scale * rng.standard_normal((T, K)) for T in frames]


def band_bins(sampling_rate, hop_length):
    """[(first bin, end bin)] and [(lower, upper) Hz] of the bands: the bins f >= 1 whose frequency f (sr / hop) / N is at or above
    the band's lower edge and below its upper one; the last band, which ends at the frame-rate Nyquist, takes bin N / 2 as well"""
    freq = [Fraction(f * sampling_rate, hop_length * N) for f in range(HALF + 1)]
    nyquist = Fraction(sampling_rate, 2 * hop_length)
    edges = [Fraction(e) for e in EDGES_HZ if e < nyquist] + [nyquist]
    bins, hz = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        inside = [f for f in range(1, HALF + 1) if lo <= freq[f] < hi or (hi == nyquist and freq[f] == nyquist)]
        if inside:
            assert inside == list(range(inside[0], inside[-1] + 1))
            bins.append((inside[0], inside[-1] + 1))
            hz.append((float(lo), float(hi)))
    return bins, hz


def _twiddles_longdouble():
    a = 2 * (np.arctan(np.longdouble(1)) * 4) * np.arange(N).astype(np.longdouble) / N
    return np.cos(a), np.sin(a)


_LD = []


def power(x, dtype=np.float64):
    """x (T, K) mean-removed -> |X[f]|^2 (K, N / 2 + 1) of the trajectories zero-padded to N"""
    T = len(x)
    if dtype == np.float64:
        X = np.fft.rfft(x, n=N, axis=0).T
        return X.real ** 2 + X.imag ** 2
    if not _LD:
        _LD.extend(_twiddles_longdouble())
    cos, sin = _LD
    out = np.empty((x.shape[1], HALF + 1), np.longdouble)
    t = np.arange(T, dtype=np.int64)
    for f0 in range(0, HALF + 1, 256):                                      # a block of bins at a time bounds the table
        idx = (np.arange(f0, min(f0 + 256, HALF + 1), dtype=np.int64)[:, None] * t[None, :]) % N
        re, im = cos[idx] @ x, sin[idx] @ x
        out[:, f0:f0 + len(idx)] = (re * re + im * im).T
    return out


def chain(c, tables=(), dtype=np.float64):
    """c (T, K) -> dict: mean, m2, gv (K,), logms (K, N / 2 + 1), and bands [(K, J)] in dB, one for each of `tables`' bin lists"""
    c = np.asarray(c, np.float64).astype(dtype)
    T = len(c)
    mean = c.sum(axis=0) / dtype(T)
    x = c - mean
    m2 = (x * x).sum(axis=0)
    logms = np.log(power(x, dtype) / dtype(T) + dtype(FLOOR))
    db = dtype(10) / np.log(dtype(10))
    bands = [np.stack([logms[:, lo:hi].mean(axis=1) for lo, hi in bins], axis=1) * db for bins in tables]
    return {"mean": mean, "m2": m2, "gv": m2 / dtype(T), "logms": logms, "bands": bands}


def smoothed(c):
    """the trajectory filtered along time with the taps (1/4, 1/2, 1/4), its end frames repeated"""
    p = np.concatenate([c[:1], c, c[-1:]])
    return 0.25 * p[:-2] + 0.5 * p[1:-1] + 0.25 * p[2:]


def row_scores(ref, syn, bins, dtype=np.float64):
    """(T1, K), (T2, K) cepstra of a pair -> its smoothing keys, from the chain in `dtype`"""
    a, b = chain(ref, [bins], dtype), chain(syn, [bins], dtype)
    nan = float("nan")
    gr = a["gv"] if len(ref) >= 2 else np.full(ref.shape[1], nan)
    gs = b["gv"] if len(syn) >= 2 else np.full(syn.shape[1], nan)
    ok = (gr > 0) & (gs > 0)
    br, bs = a["bands"][0], b["bands"][0]
    if min(len(ref), len(syn)) < MIN_FRAMES:
        br, bs = np.full_like(br, nan), np.full_like(bs, nan)
    return {"gv_ref": gr, "gv_syn": gs, "gv_ratio_db": np.mean(10 * np.log10(gs[ok] / gr[ok])) if ok.any() else nan,
            "ms_db_ref": br, "ms_db_syn": bs, "ms_band_db_ref": br.mean(axis=0), "ms_band_db_syn": bs.mean(axis=0),
            "ms_dist_db": np.sqrt(((bs - br) ** 2).mean())}
