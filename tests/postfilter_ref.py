"""An independent numpy restatement of the modulation-spectrum postfilter as the docstring of fastspeech2_amd/postfilter.py
specifies it: the statistics with a plain two-pass mean and sample standard deviation, the filter with np.fft.rfft / irfft at
N = 4096 (another algorithm than the kernel's direct sums).  Written from the specification, not from the kernels; of this project
it imports only tests/modspec_ref.py, the restatement of the modulation spectrum itself.  `dtype=np.longdouble` runs the same chain
in extended precision with direct sums against extended-precision twiddles in place of numpy's double-only FFT
(tests/golden/make_postfilter_bars.py measures the fp64 chain's own rounding with it).  Also the cases and the known-answer inputs
of tests/test_postfilter_cpu.py and tests/test_postfilter_gpu.py."""
import numpy as np

from tests import modspec_ref as mref

N, HALF, FLOOR, MIN_FRAMES = mref.N, mref.HALF, mref.FLOOR, mref.MIN_FRAMES
MAX_FRAMES = 2048
MAX_GAIN_DB = 20
K_DEFAULT = 0.85
RATE = (22050, 256)                                                         # the band table of the corpus test

# name -> (seed, K, frames per row).  Statistics: ragged batches that mix a frame, the MIN_FRAMES rule on both sides, more than one
# lane's worth of frames and the frame bound; `STATS_SPLITS` are the row ranges they are fed in, two and three unequal batches, one
# of which keeps no row at all.
STATS_CASES = {
    "s1": (8101, 1, (33, 2048, 1, 257, 31, 32, 257, 33, 32)),
    "s13": (8102, 13, (32, 1, 31, 2048, 33, 257, 32, 31, 257)),
    "s80": (8103, 80, (257, 31, 1, 2048, 32, 33, 257)),
}
STATS_SPLITS = {"s1": ((0, 4, 9), (0, 2, 3, 9)), "s13": ((0, 6, 9), (0, 1, 3, 9)), "s80": ((0, 2, 7), (0, 2, 3, 7))}
# Filter: every length at which the kernel changes what it does (one frame, the MIN_FRAMES rule, a lane's worth of frames more or
# less, the frame bound) at K = 1 and 13, the widest mel at fewer lengths, and the coefficient bound at T <= 257
EVERY_T = (1, 2, 31, 32, 33, 255, 256, 257, 2047, 2048)
FILTER_CASES = {
    "f13": (8201, 13, (33, 2048, 1, 256, 31, 2047, 2, 257, 32, 255)),
    "f1": (8202, 1, (2047, 1, 256, 2, 33, 32, 2048, 31, 257, 255)),
    "f80": (8203, 80, (257, 31, 2047, 32, 2048, 33)),
    "f128": (8204, 128, (256, 2, 257, 255, 32, 1)),
}
FILTER_K = {"f13": 0.85, "f1": 1.0, "f80": 0.85, "f128": 0.5}              # the emphasis coefficient each case runs at
STATS_ROWS, STATS_T = 6, 300                                                # the utterances behind a filter case's statistics
GAINS = (2.0, 0.5)                                                          # known answer 2: the a of mu_n = mu_g + 2 ln a
KNOWN_K = (0.3, 1.0)
KNOWN_SEED, KNOWN_T, KNOWN_COEF = 8301, 300, 3
CLAMP_BIN, CLAMP_DB = 256, 60.0                                             # known answer 5: mref's cosine sits in bin 256
CORPUS_SEED, CORPUS_ROWS, CORPUS_K, CORPUS_AR = 8401, 24, 4, 0.6            # known answer 4


def mild(c):
    """the trajectory filtered along time with the taps (0.2, 0.6, 0.2), its end frames repeated: -14 dB at the Nyquist, no zero"""
    p = np.concatenate([c[:1], c, c[-1:]])
    return 0.2 * p[:-2] + 0.6 * p[1:-1] + 0.2 * p[2:]


def average5(c):
    """the 5-tap moving average, its end frames repeated"""
    p = np.concatenate([c[:1], c[:1], c, c[-1:], c[-1:]])
    return (p[:-4] + p[1:-3] + p[2:-2] + p[3:-1] + p[4:]) / 5.0


def _noise(rng, T, K, offset, scale):
    return offset + scale * rng.standard_normal((T, K))


def stats_input(name):
    """[(T, K) float64]: the rows of a statistics case, noise about an offset per coefficient"""
    seed, K, frames = STATS_CASES[name]
    rng = np.random.default_rng(seed)
    offset, scale = 2.0 * rng.standard_normal(K), rng.uniform(0.1, 1.0, K)
    return [_noise(rng, T, K, offset, scale) for T in frames]


def filter_input(name):
    """-> (rows [(T, K) float64]: mildly smoothed noise, as generated trajectories are; tables: the fp64 restatement's statistics of
    STATS_ROWS noise utterances (natural) and of the same smoothed (generated))"""
    seed, K, frames = FILTER_CASES[name]
    rng = np.random.default_rng(seed)
    offset, scale = 2.0 * rng.standard_normal(K), rng.uniform(0.1, 1.0, K)
    natural = [_noise(rng, STATS_T + 17 * j, K, offset, scale) for j in range(STATS_ROWS)]
    rows = [mild(_noise(rng, T, K, offset, scale)) for T in frames]
    return rows, tables(natural, [mild(c) for c in natural])


# ------------------------------------------------------------------------------------------------ the specification
_LD = []


def _twiddles(dtype):
    if dtype == np.float64:
        a = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
        return np.cos(a), np.sin(a)
    if not _LD:
        _LD.extend(mref._twiddles_longdouble())
    return _LD


def logms(c, dtype=np.float64):
    """c (T, K) -> ms (K, N / 2 + 1) as `modspec` defines it"""
    return mref.chain(c, (), dtype)["logms"]


def kept(T):
    return MIN_FRAMES <= T <= MAX_FRAMES


def statistics(rows, dtype=np.float64):
    """rows [(T, K)] -> (mean, sd (K, N / 2 + 1), kept, left out): two passes over the ms of the rows of MIN_FRAMES .. MAX_FRAMES frames"""
    ms = np.stack([logms(c, dtype) for c in rows if kept(len(c))]) if any(kept(len(c)) for c in rows) else np.zeros((0, 1, HALF + 1), dtype)
    n = len(ms)
    if n < 2:
        raise ValueError(f"{n} utterances of {MIN_FRAMES}..{MAX_FRAMES} frames: the statistics need at least 2")
    mean = ms.sum(axis=0) / dtype(n)
    sd = np.sqrt(((ms - mean) ** 2).sum(axis=0) / dtype(n - 1))
    return mean, sd, n, len(rows) - n


def tables(natural, generated, dtype=np.float64):
    """-> {mu_n, sd_n, mu_g, sd_g}"""
    mu_n, sd_n, _, _ = statistics(natural, dtype)
    mu_g, sd_g, _, _ = statistics(generated, dtype)
    return {"mu_n": mu_n, "sd_n": sd_n, "mu_g": mu_g, "sd_g": sd_g}


def _forward(x, dtype):
    """x (T, K) mean-removed -> X (N / 2 + 1, K) complex as (re, im)"""
    if dtype == np.float64:
        X = np.fft.rfft(x, n=N, axis=0)
        return X.real, X.imag
    cos, sin = _twiddles(dtype)
    t = np.arange(len(x), dtype=np.int64)
    re, im = np.empty((HALF + 1, x.shape[1]), dtype), np.empty((HALF + 1, x.shape[1]), dtype)
    for f0 in range(0, HALF + 1, 256):
        idx = (np.arange(f0, min(f0 + 256, HALF + 1), dtype=np.int64)[:, None] * t[None, :]) % N
        re[f0:f0 + len(idx)], im[f0:f0 + len(idx)] = cos[idx] @ x, -(sin[idx] @ x)
    return re, im


def _inverse(re, im, T, dtype):
    """the first T samples of the real inverse transform of the half spectrum (re, im) (N / 2 + 1, K)"""
    if dtype == np.float64:
        return np.fft.irfft(re + 1j * im, n=N, axis=0)[:T]
    cos, sin = _twiddles(dtype)
    w = np.full((HALF + 1, 1), 2, dtype)
    w[0], w[HALF] = 1, 1
    a, b = w * re, w * im
    b[0], b[HALF] = 0, 0
    f = np.arange(HALF + 1, dtype=np.int64)
    out = np.empty((T, re.shape[1]), dtype)
    for t0 in range(0, T, 256):
        idx = (np.arange(t0, min(t0 + 256, T), dtype=np.int64)[:, None] * f[None, :]) % N
        out[t0:t0 + len(idx)] = (cos[idx] @ a - sin[idx] @ b) / dtype(N)
    return out


def gains(ms, tab, k, dtype=np.float64):
    """ms (K, N / 2 + 1) and the tables -> g (K, N / 2 + 1)"""
    mu_n, sd_n, mu_g, sd_g = (np.asarray(tab[n]).astype(dtype) for n in ("mu_n", "sd_n", "mu_g", "sd_g"))
    r = np.where(sd_g > 0, sd_n / np.where(sd_g > 0, sd_g, 1), dtype(1))
    target = r * (ms - mu_g) + mu_n
    bound = dtype(MAX_GAIN_DB) * np.log(dtype(10)) / dtype(20)
    g = np.exp(np.clip(dtype(0.5) * dtype(k) * (target - ms), -bound, bound))
    g[:, 0] = 1
    return g


def apply(c, tab, k=K_DEFAULT, dtype=np.float64):
    """c (T, K) -> the filtered (T, K); a row outside MIN_FRAMES .. MAX_FRAMES frames, and any row at k = 0, is returned as it is"""
    c64 = np.asarray(c, np.float64)
    T = len(c64)
    if not kept(T) or k == 0:
        return c64.astype(dtype)
    c = c64.astype(dtype)
    mean = c.sum(axis=0) / dtype(T)
    x = c - mean
    re, im = _forward(x, dtype)
    ms = np.log((re * re + im * im).T / dtype(T) + dtype(FLOOR))
    g = gains(ms, tab, k, dtype).T
    return mean + _inverse(g * re, g * im, T, dtype)


# ------------------------------------------------------------------------------------------------ known answers
def known_row():
    """(KNOWN_T, KNOWN_COEF): one seeded noise trajectory, and flat statistics around it"""
    rng = np.random.default_rng(KNOWN_SEED)
    c = _noise(rng, KNOWN_T, KNOWN_COEF, np.array([1.5, -4.0, 0.25]), np.array([1.0, 0.3, 2.0]))
    flat = {"mu_n": rng.standard_normal((KNOWN_COEF, HALF + 1)), "sd_n": rng.uniform(0.5, 2.0, (KNOWN_COEF, HALF + 1))}
    flat["mu_g"], flat["sd_g"] = flat["mu_n"].copy(), flat["sd_n"].copy()
    return c, flat


def gain_tables(a):
    """known answer 2: equal sd, mu_n = mu_g + 2 ln a at every f >= 1"""
    _, tab = known_row()
    tab = dict(tab)
    tab["mu_n"] = tab["mu_g"] + 2.0 * np.log(a)
    tab["mu_n"][:, 0] = tab["mu_g"][:, 0]
    return tab


def clamp_row():
    """(COSINE_T, 1): mref's cosine A cos(2 pi 256 t / 4096) with the angle reduced in integers first, so that the samples are good to
    an ulp (mref's own, from an angle of up to 400 radians, are good to 4e-14) and the closed form `clamp_factor` can be tested"""
    t = np.arange(mref.COSINE_T, dtype=np.int64)
    return (mref.COSINE_A * np.cos(2.0 * np.pi * ((CLAMP_BIN * t) % N).astype(np.float64) / N))[:, None]


def clamp_tables():
    """known answer 5 on `clamp_row` (K = 1): equal statistics but for bin CLAMP_BIN, whose natural mean lies CLAMP_DB above"""
    rng = np.random.default_rng(KNOWN_SEED + 1)
    tab = {"mu_g": rng.standard_normal((1, HALF + 1)), "sd_g": rng.uniform(0.5, 2.0, (1, HALF + 1))}
    tab["mu_n"], tab["sd_n"] = tab["mu_g"].copy(), tab["sd_g"].copy()
    tab["mu_n"][0, CLAMP_BIN] += CLAMP_DB * np.log(10.0) / 10.0
    return tab


def clamp_factor():
    """y = factor x for the cosine: bin CLAMP_BIN holds all of it (X = A T / 2 there), and a gain of g on that bin alone adds
    (g - 1)(2 / N)(A T / 2) cos = (g - 1)(T / N) x; g = 10 at the 20 dB clamp"""
    g = 10.0 ** (MAX_GAIN_DB / 20.0)
    return 1.0 + (g - 1.0) * mref.COSINE_T / N


def known_cases():
    """name -> (c (T, K), tables, k, expected (T, K) or None): what make_postfilter_bars.py takes the known answers' bars from"""
    c, flat = known_row()
    mean = c.sum(axis=0) / len(c)
    out = {}
    for k in KNOWN_K:
        out[f"equal_k{k}"] = (c, flat, k, c)
        for a in GAINS:
            out[f"gain{a}_k{k}"] = (c, gain_tables(a), k, mean + a ** k * (c - mean))
    const = mref.case_input("constant")[0]
    out["constant"] = (const, {n: v[:1] for n, v in flat.items()}, 1.0, const)
    cos = clamp_row()
    out["clamp"] = (cos, clamp_tables(), 1.0, clamp_factor() * cos)
    return out


def corpus():
    """known answer 4 -> (natural, generated): CORPUS_ROWS rows of 200 .. 600 frames, K = CORPUS_K; natural = AR(1) noise about an
    offset, generated = the same rows through the 5-tap moving average"""
    rng = np.random.default_rng(CORPUS_SEED)
    offset = np.array([1.0, -2.0, 0.5, 3.0])[:CORPUS_K]
    natural = []
    for T in rng.integers(200, 601, CORPUS_ROWS):
        e = rng.standard_normal((int(T) + 50, CORPUS_K))
        x = np.zeros_like(e)
        for t in range(1, len(e)):
            x[t] = CORPUS_AR * x[t - 1] + e[t]
        natural.append(offset + x[50:])
    return natural, [average5(c) for c in natural]


def corpus_summary(refs, syns, bins):
    """-> (ms_diff_db_by_band, gv_ratio_db_mean) of `modspec.summarize`, from the restatement's row scores"""
    rows = [mref.row_scores(a, b, bins) for a, b in zip(refs, syns)]
    diff = np.mean([r["ms_db_syn"] for r in rows], axis=0) - np.mean([r["ms_db_ref"] for r in rows], axis=0)
    return diff.mean(axis=0), float(np.mean([r["gv_ratio_db"] for r in rows]))
