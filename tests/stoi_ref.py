"""An independent numpy restatement of STOI (Taal et al. 2011) and ESTOI (Jensen and Taal 2016) as the docstring of
fastspeech2_amd/stoi.py specifies them, for signals that are already at 10 kHz: np.fft.rfft for the spectrum, a scatter-style
overlap-add loop, boolean indexing for the compaction.  Written from the specification, not from the kernels; it imports nothing
of the package.  `dtype=np.longdouble` runs the same chain in extended precision with a DFT matrix in place of numpy's double-only
FFT (tests/golden/make_stoi_bars.py measures the fp64 chain's own rounding with it).  Also the test inputs of tests/test_stoi_gpu.py."""
import numpy as np

FS, N, H, K, J, L = 10000, 256, 128, 512, 15, 30
EPS = 2.0 ** -52
SEED = 20111                                                                # of the test inputs
# no frame; one frame; 29 frames, M = 28; 30 frames, M = 29: the longest row without a segment; 31 frames, M = 30: one segment; long,
# with planted silences.  (The shorter rows have no silence, so that every frame of them is kept and M is what is said here.)
LENGTHS = (200, 257, 3968, 3969, 3969 + 128, 15000)


def window(dtype=np.float64):
    n = np.arange(1, N + 1).astype(dtype)
    return (1 - np.cos(2 * _pi(dtype) * n / (N + 1))) / 2


def _pi(dtype):
    return np.pi if dtype == np.float64 else np.arctan(np.longdouble(1)) * 4


def n_frames(length):
    return int(np.ceil((length - N) / H)) if length > N else 0


def bands():
    """(first bin, end bin) of each of the 15 bands, and the centre frequencies"""
    f = np.arange(K // 2 + 1) * (FS / K)
    out = []
    for k in range(J):
        lo, hi = 150.0 * 2.0 ** ((2 * k - 1) / 6.0), 150.0 * 2.0 ** ((2 * k + 1) / 6.0)
        out.append((int(np.argmin(np.abs(f - lo))), int(np.argmin(np.abs(f - hi)))))
    return out, [150.0 * 2.0 ** (k / 3.0) for k in range(J)]


def frames_of(x, dtype=np.float64):
    """(n_frames, 256): the windowed frames of x under the framing rule"""
    w = window(dtype)
    starts = [s for s in range(0, max(len(x) - N, 0), H)]
    return np.array([x[s:s + N] * w for s in starts], dtype=dtype).reshape(len(starts), N)


def remove_silent(x, y, dtype=np.float64):
    """-> (x', y', energies, mask): the frames of the clean signal within 40 dB of its loudest, overlap-added for both signals"""
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    fx, fy = frames_of(x, dtype), frames_of(y, dtype)
    e = (fx * fx).sum(axis=1) if len(fx) else np.zeros(0, dtype)
    mask = (e > dtype(1e-4) * e.max()) & (e.max() > 0) if len(e) else np.zeros(0, bool)
    fx, fy = fx[mask], fy[mask]
    n = len(fx)
    xo, yo = np.zeros((n - 1) * H + N if n else 0, dtype), np.zeros((n - 1) * H + N if n else 0, dtype)
    for i in range(n):
        xo[i * H:i * H + N] += fx[i]
        yo[i * H:i * H + N] += fy[i]
    return xo, yo, e, mask


_dft = {}


def _power(frames, dtype):
    """|DFT_512|^2 of the zero-padded frames, bins 0 .. 256"""
    if dtype == np.float64:
        s = np.fft.rfft(frames, K, axis=1)
        return s.real ** 2 + s.imag ** 2
    if "m" not in _dft:                                                     # exact angle reduction, then longdouble cos / sin
        j = (np.arange(K // 2 + 1)[:, None] * np.arange(N)[None, :]) % K
        a = 2 * _pi(dtype) * j.astype(dtype) / K
        _dft["m"] = (np.cos(a), np.sin(a))
    c, s = _dft["m"]
    re, im = frames @ c.T, frames @ s.T
    return re * re + im * im


def band_magnitudes(xo, dtype=np.float64):
    """(15, M) of a compacted signal"""
    f = frames_of(xo, dtype)
    if not len(f):
        return np.zeros((J, 0), dtype)
    p = _power(f, dtype)
    return np.sqrt(np.array([p[:, lo:hi].sum(axis=1) for lo, hi in bands()[0]], dtype=dtype))


def segment_scores(X, Y, dtype=np.float64):
    """(2, M - 29): per segment the band-averaged STOI correlation and the ESTOI score"""
    M = X.shape[1]
    S = max(M - L + 1, 0)
    out = np.zeros((2, S), dtype)
    eps, clip = dtype(EPS), 1 + dtype(10) ** (dtype(15) / dtype(20))
    for s in range(S):
        xs, ys = X[:, s:s + L], Y[:, s:s + L]
        alpha = np.sqrt((xs ** 2).sum(axis=1, keepdims=True)) / (np.sqrt((ys ** 2).sum(axis=1, keepdims=True)) + eps)
        yp = np.minimum(alpha * ys, clip * xs)
        a = xs - xs.mean(axis=1, keepdims=True)
        b = yp - yp.mean(axis=1, keepdims=True)
        a = a / (np.sqrt((a ** 2).sum(axis=1, keepdims=True)) + eps)
        b = b / (np.sqrt((b ** 2).sum(axis=1, keepdims=True)) + eps)
        out[0, s] = (a * b).sum(axis=1).mean()
        a, b = xs - xs.mean(axis=1, keepdims=True), ys - ys.mean(axis=1, keepdims=True)
        a = a / (np.sqrt((a ** 2).sum(axis=1, keepdims=True)) + eps)
        b = b / (np.sqrt((b ** 2).sum(axis=1, keepdims=True)) + eps)
        a, b = a - a.mean(axis=0, keepdims=True), b - b.mean(axis=0, keepdims=True)
        a = a / (np.sqrt((a ** 2).sum(axis=0, keepdims=True)) + eps)
        b = b / (np.sqrt((b ** 2).sum(axis=0, keepdims=True)) + eps)
        out[1, s] = (a * b).sum() / L
    return out


def chain(x, y, dtype=np.float64):
    """every stage of one pair at 10 kHz, cut to the shorter length: a dict of e, mask, map, xo, yo, X, Y, seg, stoi, estoi, frames,
    frames_kept, segments, too_short"""
    n = min(len(x), len(y))
    xo, yo, e, mask = remove_silent(x[:n], y[:n], dtype)
    X, Y = band_magnitudes(xo, dtype), band_magnitudes(yo, dtype)
    seg = segment_scores(X, Y, dtype)
    S = seg.shape[1]
    nan = dtype(np.nan)
    return {"e": e, "mask": mask, "map": np.flatnonzero(mask), "xo": xo, "yo": yo, "X": X, "Y": Y, "seg": seg,
            "stoi": seg[0].mean() if S else nan, "estoi": seg[1].mean() if S else nan, "frames": len(e), "frames_kept": int(mask.sum()),
            "segments": S, "too_short": S == 0}


def scores(x, y):
    c = chain(x, y)
    return float(c["stoi"]), float(c["estoi"])


# ------------------------------------------------------------------------------------------------ test inputs
def signal(length, rng, silences=True):
    """harmonic tones under a slow envelope plus noise, float32, with (near) silence planted at the start, in the middle and at the end"""
    t = np.arange(length) / FS
    f0 = rng.uniform(110.0, 220.0)
    x = sum(rng.uniform(0.3, 1.0) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) for h in range(1, 16))
    x = 0.1 * x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 2 * np.pi))) + 0.01 * rng.standard_normal(length)
    if silences and length >= 10000:
        for a, b in ((0, length // 12), (length // 2, length // 2 + length // 10), (length - length // 9, length)):
            x[a:b] = 1e-5 * rng.standard_normal(b - a)
    return x.astype(np.float32)


def pairs(lengths=LENGTHS, seed=SEED):
    """[(clean, degraded)] float32 at 10 kHz: the degraded side is the clean one through a gain, a soft clipper and added noise"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        x = signal(n, rng)
        y = np.tanh(3.0 * x.astype(np.float64)) / 3.0 * 0.8 + 0.02 * rng.standard_normal(n)
        out.append((x, y.astype(np.float32)))
    return out


LENGTHS_22K = (9100, 33075, 500)                                            # at 22 050 Hz: one segment and a bit; 1.5 s; no frame


def pairs_22k(lengths=LENGTHS_22K, seed=SEED + 1):
    """the same kind of pairs, generated on a 22 050 Hz grid (for the end-to-end test, which resamples them)"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        t = np.arange(n) / 22050.0
        f0 = rng.uniform(110.0, 220.0)
        x = sum(rng.uniform(0.3, 1.0) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) for h in range(1, 16))
        x = 0.1 * x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t)) + 0.01 * rng.standard_normal(n)
        if n >= 30000:
            x[n // 2:n // 2 + n // 8] = 1e-5 * rng.standard_normal(n // 8)
        y = np.tanh(3.0 * x) / 3.0 * 0.8 + 0.02 * rng.standard_normal(n)
        out.append((x.astype(np.float32), y.astype(np.float32)))
    return out


def threshold_margin(c):
    """the smallest | e_j / (1e-4 e_max) - 1 | over the frames of a chain: how far the keep decision is from flipping"""
    e = np.asarray(c["e"], np.float64)
    return float(np.abs(e / (1e-4 * e.max()) - 1.0).min()) if len(e) and e.max() > 0 else np.inf
