"""ITU-R BS.1770-4 programme loudness of a mono signal, restated in fp64 numpy / scipy for tests/test_loudness_cpu.py and
tests/test_loudness_gpu.py.  Independent of fastspeech2_amd/loudness.py: it shares no code with it.  The cascade is
scipy.signal.lfilter sample by sample from zero state, the blocks are a plain loop."""
import numpy as np
from scipy.signal import lfilter


def coefficients(fs):
    """the pre-filter (high shelf) and the RLB high-pass as (b, a) pairs, re-derived for rate fs by the bilinear transform"""
    def denominator(f0, Q):
        K = np.tan(np.pi * f0 / fs)
        a0 = 1.0 + K / Q + K * K
        return K, a0, np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    Q = 0.7071752369554196
    K, a0, a_shelf = denominator(1681.974450955533, Q)
    Vh = np.power(10.0, 3.999843853973347 / 20.0)
    Vb = np.power(Vh, 0.4996667741545416)
    b_shelf = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    _, _, a_hp = denominator(38.13547087602444, 0.5003270373238773)
    return (b_shelf, a_shelf), (np.array([1.0, -2.0, 1.0]), a_hp)


def sizes(fs):
    return int(round(0.4 * fs)), int(round(0.1 * fs))


def k_weight(x, fs):
    (b1, a1), (b2, a2) = coefficients(fs)
    return lfilter(b2, a2, lfilter(b1, a1, np.asarray(x, dtype=np.float64)))


def block_energies(x, fs):
    """z[i]: mean square of the K-weighted signal over [i h, i h + n), whole blocks only"""
    n, h = sizes(fs)
    y = k_weight(x, fs)
    z = []
    i = 0
    while i * h + n <= len(y):
        seg = y[i * h:i * h + n]
        z.append(float(np.sum(seg * seg)) / n)
        i += 1
    return np.array(z, dtype=np.float64)


def block_loudness(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def gated(z):
    """-> (integrated loudness, momentary maximum, blocks above the absolute gate, blocks above both gates, relative threshold)"""
    z = np.asarray(z, dtype=np.float64)
    if len(z) == 0:
        return float("nan"), float("nan"), 0, 0, float("nan")
    l = block_loudness(z)
    absolute = l > -70.0
    if not absolute.any():
        return float("-inf"), float(l.max()), 0, 0, float("nan")
    threshold = -0.691 + 10.0 * np.log10(z[absolute].mean()) - 10.0
    keep = absolute & (l > threshold)
    return float(-0.691 + 10.0 * np.log10(z[keep].mean())), float(l.max()), int(absolute.sum()), int(keep.sum()), float(threshold)


def loudness(x, fs):
    return gated(block_energies(x, fs))[0]


def ungated(x, fs):
    """the same measure without blocks or gates: the mean square of the whole K-weighted signal"""
    y = k_weight(x, fs)
    return float(-0.691 + 10.0 * np.log10(np.mean(y * y)))


def gain(loud, peak, target, ceiling_db):
    """-> (g, limited, fallback) for one utterance"""
    cap = 10.0 ** (ceiling_db / 20.0) / peak if peak > 0 else 0.0
    if not np.isfinite(loud):
        return cap, False, True
    g = 10.0 ** ((target - loud) / 20.0)
    return (cap, True, False) if g > cap else (g, False, False)


def cast(x, g):
    """-> (int16 samples, number of saturated samples)"""
    v = np.rint(np.asarray(x, dtype=np.float64) * g * 32768.0)
    return np.clip(v, -32768, 32767).astype(np.int16), int(np.count_nonzero((v > 32767) | (v < -32768)))
