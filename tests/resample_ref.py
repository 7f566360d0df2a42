"""fp64 numpy statement of the resampler and peak normalisation that fastspeech2_amd/resample.py specifies (the oracle of
tests/test_resample_cpu.py and tests/test_resample_gpu.py).  Written from the formula, independent of the product's tap builder."""
from math import gcd

import numpy as np
from scipy.signal import firwin


def factors(sr_in, sr_out):
    g = gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def taps(up, down):
    """(h [2 half + 1] fp64, half)"""
    m = max(up, down)
    half = 10 * m
    return up * firwin(2 * half + 1, 1.0 / m, window=("kaiser", 5.0)), half


def resample_ref(x, sr_in, sr_out):
    """y[j] = sum_i x[i] h[j down - i up + half], n_out = ceil(n_in up / down); fp64 in, fp64 out.  The terms are accumulated one input offset at a time,
    in descending i (<= 45 terms per output)."""
    x = np.asarray(x, dtype=np.float64)
    up, down = factors(sr_in, sr_out)
    if up == down:
        return x.copy()
    h, half = taps(up, down)
    n_in = len(x)
    n_out = -(-n_in * up // down)
    y = np.zeros(n_out)
    j = np.arange(n_out, dtype=np.int64)
    c = j * down + half                                         # k = c - i up in [0, 2 half]  <=>  i in [ceil((c - 2 half) / up), c // up]
    i_hi = c // up
    n_terms = 2 * half // up + 1
    for t in range(n_terms + 1):
        i = i_hi - t
        k = c - i * up
        ok = (k >= 0) & (k <= 2 * half) & (i >= 0) & (i < n_in)
        term = np.zeros(n_out)
        term[ok] = x[i[ok]] * h[k[ok]]
        y += term
    return y


def peaknorm_ref(y, max_wav_value):
    """the reference's `(wav / max(abs(wav)) * max_wav_value).astype(np.int16)` on a float32 array (numpy float32 arithmetic)"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (y / np.max(np.abs(y)) * np.float32(max_wav_value)).astype(np.int16)
