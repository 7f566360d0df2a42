"""Programme loudness on the GPU (csrc/fs2_loudness.hip): the measurement of ITU-R BS.1770-4 / EBU R 128 for mono signals over ragged
batches, and the gain + int16 cast that `prepare_align(normalize="loudness")` uses.  The specification below is what the kernels and
the independent numpy / scipy restatement (tests/loudness_ref.py) implement.  Everything after the float32 load is fp64.

K-weighting.  Two biquads in cascade, the high-shelf "pre-filter" and the RLB high-pass, as bilinear re-parametrisations of the
standard's 48 kHz table so that the filter is right at any rate (`k_weighting`):

    shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
               K = tan(pi f0 / fs), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2
               b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0]
               a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
    high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and a0;  b = [1, -2, 1],  a as above

At fs = 48 000 these are the standard's coefficients (tests/test_loudness_cpu.py, to 1e-12).  The filter starts from zero state at
sample 0 of each utterance.

Blocks.  n = round(0.4 fs), h = round(0.1 fs) (`block_sizes`): block i covers [i h, i h + n), 400 ms with 75 % overlap; only whole
blocks inside the utterance count, n_blocks = (len - n) // h + 1, or 0 when len < n.  z[i] is the mean square of the K-weighted signal
over block i, l_i = -0.691 + 10 log10 z_i.

Gating.  Absolute gate l_i > -70; relative gate 10 LU below -0.691 + 10 log10 of the mean z of the absolutely gated blocks; the
integrated loudness is -0.691 + 10 log10 of the mean z over the blocks that pass both.  No block: NaN.  No block above -70: -inf.

The recursion on the GPU.  Each biquad runs in transposed direct form II (scipy.signal.lfilter's form, whose `zi` / `zf` are these
states):  y = b0 x + s1;  s1 = b1 x - a1 y + s2;  s2 = b2 x - a2 y.  The cascade's four states S = (shelf s1, s2, high-pass s1, s2)
follow S' = A S + B x, so a row is cut into chunks of L samples (`chunk_tables`): every chunk runs from ZERO state (one GPU thread per
chunk) and keeps its end state e0; the true start states follow from S[c + 1] = e0[c] + A^L S[c], a scan along the row that the
kernel carries out in log steps with the powers A^(L 2^d); the chunk's true output is its zero-state output plus the zero-input
response sum_j S[c][j] r_j[k].  `chunk_tables` returns A^L and the four r_j, and tests/test_loudness_cpu.py checks that identity in
numpy against lfilter over the whole row.  The kernel uses the start state directly: it runs the chunk a second time from S[c], which
is the same sum without a table.  Squares are added per chunk into pieces (hop i split at i h + n mod h, since 4 h != n at some
rates), chunks in ascending order, pieces in ascending order into blocks: fixed order, no atomics, the same bytes on every run.

Gain and cast (`gain`, `gain_pcm`).  g = 10^((target - L) / 20), then g = min(g, 10^(ceiling_db / 20) / peak) with peak the float32
sample peak (`resample.peak_abs`); `limited` says that the ceiling bound it.  NaN or -inf loudness (shorter than 400 ms, or digital
silence) takes the fallback g = 10^(ceiling_db / 20) / peak; a zero peak gives g = 0 and zeros.  pcm = int16(rint(x g 32768)) saturated
to [-32768, 32767], round-half-even, with a count of saturated samples per utterance.  This is deliberately not `peaknorm_pcm`'s
truncating, wrapping cast, which restates a quirk of the reference.

True peak (`measure(true_peak=True)`) is the sample peak of the row oversampled x 4 by this project's own `resample_poly` (scipy's
default Kaiser filter), NOT Annex 2's 48-tap interpolator: a reported number only, nothing is normalised to it.
"""
import math

import numpy as np
import torch

from . import _lib, ops, ragged

SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416)      # f0, gain in dB, Q, exponent of Vb
HIGHPASS = (38.13547087602444, 0.5003270373238773)                                          # f0, Q


# ------------------------------------------------------------------------------------------------ host, fp64
def _rate(fs):
    if int(fs) != fs or fs <= 0:
        raise ValueError(f"the sampling rate must be a positive integer, got {fs!r}")
    return int(fs)


def k_weighting(fs):
    """((b, a), (b, a)): the shelf and the high-pass at sampling rate fs, each b [3], a [3] (a[0] = 1), fp64."""
    fs = _rate(fs)
    f0, G, Q, e = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** e
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, highpass


def block_sizes(fs):
    """(n, h): samples per 400 ms block and per 100 ms hop."""
    fs = _rate(fs)
    return int(round(0.4 * fs)), int(round(0.1 * fs))


def n_blocks(length, fs):
    """whole blocks inside an utterance of `length` samples"""
    n, h = block_sizes(fs)
    return (int(length) - n) // h + 1 if length >= n else 0


def state_matrix(fs):
    """(A [4, 4], C [4]): zero-input recursion S' = A S and output y = C S of the cascade, S = (shelf s1, s2, high-pass s1, s2)."""
    (b, a), (c, d) = k_weighting(fs)
    A = np.array([[-a[1], 1.0, 0.0, 0.0],
                  [-a[2], 0.0, 0.0, 0.0],
                  [c[1] - d[1] * c[0], 0.0, -d[1], 1.0],
                  [c[2] - d[2] * c[0], 0.0, -d[2], 0.0]])
    return A, np.array([c[0], 0.0, 1.0, 0.0])


def chunk_tables(fs, L):
    """(AL [4, 4], R [4, L]) for chunks of L samples: AL = A^L carries a chunk's start state to its contribution to the end state,
    end = e0 + AL @ start; R[j][k] is the cascade's output at sample k of a chunk with zero input started from the unit state e_j, so
    the chunk's output is its zero-state output + start @ R."""
    L = int(L)
    if L < 1:
        raise ValueError(f"chunk length must be positive, got {L}")
    A, C = state_matrix(fs)
    R = np.empty((4, L))
    M = np.eye(4)
    for k in range(L):
        R[:, k] = C @ M
        M = A @ M
    return M, R


def gain_rule(loud, peak, target=-23.0, ceiling_db=-1.0):
    """The gain rule on the host, for one utterance or arrays: -> (g, limited, fallback)."""
    loud, peak = np.asarray(loud, dtype=np.float64), np.asarray(peak, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cap = np.where(peak > 0, 10.0 ** (ceiling_db / 20.0) / peak, 0.0)
        fallback = ~np.isfinite(loud)
        g = np.where(fallback, cap, 10.0 ** ((target - np.where(fallback, 0.0, loud)) / 20.0))
    limited = ~fallback & (g > cap)
    return np.where(limited, cap, g), limited, fallback


def check_options(target_lufs=-23.0, ceiling_db=-1.0):
    if not -70.0 <= float(target_lufs) <= 0.0:                                # also refuses NaN
        raise ValueError(f"target_lufs must lie in [-70, 0], got {target_lufs!r}")
    if not float(ceiling_db) <= 0.0:
        raise ValueError(f"ceiling_db must be at most 0 dBFS, got {ceiling_db!r}")


# ------------------------------------------------------------------------------------------------ device
_tables = {}


def _device_tables(dev, fs):
    """(coef host [10], pw device [8][16], L, n, h) per (device, rate): pw[d] = A^(L 2^d)"""
    key = (str(dev), fs)
    if key not in _tables:
        lib = _lib.load()
        L, T = lib.fs2_kweight_chunk(), lib.fs2_kweight_chunks_per_tile()
        n, h = block_sizes(fs)
        if not L <= h <= L * T:
            raise ValueError(f"{fs} Hz: hops of {h} samples are outside what the kernel takes ({L} .. {L * T})")
        (b, a), (c, d) = k_weighting(fs)
        coef = np.ascontiguousarray(np.concatenate([b, a[1:], c, d[1:]]))
        M = chunk_tables(fs, L)[0]
        pw = []
        while len(pw) <= int(math.log2(T)):
            pw.append(M)
            M = M @ M
        assert 1 << (len(pw) - 1) == T
        _tables[key] = (coef, torch.from_numpy(np.stack(pw).reshape(len(pw), 16)).to(dev), L, n, h)
    return _tables[key]


def _vec(t, B, dtype, dev, what):
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or t.dim() != 1 or t.numel() != B:
        raise ValueError(f"{what} must be a ({B},) {dtype} tensor on {dev}")
    return t.contiguous()


def block_energy(y, lens, fs):
    """K-weighted block energies of a ragged batch: y (B, N) float32 on the GPU, row b holding lens[b] samples at rate fs ->
    (z (B, max blocks) fp64, n_blocks (B,) int32), both on the device; z[b, n_blocks[b]:] is unspecified."""
    fs = _rate(fs)
    y, lens_h, lens_d = ragged.rows(y, lens, "fastspeech2_amd.loudness.block_energy")
    B, N = y.shape
    coef, pw, L, n, h = _device_tables(y.device, fs)
    max_blocks = (N - n) // h + 1 if N >= n else 0
    z = torch.empty(B, max_blocks, dtype=torch.float64, device=y.device)
    nb = torch.empty(B, dtype=torch.int32, device=y.device)
    lib = _lib.load()
    need = lib.fs2_kweight_energy_ws(B, N, h)
    if need < 0:
        raise ValueError(f"a batch of {B} x {N} samples is too large for one call")
    ws = torch.empty(need if max_blocks else 0, dtype=torch.float64, device=y.device)
    _lib.call("fs2_kweight_energy", y.data_ptr(), N, lens_d.data_ptr(), coef.ctypes.data, pw.data_ptr(), L, n, h,
              z.data_ptr() if max_blocks else None, max_blocks, nb.data_ptr(), ws.data_ptr() if max_blocks else None, ws.numel(), B, N,
              ops._stream())
    return z, nb


def integrated(z, n_blocks):
    """Gated loudness per utterance: z (B, M) fp64 and n_blocks (B,) int32 on the GPU -> (B, 5) fp64 on the device, columns
    integrated loudness (LKFS), momentary maximum, n_blocks, blocks above the absolute gate, blocks above both gates."""
    ragged.require_device(z, "fastspeech2_amd.loudness.integrated")
    if z.dim() != 2 or z.dtype != torch.float64:
        raise ValueError(f"integrated: expected a (B, M) float64 tensor, got {tuple(z.shape)} {z.dtype}")
    z = z.contiguous()
    B, M = z.shape
    nb = _vec(n_blocks, B, torch.int32, z.device, "n_blocks")
    out = torch.empty(B, 5, dtype=torch.float64, device=z.device)
    _lib.call("fs2_gated_loudness", z.data_ptr() if M else None, M, nb.data_ptr(), out.data_ptr(), B, M, ops._stream())
    return out


def gain(loud, peak, target=-23.0, ceiling_db=-1.0):
    """The gain rule on the device: loud (B,) fp64 (or the (B, 5) result of `integrated`, whose first column is used), peak (B,)
    float32 -> (g (B,) fp64, flags (B,) int32: bit 0 limited, bit 1 fallback)."""
    check_options(target, ceiling_db)
    ragged.require_device(loud, "fastspeech2_amd.loudness.gain")
    if loud.dtype != torch.float64 or loud.dim() not in (1, 2) or not loud.is_contiguous():
        raise ValueError("loud must be a contiguous float64 tensor, (B,) or (B, 5)")
    B = loud.shape[0]
    ld = 1 if loud.dim() == 1 else loud.shape[1]
    peak = _vec(peak, B, torch.float32, loud.device, "peak")
    g = torch.empty(B, dtype=torch.float64, device=loud.device)
    flags = torch.empty(B, dtype=torch.int32, device=loud.device)
    _lib.call("fs2_loudness_gain", loud.data_ptr(), ld, peak.data_ptr(), float(target), float(ceiling_db), g.data_ptr(), flags.data_ptr(),
              B, ops._stream())
    return g, flags


def gain_pcm(y, lens, g, out=None):
    """int16(rint(y g 32768)) saturated, per row: -> (pcm (B, N) int16, zero beyond lens[b]; saturated (B,) int32), on the device.
    `out`: a contiguous (B, N) int16 device tensor to write into."""
    y, _, lens_d = ragged.rows(y, lens, "fastspeech2_amd.loudness.gain_pcm")
    B, N = y.shape
    g = _vec(g, B, torch.float64, y.device, "g")
    if out is None:
        out = torch.empty(B, N, dtype=torch.int16, device=y.device)
    elif out.dtype != torch.int16 or out.shape != y.shape or out.device != y.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous (B, N) int16 tensor on y's device")
    sat = torch.empty(B, dtype=torch.int32, device=y.device)
    _lib.call("fs2_gain_pcm", y.data_ptr(), N, lens_d.data_ptr(), g.data_ptr(), out.data_ptr(), N, sat.data_ptr(), B, N, ops._stream())
    return out, sat


def _db(x):
    return 20.0 * math.log10(x) if x > 0 else -math.inf


def measure(y, lens, fs, true_peak=False):
    """Per utterance a dict: lufs, momentary_max, sample_peak_dbfs, n_blocks, gated_abs, gated_rel; with true_peak=True also
    true_peak_dbtp (see the module docstring for what that number is)."""
    from . import resample as R
    z, nb = block_energy(y, lens, fs)
    cols = [integrated(z, nb), R.peak_abs(y, lens).double().unsqueeze(1)]
    if true_peak:
        y4, lens4 = R.resample_poly(y, lens, fs, 4 * _rate(fs))
        cols.append(R.peak_abs(y4, lens4).double().unsqueeze(1))
    rows = torch.cat(cols, dim=1).cpu().tolist()                             # one D2H copy
    out = []
    for r in rows:
        d = {"lufs": r[0], "momentary_max": r[1], "sample_peak_dbfs": _db(r[5]), "n_blocks": int(r[2]), "gated_abs": int(r[3]),
             "gated_rel": int(r[4])}
        if true_peak:
            d["true_peak_dbtp"] = _db(r[6])
        out.append(d)
    return out
