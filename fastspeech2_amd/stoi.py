"""Time-aligned intelligibility scores on the GPU (csrc/fs2_stoi.hip): the short-time objective intelligibility measure STOI (Taal,
Hendriks, Heusdens, Jensen 2011) and its extended form ESTOI (Jensen and Taal 2016) of a clean signal x and a processed signal y
that share a time axis, over ragged batches of pairs.  They are defined only where the two signals are sample-aligned: copy
synthesis (copysynth.py: a recorded mel through the vocoder) is, synthesis from predicted durations is not.  The specification
below is what the kernels and the independent numpy restatement (tests/stoi_ref.py) implement.  Everything after the float32 load
is fp64; no atomics, every sum in a fixed order, a second run gives the same bytes.

Constants, the papers': fs = 10 000, frame N = 256, hop H = 128, transform K = 512, J = 15 bands, lowest centre 150 Hz, segments of
L = 30 frames, beta = -15 dB, dynamic range 40 dB.  EPS = 2^-52.

Rate.  Both signals are cut to the shorter length, then resampled to 10 kHz with this project's `resample.resample_poly`
(`resample.ratio(sr, 10000)`); at 10 kHz nothing is resampled.

Window.  w[n] = 0.5 (1 - cos(2 pi (n + 1) / 257)), n = 0 .. 255: MATLAB's hanning(256), without zero end points (`window`).

Framing rule, used twice.  Frame starts s = 0, H, 2H, .. with s < len - N: n_frames = ceil((len - N) / H) for len > N, 0 otherwise
(`n_frames`).

Silent-frame removal (the clean signal decides, both are cut).  e_j = sum_n (x[s_j + n] w[n])^2.  Frame j is kept iff e_max > 0
and e_j > 1e-4 e_max: the papers' 40 dB rule without the logarithm.  The kept frames j_0 < j_1 < .. are overlap-added at hop H:
x'[i H + n] += x[s_{j_i} + n] w[n], the same for y; len' = (n_kept - 1) H + N, or 0 when nothing is kept.  The kernel writes it as a
gather: every output sample reads the at most two kept frames that cover it through the compaction map, lower frame first.

Spectrum.  x' and y' are framed by the same rule, which gives M = n_kept - 1 frames; each is windowed with w, zero-padded to 512
and transformed; the power |.|^2 of the bins the bands use is formed.  The kernel evaluates the DFT directly against a table of
cos / sin(2 pi j / 512) built on the host (`twiddle`): the device evaluates no sine.

Bands.  f_b = b 10000 / 512.  For k = 0 .. 14: lo_k = 150 2^((2 k - 1) / 6), hi_k = 150 2^((2 k + 1) / 6); band k sums the bins
[argmin_b |f_b - lo_k|, argmin_b |f_b - hi_k|), the first minimum; X[k, m] = sqrt(sum of the power), Y likewise (`band_edges`).
Band 0 starts at bin 7, band 14 ends before bin 219, and band k + 1 starts where band k ends.

STOI.  For every segment of 30 consecutive frames (M - 29 segments) and every band: alpha = |X_seg| / (|Y_seg| + EPS),
Y' = min(alpha Y_seg, (1 + 10^(15 / 20)) X_seg); each of X_seg and Y' has its mean over the 30 frames subtracted and is divided by
(its norm + EPS); d = their dot product.  STOI is the mean of d over all bands and segments.

ESTOI.  Per segment, on the 15 x 30 blocks of X and Y: subtract each row's mean and divide it by (its norm + EPS), then subtract
each column's mean and divide it by (its norm + EPS); d = sum (X~ o Y~) / 30.  ESTOI is the mean of d over the segments.

Too short.  With M < 30 there is no segment: both scores are NaN and the row is flagged `too_short` (no small sentinel value).

What is claimed: the published algorithms as written above, held against the restatement and against known answers (a signal
against itself, its negative and its double scores 1; added noise lowers both scores monotonically; silence common to both
signals changes nothing).  Not claimed: agreement with pystoi or the authors' MATLAB code, neither of which can be run here;
anything about the resampler, which is this project's and not MATLAB's `resample`; any measurement on real speech.
"""
import numpy as np
import torch

from . import _lib, ops, ragged

WHO = "fastspeech2_amd.stoi"
FS, N, H, K, J, L = 10000, 256, 128, 512, 15, 30
F_LOW = 150.0
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)                        # beta = -15 dB
EPS = 2.0 ** -52
RANGE = 1e-4                                              # 40 dB, as an energy ratio
BYTES_PER_SAMPLE = 96                                     # a pair on the device: two float32 rows at each rate, two fp64 rows, bands


# ------------------------------------------------------------------------------------------------ host, fp64
def window():
    """w [256] fp64: MATLAB's hanning(256)."""
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, N + 1, dtype=np.float64) / (N + 1)))


def n_frames(length):
    """frames of `length` samples under the framing rule"""
    length = int(length)
    return -(-(length - N) // H) if length > N else 0


def band_centres():
    return F_LOW * 2.0 ** (np.arange(J, dtype=np.float64) / 3.0)


def band_edges():
    """(lo [15], hi [15]) int: band k sums the bins [lo[k], hi[k])."""
    f = np.arange(K // 2 + 1, dtype=np.float64) * FS / K
    k = np.arange(J, dtype=np.float64)
    lo = np.array([int(np.argmin(np.abs(f - v))) for v in F_LOW * 2.0 ** ((2.0 * k - 1.0) / 6.0)])
    hi = np.array([int(np.argmin(np.abs(f - v))) for v in F_LOW * 2.0 ** ((2.0 * k + 1.0) / 6.0)])
    return lo, hi


def twiddle():
    """[512][2] fp64: cos and sin of 2 pi j / 512."""
    a = 2.0 * np.pi * np.arange(K, dtype=np.float64) / K
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


# ------------------------------------------------------------------------------------------------ device
_tables = {}


def _device_tables(dev):
    """(window, twiddle on the device, the 16 band edges on the host) per device"""
    key = str(dev)
    if key not in _tables:
        lo, hi = band_edges()
        if not np.array_equal(lo[1:], hi[:-1]):
            raise AssertionError("the one-third octave bands are not contiguous")
        edges = np.ascontiguousarray(np.concatenate([lo, hi[-1:]]).astype(np.int32))
        _tables[key] = (torch.from_numpy(window()).to(dev), torch.from_numpy(twiddle()).to(dev), edges)
    return _tables[key]


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _vec(t, B, dev, what):
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != B:
        raise ValueError(f"{what} must be a ({B},) int32 tensor on {dev}")
    return t.contiguous()


def _mat(t, dtype, dim, what):
    ragged.require_device(t, WHO)
    if t.dtype != dtype or t.dim() != dim:
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _rows(x, lens, who):
    x, lens_h, lens_d = ragged.rows(x, lens, who)
    if x.shape[1] == 0:                                                      # rows without a sample still need an address
        x = x.new_zeros(x.shape[0], 1)
    return x, lens_h, lens_d


def frame_energy(x, lens):
    """Windowed frame energies of the clean rows: x (B, N) float32 on the GPU at 10 kHz -> e (B, n_frames(max lens)) fp64;
    e[b, n_frames(lens[b]):] is unspecified."""
    x, lens_h, lens_d = _rows(x, lens, WHO + ".frame_energy")
    B, Nmax = x.shape[0], max(lens_h, default=0)
    w, _, _ = _device_tables(x.device)
    e = torch.empty(B, n_frames(Nmax), dtype=torch.float64, device=x.device)
    _lib.call("fs2_stoi_frame_energy", x.data_ptr(), x.shape[1], lens_d.data_ptr(), w.data_ptr(), _ptr(e), e.shape[1], B, Nmax,
              ops._stream())
    return e


def keep(e, lens):
    """e (B, >= n_frames(max lens)) fp64 -> (mask (B, F) int32, map (B, F) int32, n_kept (B,) int32): the kept frames of each row
    and the frame that becomes frame i; entries beyond a row's frames / kept frames are unspecified."""
    e = _mat(e, torch.float64, 2, "e")
    B = e.shape[0]
    lens_h, lens_d = ragged.lengths(lens, B, (1 << 31) - 1, "lens", e.device)
    Nmax = max(lens_h, default=0)
    F = n_frames(Nmax)
    if e.shape[1] < F:
        raise ValueError(f"e {tuple(e.shape)} does not hold the {F} frames of {Nmax} samples")
    mask = torch.empty(B, F, dtype=torch.int32, device=e.device)
    cmap = torch.empty(B, F, dtype=torch.int32, device=e.device)
    n_kept = torch.empty(B, dtype=torch.int32, device=e.device)
    _lib.call("fs2_stoi_keep", _ptr(e), e.shape[1], lens_d.data_ptr(), _ptr(mask), _ptr(cmap), F, n_kept.data_ptr(), B, Nmax,
              ops._stream())
    return mask, cmap, n_kept


def overlap_add(x, y, lens, cmap, n_kept):
    """The kept frames of both signals, windowed and overlap-added at hop 128: x, y (B, N) float32 sharing `lens`, the map and counts
    of `keep` -> (x', y') (B, (F - 1) 128 + 256) fp64, row b holding (n_kept[b] - 1) 128 + 256 samples (none when nothing is kept)."""
    x, lens_h, lens_d = _rows(x, lens, WHO + ".overlap_add")
    y, _, _ = _rows(y, lens, WHO + ".overlap_add")
    if y.shape != x.shape:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have one shape")
    B, Nmax = x.shape[0], max(lens_h, default=0)
    F = n_frames(Nmax)
    cmap, n_kept = _mat(cmap, torch.int32, 2, "map"), _vec(n_kept, B, x.device, "n_kept")
    if cmap.shape[0] != B or cmap.shape[1] < F:
        raise ValueError(f"map {tuple(cmap.shape)} does not hold {B} rows of {F} frames")
    w, _, _ = _device_tables(x.device)
    Lmax = (F - 1) * H + N if F else 0
    xo = torch.empty(B, Lmax, dtype=torch.float64, device=x.device)
    yo = torch.empty(B, Lmax, dtype=torch.float64, device=x.device)
    _lib.call("fs2_stoi_ola", x.data_ptr(), y.data_ptr(), x.shape[1], lens_d.data_ptr(), w.data_ptr(), _ptr(cmap), cmap.shape[1],
              n_kept.data_ptr(), _ptr(xo), _ptr(yo), Lmax, B, Nmax, ops._stream())
    return xo, yo


def band_magnitudes(xo, n_kept):
    """One-third octave band magnitudes of the frames of a compacted signal: xo (B, (F - 1) 128 + 256) fp64 as `overlap_add` returns
    it -> X (B, 15, F - 1) fp64, row b holding n_kept[b] - 1 frames."""
    xo = _mat(xo, torch.float64, 2, "xo")
    B = xo.shape[0]
    F = (xo.shape[1] - N) // H + 1 if xo.shape[1] >= N else 0
    n_kept = _vec(n_kept, B, xo.device, "n_kept")
    w, tw, edges = _device_tables(xo.device)
    M = max(F - 1, 0)
    X = torch.empty(B, J, M, dtype=torch.float64, device=xo.device)
    _lib.call("fs2_stoi_bands", _ptr(xo), xo.shape[1], n_kept.data_ptr(), w.data_ptr(), tw.data_ptr(), edges.ctypes.data, _ptr(X), J * M,
              M, B, F, ops._stream())
    return X


def segment_scores(X, Y, n_kept):
    """X, Y (B, 15, M) fp64 as `band_magnitudes` returns them -> seg (B, 2, max(M - 29, 0)) fp64: per segment the STOI correlation
    averaged over the bands and the ESTOI score; row b holds max(n_kept[b] - 30, 0) segments."""
    X, Y = _mat(X, torch.float64, 3, "X"), _mat(Y, torch.float64, 3, "Y")
    if X.shape != Y.shape or X.shape[1] != J:
        raise ValueError(f"X {tuple(X.shape)} and Y {tuple(Y.shape)} must both be (B, {J}, M)")
    B, M = X.shape[0], X.shape[2]
    n_kept = _vec(n_kept, B, X.device, "n_kept")
    S = max(M - L + 1, 0)
    seg = torch.empty(B, 2, S, dtype=torch.float64, device=X.device)
    _lib.call("fs2_stoi_segments", _ptr(X), _ptr(Y), J * M, M, n_kept.data_ptr(), CLIP, _ptr(seg), 2 * S, S, B, M + 1 if M else 0,
              ops._stream())
    return seg


def row_scores(seg, lens, n_kept):
    """seg (B, 2, S) of `segment_scores`, the rows' lengths at 10 kHz and kept-frame counts -> (B, 6) fp64 on the device: STOI,
    ESTOI, frames, kept frames, segments, too short (1 or 0)."""
    seg = _mat(seg, torch.float64, 3, "seg")
    B, S = seg.shape[0], seg.shape[2]
    if seg.shape[1] != 2:
        raise ValueError(f"seg {tuple(seg.shape)} must be (B, 2, S)")
    lens_h, lens_d = ragged.lengths(lens, B, (1 << 31) - 1, "lens", seg.device)
    Nmax = max(lens_h, default=0)
    if max(n_frames(Nmax) - L, 0) > S:
        raise ValueError(f"seg {tuple(seg.shape)} does not hold the segments of {Nmax} samples")
    n_kept = _vec(n_kept, B, seg.device, "n_kept")
    out = torch.empty(B, 6, dtype=torch.float64, device=seg.device)
    _lib.call("fs2_stoi_mean", _ptr(seg), 2 * S, S, lens_d.data_ptr(), n_kept.data_ptr(), out.data_ptr(), B, Nmax, ops._stream())
    return out


def to_10k(ref, ref_lens, syn, syn_lens, sr):
    """Both sides cut to the shorter length and brought to 10 kHz: -> (x, y (B, N) float32 of one shape, lens on the host)."""
    from . import resample as R
    sr = int(sr)
    ref, rl, _ = ragged.rows(ref, ref_lens, WHO, device_lens=False)
    syn, sl, _ = ragged.rows(syn, syn_lens, WHO, device_lens=False)
    if ref.shape[0] != syn.shape[0] or ref.device != syn.device:
        raise ValueError(f"ref {tuple(ref.shape)} and syn {tuple(syn.shape)} are not B pairs on one device")
    lens = [min(a, b) for a, b in zip(rl, sl)]
    if sr == FS:
        n = max(lens, default=0)
        return ref[:, :n].contiguous(), syn[:, :n].contiguous(), lens
    x, xl = R.resample_poly(ref, lens, sr, FS)
    y, _ = R.resample_poly(syn, lens, sr, FS)
    return x, y, [int(v) for v in xl.tolist()]


def stages(x, y, lens):
    """Every stage of a batch at 10 kHz, for tests and `measure`: a dict of the device tensors e, mask, map, n_kept, xo, yo, X, Y,
    seg and out."""
    e = frame_energy(x, lens)
    mask, cmap, n_kept = keep(e, lens)
    xo, yo = overlap_add(x, y, lens, cmap, n_kept)
    X, Y = band_magnitudes(xo, n_kept), band_magnitudes(yo, n_kept)
    seg = segment_scores(X, Y, n_kept)
    return {"e": e, "mask": mask, "map": cmap, "n_kept": n_kept, "xo": xo, "yo": yo, "X": X, "Y": Y, "seg": seg,
            "out": row_scores(seg, lens, n_kept)}


def measure(ref, ref_lens, syn, syn_lens, sr):
    """STOI and ESTOI of B time-aligned pairs: ref (clean) and syn (B, N) float32 on the GPU at rate `sr`, row b holding ref_lens[b]
    and syn_lens[b] samples -> a dict of (B,) device tensors: stoi, estoi (fp64, NaN when too short), frames, frames_kept, segments
    (int32) and too_short (bool)."""
    x, y, lens = to_10k(ref, ref_lens, syn, syn_lens, sr)
    out = stages(x, y, lens)["out"]
    return {"stoi": out[:, 0], "estoi": out[:, 1], "frames": out[:, 2].to(torch.int32), "frames_kept": out[:, 3].to(torch.int32),
            "segments": out[:, 4].to(torch.int32), "too_short": out[:, 5] != 0}


# ------------------------------------------------------------------------------------------------ the corpus pass
def score_pairs(ref_wavs, syn_wavs, sampling_rate, device="cuda", budget=1 << 30):
    """(recorded, copy-synthesized) pairs of float32 waveforms at `sampling_rate`, each cut to its shorter side -> one dict per pair,
    in the order given: stoi, estoi, stoi_frames_kept, stoi_segments, aligned_samples.  Pairs are packed longest first into ragged
    batches under `budget` bytes of device buffers, both sides through one pinned staging buffer, one D2H copy of the scores per
    batch."""
    if len(ref_wavs) != len(syn_wavs):
        raise ValueError(f"{len(ref_wavs)} reference and {len(syn_wavs)} synthesized waveforms")
    dev = ragged.require_device(torch.device(device), WHO)
    n = [min(len(r), len(s)) for r, s in zip(ref_wavs, syn_wavs)]
    staging = ragged.Staging()
    rows = [None] * len(n)
    for batch in ragged.greedy_batches([(v,) for v in n], budget, lambda k, top: k * top * BYTES_PER_SAMPLE):
        lens = [n[i] for i in batch]
        staging.pack([ref_wavs[i][:n[i]] for i in batch])
        x = staging.to(dev)
        staging.pack([syn_wavs[i][:n[i]] for i in batch])
        y = staging.to(dev)
        x, y, lens10 = to_10k(x, lens, y, lens, sampling_rate)
        host = stages(x, y, lens10)["out"].cpu().numpy()                    # the batch's one D2H copy
        for r, i in enumerate(batch):
            rows[i] = {"stoi": float(host[r, 0]), "estoi": float(host[r, 1]), "stoi_frames_kept": int(host[r, 3]),
                       "stoi_segments": int(host[r, 4]), "aligned_samples": n[i]}
    return rows


def summarize(rows):
    """Corpus means of stoi and estoi over the rows that are not too short, and the number of rows that are."""
    ok = [r for r in rows if r["stoi_segments"] > 0]
    nan = float("nan")
    return {"stoi_mean": float(np.mean([r["stoi"] for r in ok])) if ok else nan,
            "estoi_mean": float(np.mean([r["estoi"] for r in ok])) if ok else nan,
            "stoi_too_short_utterances": len(rows) - len(ok)}
