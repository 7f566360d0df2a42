"""F0 extraction on the GPU: WORLD's DIO estimator followed by StoneMask refinement (reference preprocessor/preprocessor.py:182-187
calls pyworld's `dio` + `stonemask`), as HIP kernels in fp64 over ragged batches (csrc/fs2_f0.hip).

Written from the published description of DIO (Morise, Kawahara, Katayose 2009) and of WORLD (Morise, Yokomori, Ozawa 2016).
The specification below is what the kernels and the numpy oracle (tests/f0_ref.py) implement; it is not claimed to equal
pyworld's output.  Defaults are the reference's: f0_floor 71, f0_ceil 800, channels_in_octave 2, speed 1 (no decimation),
allowed_range 0.1, frame_period = hop / fs * 1000 ms.  0 marks an unvoiced frame.

Frames.  F = 1 + int(N / fs / (frame_period / 1000)) for a row of N samples, in double as written; frame f is at
t_f = f * frame_period / 1000 s.

DIO
  1. DC.  The row is extended by one zero sample (N + 1 samples).  mean = sum / (N + 1) over those samples;
     y[n] = x[n] - mean for n <= N (so y[N] = -mean), y = 0 outside [0, N].  tau = 1e-9 * max_{n <= N} |y[n]|.
  2. Low-cut.  R = round(fs / 50) (round half away from zero); Hann w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / (2R + 2)), j < 2R + 1;
     zero-phase taps g[k] = delta[k] - w[k + R] / sum(w), k in [-R, R]; lc = y * g, the full linear convolution (lc[m] for
     every integer m, non-zero on [-R, N + R]).
  3. Bands.  nb = 1 + int(log(f0_ceil / f0_floor) / log 2 * channels_in_octave); boundary b_j = f0_floor 2^((j + 1) / ch).
     h_j = round(fs / b_j / 2); Nuttall v[k] = 0.355768 - 0.487396 cos(2 pi k / (4h - 1)) + 0.144232 cos(4 pi k / (4h - 1))
     - 0.012604 cos(6 pi k / (4h - 1)), k < 4h, normalised to sum 1; band signal s[i] = sum_k v[k] lc[i + 2h - k] for
     i in [0, N] (the 2h-sample delay compensated).  s~[i] = s[i] if |s[i]| > tau else 0 (digital silence and rounding
     residue carry no events); d[i] = s~[i + 1] - s~[i], i < N.
  4. Events.  For u in (s~, -s~) on i < N and (d, -d) on i < N - 1 (negative-going, positive-going, peak, dip): an event at
     i when u[i] > 0 and u[i + 1] <= 0, at position e = (i + 1) - u[i] / (u[i + 1] - u[i]).  Consecutive events give
     intervals with location (e_k + e_{k+1}) / 2 / fs and F0 fs / (e_{k+1} - e_k).
  5. Candidates.  A band has a candidate at t_f only when each of its four streams has >= 3 intervals, t_f lies within
     [first, last] interval location of each stream (no extrapolation), and the two intervals bracketing t_f (k = number of
     locations <= t_f, clamped to [1, n - 1]; intervals k - 1 and k) both have F0 >= f0_floor (no interpolation across a gap).
     Each stream's value is the linear interpolation between those two; the candidate c is the mean of the four values, the
     score their sample standard deviation (divisor 3).  c is rejected (c = 0, score = 1e5) when c > b_j, c < b_j / 2,
     c > f0_ceil or c < f0_floor.  Normalised score = score / (c + 1e-12).
  6. Best band per frame: the lowest normalised score (first band on ties).
  7. Fixing, vrm = int(0.5 + 1000 / frame_period / f0_floor) * 2 + 1; all frames 0 when F <= vrm.
     step 1: base = best with the first and last vrm frames set to 0; f1[i] = 0 for i < vrm, else base[i] when
             |(base[i] - base[i-1]) / (1e-12 + base[i])| < allowed_range, else 0.
     step 2: f2[i] = 0 when any f1[i + j], |j| <= (vrm - 1) / 2, is 0 (for i in [(vrm-1)/2, F - (vrm-1)/2)), else f1[i].
     step 3: for each voiced run of f2 in time order, from its last frame j up to (excluding) the next run's last frame (or
             F - 1): f3[j + 1] = select(f3[j], f3[j - 1], j + 1), stop at the first 0.
     step 4: for each run in reverse order, from its first frame j down to (excluding) the previous run's first frame (or 1):
             f4[j - 1] = select(f4[j], f4[j + 1], j - 1), stop at the first 0.
     select(cur, past, i): r = (3 cur - past) / 2; the band candidate at frame i closest to r (first on ties); 0 when
             |1 - best / r| > allowed_range.

StoneMask (per frame with 40 < f0 <= fs / 12, else 0), on the DC-intact x[0, N)
  hw = int(1.5 fs / f0 + 1); for n in [0, 2 hw]: r_n = round((t_f + (n - hw) / fs) fs), sample x[clamp(r_n - 1, 0, N - 1)]
  (the row's own bounds); Blackman w_n = 0.42 + 0.5 cos(2 pi tm / T) + 0.08 cos(4 pi tm / T), tm = (r_n - 1) / fs - t_f,
  T = (2 hw + 1) / fs; derivative window dw_0 = -w_1 / 2, dw_n = -(w_{n+1} - w_{n-1}) / 2, dw_2hw = w_{2hw-1} / 2.
  L = 4 * 2^floor(log2(2 hw + 1)); M, D = DFTs of length L (X[k] = sum_n v_n exp(-2 pi i k n / L)) of x w and x dw, evaluated
  only at the bins needed.  IF(f, H) = sum_{h<=H} a_h IF_h / (sum_{h<=H} a_h h + 1e-12), with k_h = round(f L / fs h),
  a_h = |M[k_h]|, IF_h = k_h fs / L + (Re M Im D - Im M Re D) / |M|^2 fs / (2 pi) (0 when |M| = 0).
  f' = IF(f0, 2); f'' = 0 if f' <= 0 or f' > 2 f0, else IF(f', 6); the result is f'' unless |f'' - f0| > 0.2 f0, then f0.
"""
import math

import numpy as np
import torch

from . import _lib, ops, ragged

F0_FLOOR, F0_CEIL, CHANNELS_IN_OCTAVE, ALLOWED_RANGE = 71.0, 800.0, 2.0, 0.1


def matlab_round(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def frame_count(n, fs, frame_period):
    """DIO's frame count for n samples, in double exactly as written (where n % hop == 0 float rounding decides)."""
    return 1 + int(n / fs / (frame_period / 1000))


def bands(f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, channels_in_octave=CHANNELS_IN_OCTAVE):
    nb = 1 + int(math.log(f0_ceil / f0_floor) / 0.69314718055994529 * channels_in_octave)
    return [f0_floor * 2.0 ** ((i + 1) / channels_in_octave) for i in range(nb)]


def lowcut_taps(fs):
    R = matlab_round(fs / 50.0)
    L = 2 * R + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, L + 1) / (L + 1))
    g = -w / w.sum()
    g[R] += 1.0
    return g


def nuttall(L):
    tmp = np.arange(L) / (L - 1.0)
    w = 0.355768 - 0.487396 * np.cos(2.0 * np.pi * tmp) + 0.144232 * np.cos(4.0 * np.pi * tmp) - 0.012604 * np.cos(6.0 * np.pi * tmp)
    return w / w.sum()


def voice_range_minimum(frame_period, f0_floor=F0_FLOOR):
    return int(0.5 + 1000.0 / frame_period / f0_floor) * 2 + 1


_consts = {}


def _device_consts(dev, fs, f0_floor, f0_ceil, channels_in_octave):
    key = (str(dev), float(fs), float(f0_floor), float(f0_ceil), float(channels_in_octave))
    if key not in _consts:
        bf = bands(f0_floor, f0_ceil, channels_in_octave)
        hs = [matlab_round(fs / b / 2.0) for b in bf]
        if min(hs) < 1:
            raise ValueError(f"f0_ceil {f0_ceil} is too high for fs {fs}")
        nut = np.concatenate([nuttall(4 * h) for h in hs])
        taps = lowcut_taps(fs)
        _consts[key] = dict(taps=torch.tensor(taps, dtype=torch.float64, device=dev), R=(len(taps) - 1) // 2,
                            nut=torch.tensor(nut, dtype=torch.float64, device=dev),
                            band_h=torch.tensor(hs, dtype=torch.int32, device=dev),
                            band_f0=torch.tensor(bf, dtype=torch.float64, device=dev), nb=len(bf), max_h=max(hs))
    return _consts[key]


def _frames(lens_h, fs, frame_period, dev):
    frames_h = [frame_count(n, fs, frame_period) for n in lens_h]
    Fmax = max(frames_h) if frames_h else 0
    return frames_h, Fmax, torch.tensor(frames_h, dtype=torch.int32, device=dev)


def dio(y, lens, fs, frame_period, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, channels_in_octave=CHANNELS_IN_OCTAVE,
        allowed_range=ALLOWED_RANGE):
    """DIO over a ragged batch: y (B, N) float32 on the GPU, row b holds lens[b] samples.  Returns (f0 (B, Fmax) float64 on the
    device, t (Fmax,) float64, frames (B,) int64); f0[b, frames[b]:] = 0."""
    y, lens_h, lens_d = ragged.rows(y, lens, "fastspeech2_amd.pitch")
    dev, (B, N) = y.device, y.shape
    c = _device_consts(dev, fs, f0_floor, f0_ceil, channels_in_octave)
    frames_h, Fmax, frames_d = _frames(lens_h, fs, frame_period, dev)
    nb, H = c["nb"], 2 * c["max_h"]
    ldl = N + 2 * H + 1
    ntile = -(-N // 256)
    cap = N // 2 + 2
    st = ops._stream()
    stats = torch.empty(B, 2, dtype=torch.float64, device=dev)
    lc = torch.empty(B, ldl, dtype=torch.float64, device=dev)
    counts = torch.empty(B, nb, 4, max(ntile, 1), dtype=torch.int32, device=dev)
    offs = torch.empty_like(counts)
    totals = torch.empty(B, nb, 4, dtype=torch.int32, device=dev)
    events = torch.empty(B, nb, 4, cap, dtype=torch.float64, device=dev)
    cand = torch.empty(B, nb, Fmax, dtype=torch.float64, device=dev)
    score = torch.empty_like(cand)
    tmp = torch.empty(B, 2, Fmax, dtype=torch.float64, device=dev)
    f0 = torch.empty(B, Fmax, dtype=torch.float64, device=dev)
    _lib.call("fs2_f0_dc", y.data_ptr(), N, lens_d.data_ptr(), stats.data_ptr(), B, N, st)
    _lib.call("fs2_f0_lowcut", y.data_ptr(), N, lens_d.data_ptr(), stats.data_ptr(), c["taps"].data_ptr(), c["R"], lc.data_ptr(),
              ldl, H, B, N, st)
    for emit in (0, 1):
        _lib.call("fs2_f0_events", lc.data_ptr(), ldl, H, lens_d.data_ptr(), stats.data_ptr(), c["nut"].data_ptr(),
                  c["band_h"].data_ptr(), nb, c["max_h"], counts.data_ptr(), offs.data_ptr(), events.data_ptr(), cap, B, N, emit, st)
        if not emit:
            _lib.call("fs2_f0_scan", counts.data_ptr(), offs.data_ptr(), totals.data_ptr(), B, nb, N, st)
    _lib.call("fs2_f0_candidates", events.data_ptr(), cap, totals.data_ptr(), frames_d.data_ptr(), c["band_f0"].data_ptr(), nb,
              float(fs), float(frame_period), float(f0_floor), float(f0_ceil), cand.data_ptr(), score.data_ptr(), B, Fmax, st)
    _lib.call("fs2_f0_fix", cand.data_ptr(), score.data_ptr(), frames_d.data_ptr(), nb, voice_range_minimum(frame_period, f0_floor),
              float(allowed_range), tmp.data_ptr(), f0.data_ptr(), B, Fmax, st)
    t = np.arange(Fmax) * frame_period / 1000.0
    return f0, t, torch.tensor(frames_h, dtype=torch.int64)


def stonemask(y, lens, f0, frames, fs, frame_period):
    """StoneMask refinement of `f0` (B, Fmax) float64 (device) from the rows of y (B, N) float32 (device); frames (B,) as dio
    returns.  Returns a new (B, Fmax) float64 device tensor."""
    y, lens_h, lens_d = ragged.rows(y, lens, "fastspeech2_amd.pitch")
    if not isinstance(f0, torch.Tensor) or f0.device != y.device or f0.dtype != torch.float64 or f0.dim() != 2 \
            or f0.shape[0] != y.shape[0]:
        raise ValueError("f0 must be a (B, Fmax) float64 tensor on y's device")
    _, frames_d = ragged.lengths(frames, y.shape[0], f0.shape[1], "frames", y.device)
    f0 = f0.contiguous()
    B, Fmax = f0.shape
    out = torch.empty_like(f0)
    _lib.call("fs2_f0_stonemask", y.data_ptr(), y.shape[1], lens_d.data_ptr(), f0.data_ptr(), frames_d.data_ptr(), float(fs),
              float(frame_period), out.data_ptr(), B, Fmax, y.shape[1], ops._stream())
    return out


def dio_stonemask(y, lens, fs, frame_period, **dio_kw):
    """Both stages on the device, one D2H copy at the end: (f0 (B, Fmax) float64 numpy, t (Fmax,), frames (B,) int64 numpy)."""
    f0, t, frames = dio(y, lens, fs, frame_period, **dio_kw)
    f0 = stonemask(y, lens, f0, frames, fs, frame_period)
    return f0.cpu().numpy(), t, frames.numpy()


def pitch_fn(device="cuda"):
    """`pitch_fn(wav, sampling_rate, hop_length) -> f0` (numpy in, float64 numpy out, one value per DIO frame), the signature
    `Preprocessor(pitch_fn=...)` takes, computed on `device`."""
    dev = torch.device(device)

    def fn(wav, sampling_rate, hop_length):
        w = torch.as_tensor(np.ascontiguousarray(wav, dtype=np.float32)).reshape(1, -1).to(dev)
        f0, _, frames = dio_stonemask(w, [w.shape[1]], sampling_rate, hop_length / sampling_rate * 1000)
        return f0[0, :frames[0]]
    return fn
