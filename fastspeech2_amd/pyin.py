"""F0 extraction on the GPU by probabilistic YIN, a second estimator beside DIO + StoneMask (`pitch`), as HIP kernels in fp64 over
ragged batches (csrc/fs2_pyin.hip).

Written from the published description of YIN (de Cheveigne, Kawahara 2002) and of pYIN (Mauch, Dixon, ICASSP 2014).  The
specification below is what the kernels and the numpy oracle (tests/pyin_ref.py) implement; it is the published algorithm with the
paper's first-trough rule, and it is not claimed to equal `librosa.pyin`, which is not available here: that agreement is unmeasured.
Defaults: fmin 71, fmax 800 (`pitch.F0_FLOOR`, `pitch.F0_CEIL`), frame_length L = 2048, integration window W = L / 2, 100
thresholds, Beta(2, 18) threshold prior, no_trough_prob 0.01, 20 bins per semitone (bo = 240 bins per octave), max_transition_rate
35.92 octaves / s, switch_prob 0.01.  0 marks an unvoiced frame.  round(v) below is floor(v + 0.5): halves go up.

Frames.  hop = round(frame_period / 1000 fs) samples (>= 1).  F = pitch.frame_count(N, fs, frame_period) for a row of N samples, so
  the track drops in wherever DIO's does; frame f is centred at sample f hop, t_f = f frame_period / 1000 s, and covers the samples
  s0 .. s0 + L - 1 with s0 = f hop - L / 2.  x[n] = 0 outside [0, N).
Difference function.  tau_max = min(ceil(fs / fmin), L - W - 1), tau_min = floor(fs / fmax); 1 <= tau_min < tau_max is required.
  d_f(tau) = sum_{j < W} (x[s0 + j] - x[s0 + j + tau])^2 for tau in [0, tau_max]: the direct form, the float32 samples widened to
  double, the terms added in double in the order of j.  (The energy-minus-autocorrelation identity is not used: it cancels.)
Cumulative-mean normalisation.  d'(0) = 1; d'(tau) = d(tau) tau / sum_{j = 1..tau} d(j); d'(tau) = 1 where that sum is 0.
Troughs, on tau in [tau_min, tau_max].  An interior tau is a trough when d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1); tau_min is
  one when d'(tau_min) < d'(tau_min + 1), tau_max when d'(tau_max) < d'(tau_max - 1).  (No two troughs are neighbours.)  The height
  of a trough is d'(tau) itself.  shift(tau) = (a - c) / (2 (a - 2 b + c)) with a, b, c = d'(tau - 1), d'(tau), d'(tau + 1) for an
  interior tau with a - 2 b + c > 0; 0 at tau_min, at tau_max and for a degenerate parabola.  |shift| <= 1 / 2 at a trough.
Candidates.  s_k = k / K (in double), k = 1..K, K = 100; beta_k = I(s_k) - I(s_{k-1}), I the Beta(a, b) distribution function, for
  integer a, b: I(x) = sum_{j = a}^{a + b - 1} C(a + b - 1, j) x^j (1 - x)^(a + b - 1 - j)  (1 - (1 - x)^18 (1 + 18 x) for Beta(2, 18)).
  For each k the trough with the smallest tau whose height is < s_k receives beta_k; when no trough is below s_k, the global minimum
  of d' on [tau_min, tau_max] (the smallest tau on ties) receives no_trough_prob beta_k.  A frame whose d' is the same at every
  lag of [tau_min, tau_max] (digital silence or any constant signal: d = 0, so d' = 1 throughout) has no minimum, only a tie: it has
  no candidate, no mass is given, its voiced entries are 0 and p_v = 0.  (Without this rule the tie-break would put 0.01 on the bin
  of tau_min, which outweighs (1 - 0.01) / nb per unvoiced state: exact zeros longer than about 0.5 s would decode as voiced at
  the top bin.)  As the first trough below s_k moves to smaller tau when k grows, trough i (in lag order, height h_i) receives the
  k with h_i < s_k and not (min_{j < i} h_j < s_k).
  A candidate at tau has frequency fs / (tau + shift(tau)) and pitch bin clip(round(bo log2(frequency / fmin)), 0, nb - 1),
  nb = floor(bo log2(fmax / fmin)) + 1 (839).  The bin does not grow with tau, so the troughs of one bin are neighbours.
Observation row, 2 nb values.  Mass m_i of trough i: its beta_k added in the order of k; mass g of the global minimum likewise.
  voiced[bin] = the m_i of that bin added in lag order, g added last to its own bin; S = the m_i added in lag order, then g;
  p_v = min(S, 1); every one of the nb unvoiced entries is (1 - p_v) / nb.  p_v is returned as the voiced probability.
HMM.  State s = v nb + bin, v = 0 voiced, v = 1 unvoiced; initial distribution 1 / (2 nb).  h = round(max_transition_rate 12 hop / fs)
  (bins_per_semitone / 2) bins (50 at hop 256, 22 050 Hz; bins_per_semitone must be even).  w(delta) = h + 1 - |delta| for
  |delta| <= h, else 0; Z_i = sum of w(j - i) over the bins j in [0, nb): the window is renormalised at the edges of the bin range.
  P((i, v) -> (j, v')) = w(j - i) / Z_i times (1 - switch_prob) when v' = v, switch_prob when it flips.
Viterbi, in the log domain, log 0 = -inf (and never inf - inf: Z and the in-band w are positive).  delta_0(s) = log(1 / (2 nb)) +
  log obs_0(s); delta_t(j, v') = log obs_t(j, v') + max over the predecessors (i, v) with |i - j| <= h of
  ((delta_{t-1}(i, v) - log Z_i) + log w(j - i)) + log P(switch).  Predecessors are taken in the order of their state index (the voiced
  bins ascending, then the unvoiced ones) and a later one replaces the best only when strictly greater: ties go to the lowest
  predecessor index, also when every value is -inf.  The path ends in the best final state, the lowest index on ties, and follows
  the backpointers.  f0[f] = fmin 2^(bin / bo) for a voiced state, 0 for an unvoiced one.
"""
import math

import numpy as np
import torch

from . import _lib, ops, ragged
from .pitch import F0_CEIL, F0_FLOOR, frame_count

FRAME_LENGTH, N_THRESHOLDS, BETA, NO_TROUGH_PROB = 2048, 100, (2, 18), 0.01
BINS_PER_SEMITONE, MAX_TRANSITION_RATE, SWITCH_PROB = 20, 35.92, 0.01
FRAME_BUDGET = 32768                    # padded frames per chunk of rows: 13.4 KB of observations, 2.5 KB of d', 1.7 KB of backpointers each
WHO = "fastspeech2_amd.pyin"


def _round(v):
    return int(math.floor(v + 0.5))


def hop_samples(fs, frame_period):
    return _round(frame_period / 1000.0 * fs)


def lag_range(fs, fmin=F0_FLOOR, fmax=F0_CEIL, frame_length=FRAME_LENGTH):
    """(tau_min, tau_max)"""
    W = frame_length // 2
    return int(math.floor(fs / fmax)), min(int(math.ceil(fs / fmin)), frame_length - W - 1)


def n_bins(fmin=F0_FLOOR, fmax=F0_CEIL, bins_per_semitone=BINS_PER_SEMITONE):
    return int(math.floor(12 * bins_per_semitone * math.log2(fmax / fmin))) + 1


def half_width(fs, hop, max_transition_rate=MAX_TRANSITION_RATE, bins_per_semitone=BINS_PER_SEMITONE):
    return _round(max_transition_rate * 12 * hop / fs) * (bins_per_semitone // 2)


def beta_cdf(x, a, b):
    n = a + b - 1
    return sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))


def threshold_weights(n_thresholds=N_THRESHOLDS, beta=BETA):
    c = [beta_cdf(k / n_thresholds, *beta) for k in range(n_thresholds + 1)]
    return np.diff(np.array(c, dtype=np.float64))


def transition_band(nb, h):
    """(log w(delta) for delta = -h .. h, log Z_i for the nb bins)"""
    w = h + 1.0 - np.abs(np.arange(-h, h + 1, dtype=np.float64))
    i = np.arange(nb)[:, None] + np.arange(-h, h + 1)[None, :]
    Z = np.where((i >= 0) & (i < nb), w[None, :], 0.0).sum(axis=1)
    return np.log(w), np.log(Z)


_consts = {}


def _params(fs, frame_period, fmin, fmax, frame_length, n_thresholds, beta, no_trough_prob, bins_per_semitone, max_transition_rate,
            switch_prob):
    hop = hop_samples(fs, frame_period)
    if not (isinstance(frame_length, int) and frame_length >= 4 and frame_length % 2 == 0) or hop < 1:
        raise ValueError(f"frame_length must be an even integer >= 4 and the hop at least one sample, got {frame_length}, {hop}")
    if not 0 < fmin < fmax or bins_per_semitone < 2 or bins_per_semitone % 2 or n_thresholds < 1 \
            or not all(isinstance(v, int) and v >= 1 for v in beta) or not 0 <= switch_prob <= 1 or not 0 <= no_trough_prob <= 1:
        raise ValueError("pyin: 0 < fmin < fmax, an even bins_per_semitone, integer Beta parameters and probabilities in [0, 1] are needed")
    tmin, tmax = lag_range(fs, fmin, fmax, frame_length)
    if not 1 <= tmin < tmax:
        raise ValueError(f"fmin {fmin}, fmax {fmax} and frame_length {frame_length} leave no lag range at fs {fs} ({tmin}..{tmax})")
    return dict(hop=hop, L=frame_length, tmin=tmin, tmax=tmax, nb=n_bins(fmin, fmax, bins_per_semitone), bo=12 * bins_per_semitone,
                h=half_width(fs, hop, max_transition_rate, bins_per_semitone))


def _device_consts(dev, p, n_thresholds, beta):
    key = (str(dev), p["nb"], p["h"], n_thresholds, tuple(beta))
    if key not in _consts:
        logw, logz = transition_band(p["nb"], p["h"])
        _consts[key] = dict(beta=torch.tensor(threshold_weights(n_thresholds, beta), dtype=torch.float64, device=dev),
                            logw=torch.tensor(logw, dtype=torch.float64, device=dev),
                            logz=torch.tensor(logz, dtype=torch.float64, device=dev))
    return _consts[key]


def _frames_arg(frames, B, Fmax, dev):
    return ragged.lengths(frames, B, Fmax, "frames", dev)[1]


def _stage_input(t, ndim, what):
    """a float64 tensor of `ndim` dimensions on the GPU, contiguous"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != ndim:
        raise ValueError(f"{what} must be a {ndim}-dimensional float64 tensor on the GPU")
    return ragged.require_device(t, WHO).contiguous()


# The launches proper: validated inputs, lengths already on the device.  `pyin` builds lens / frames once per batch and hands each
# chunk of rows a slice; the public stage functions below validate and build them for one call.
def _cmnd(y, lens_d, frames_d, hop, frame_length, tmax, Fmax):
    B, N = y.shape
    out = torch.empty(B, Fmax, tmax + 1, dtype=torch.float64, device=y.device)
    _lib.call("fs2_pyin_cmnd", y.data_ptr(), y.stride(0), lens_d.data_ptr(), frames_d.data_ptr(), hop, frame_length, tmax,
              out.data_ptr(), B, Fmax, N, ops._stream())
    return out


def _observe(dprime, frames_d, tmin, fs, fmin, no_trough_prob, bins_per_semitone, nb, weights):
    B, Fmax, nl = dprime.shape
    obs = torch.empty(B, Fmax, 2 * nb, dtype=torch.float64, device=dprime.device)
    pv = torch.empty(B, Fmax, dtype=torch.float64, device=dprime.device)
    _lib.call("fs2_pyin_observe", dprime.data_ptr(), frames_d.data_ptr(), tmin, nl - 1, weights.data_ptr(), weights.numel(),
              float(no_trough_prob), float(fs), float(fmin), 12 * bins_per_semitone, nb, obs.data_ptr(), pv.data_ptr(), B, Fmax,
              ops._stream())
    return obs, pv


def _viterbi(obs, frames_d, h, fmin, bins_per_semitone, switch_prob, logw, logz):
    B, Fmax, S = obs.shape
    bp = torch.empty(B, Fmax, S, dtype=torch.uint8, device=obs.device)      # one byte per (frame, state): the workspace is sized here
    states = torch.empty(B, Fmax, dtype=torch.int32, device=obs.device)
    f0 = torch.empty(B, Fmax, dtype=torch.float64, device=obs.device)
    _lib.call("fs2_pyin_viterbi", obs.data_ptr(), frames_d.data_ptr(), S // 2, h, logw.data_ptr(), logz.data_ptr(), float(switch_prob),
              float(fmin), 12 * bins_per_semitone, bp.data_ptr(), states.data_ptr(), f0.data_ptr(), B, Fmax, ops._stream())
    return states, f0


def cmnd(y, lens, frames, hop, frame_length, tmax, Fmax=None):
    """Stage 1: y (B, N) float32 on the GPU, lens, frames per row -> d' (B, Fmax, tmax + 1) float64."""
    y, _, lens_d = ragged.rows(y, lens, WHO)
    frames_h = ragged.lengths(frames, y.shape[0], 1 << 30, "frames")
    Fmax = max(frames_h, default=0) if Fmax is None else Fmax
    return _cmnd(y, lens_d, _frames_arg(frames_h, y.shape[0], Fmax, y.device), hop, frame_length, tmax, Fmax)


def observe(dprime, frames, tmin, fs, fmin=F0_FLOOR, fmax=F0_CEIL, n_thresholds=N_THRESHOLDS, beta=BETA,
            no_trough_prob=NO_TROUGH_PROB, bins_per_semitone=BINS_PER_SEMITONE):
    """Stage 2: d' (B, Fmax, tmax + 1) float64 on the GPU -> (obs (B, Fmax, 2 nb) float64, voiced probability (B, Fmax))."""
    dprime = _stage_input(dprime, 3, "dprime")
    weights = torch.tensor(threshold_weights(n_thresholds, beta), dtype=torch.float64, device=dprime.device)
    return _observe(dprime, _frames_arg(frames, dprime.shape[0], dprime.shape[1], dprime.device), tmin, fs, fmin, no_trough_prob,
                    bins_per_semitone, n_bins(fmin, fmax, bins_per_semitone), weights)


def viterbi(obs, frames, h, fmin=F0_FLOOR, bins_per_semitone=BINS_PER_SEMITONE, switch_prob=SWITCH_PROB):
    """Stage 3: obs (B, Fmax, 2 nb) float64 on the GPU -> (states (B, Fmax) int32, f0 (B, Fmax) float64)."""
    obs = _stage_input(obs, 3, "obs")
    if obs.shape[2] % 2:
        raise ValueError("obs must hold 2 nb values per frame")
    logw, logz = (torch.tensor(v, dtype=torch.float64, device=obs.device) for v in transition_band(obs.shape[2] // 2, h))
    return _viterbi(obs, _frames_arg(frames, obs.shape[0], obs.shape[1], obs.device), h, fmin, bins_per_semitone, switch_prob, logw, logz)


def workspace_bytes(rows, Fmax, nb=None, tmax=None, frame_budget=FRAME_BUDGET):
    """Device bytes `pyin` holds at its peak for a batch of `rows` rows of at most Fmax frames: one chunk's d', observations and
    backpointers (a chunk is at most `frame_budget` padded frames, or one row), besides the (rows, Fmax) results."""
    nb = n_bins() if nb is None else nb
    tmax = 311 if tmax is None else tmax
    padded = min(rows * Fmax, max(frame_budget, Fmax))
    return padded * (2 * nb * 8 + (tmax + 1) * 8 + 2 * nb + 24) + rows * Fmax * 20


def row_chunks(frames_h, budget=FRAME_BUDGET):
    """Consecutive rows [r0, r1) whose padded frame count (r1 - r0) max(frames) stays within `budget`; a chunk holds at least one row."""
    r0 = 0
    while r0 < len(frames_h):
        r1, top = r0 + 1, frames_h[r0]
        while r1 < len(frames_h) and (r1 + 1 - r0) * max(top, frames_h[r1]) <= budget:
            top = max(top, frames_h[r1])
            r1 += 1
        yield r0, r1
        r0 = r1


def pyin(y, lens, fs, frame_period, fmin=F0_FLOOR, fmax=F0_CEIL, frame_length=FRAME_LENGTH, n_thresholds=N_THRESHOLDS, beta=BETA,
         no_trough_prob=NO_TROUGH_PROB, bins_per_semitone=BINS_PER_SEMITONE, max_transition_rate=MAX_TRANSITION_RATE,
         switch_prob=SWITCH_PROB, frame_budget=FRAME_BUDGET, return_states=False):
    """pYIN over a ragged batch: y (B, N) float32 on the GPU, row b holds lens[b] samples.  Returns (f0 (B, Fmax) float64 on the
    device, voiced probability (B, Fmax) float64 on the device, t (Fmax,) float64, frames (B,) int64); both are 0 at and beyond
    frames[b].  The workspaces (d', observations, backpointers) are allocated per chunk of rows of at most `frame_budget` padded
    frames, never for the whole batch.  With `return_states` the HMM states (B, Fmax) int32 follow as a fifth value."""
    y, lens_h, lens_d = ragged.rows(y, lens, WHO)
    dev, (B, N) = y.device, y.shape
    p = _params(fs, frame_period, fmin, fmax, frame_length, n_thresholds, beta, no_trough_prob, bins_per_semitone,
                max_transition_rate, switch_prob)
    if 2 * (2 * p["h"] + 1) > 255:
        raise ValueError(f"a transition band of {2 * p['h'] + 1} bins does not fit the one-byte backpointer (FS2_EINVAL): lower "
                         f"max_transition_rate, bins_per_semitone or the hop")
    c = _device_consts(dev, p, n_thresholds, beta)
    frames_h = [frame_count(n, fs, frame_period) for n in lens_h]
    Fmax = max(frames_h, default=0)
    f0 = torch.zeros(B, Fmax, dtype=torch.float64, device=dev)
    pv = torch.zeros(B, Fmax, dtype=torch.float64, device=dev)
    states = torch.zeros(B, Fmax, dtype=torch.int32, device=dev)
    frames_d = torch.tensor(frames_h, dtype=torch.int32, device=dev)         # once per batch; a chunk takes slices
    nb = p["nb"]
    for r0, r1 in row_chunks(frames_h, frame_budget):
        Fc, fd = max(frames_h[r0:r1]), frames_d[r0:r1]
        d = _cmnd(y[r0:r1], lens_d[r0:r1], fd, p["hop"], p["L"], p["tmax"], Fc)
        obs, pvc = _observe(d, fd, p["tmin"], fs, fmin, no_trough_prob, bins_per_semitone, nb, c["beta"])
        del d
        st, f = _viterbi(obs, fd, p["h"], fmin, bins_per_semitone, switch_prob, c["logw"], c["logz"])
        del obs
        f0[r0:r1, :Fc], pv[r0:r1, :Fc], states[r0:r1, :Fc] = f, pvc, st
    t = np.arange(Fmax) * frame_period / 1000.0
    out = (f0, pv, t, torch.tensor(frames_h, dtype=torch.int64))
    return out + (states,) if return_states else out


def pyin_numpy(y, lens, fs, frame_period, **params):
    """`pyin` with one D2H copy at the end: (f0 (B, Fmax) float64 numpy, voiced probability numpy, t (Fmax,), frames (B,) int64 numpy)."""
    f0, pv, t, frames = pyin(y, lens, fs, frame_period, **params)
    both = torch.stack([f0, pv]).cpu().numpy()
    return both[0], both[1], t, frames.numpy()


def pitch_fn(device="cuda"):
    """`pitch_fn(wav, sampling_rate, hop_length) -> f0` (numpy in, float64 numpy out, one value per frame), the signature
    `Preprocessor(pitch_fn=...)` takes, computed on `device`."""
    dev = torch.device(device)

    def fn(wav, sampling_rate, hop_length):
        w = torch.as_tensor(np.ascontiguousarray(wav, dtype=np.float32)).reshape(1, -1).to(dev)
        f0, _, _, frames = pyin_numpy(w, [w.shape[1]], sampling_rate, hop_length / sampling_rate * 1000)
        return f0[0, :frames[0]]
    return fn
