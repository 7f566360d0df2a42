"""Modulation-spectrum postfilter on the GPU (csrc/fs2_msfilter.hip): the remedy of Takamichi, Toda, Black, Neubig, Sakti, Nakamura
2016 for the over-smoothing that `modspec` measures.  The acoustic model is not retrained: the log modulation spectrum (MS) of every
generated trajectory is moved from the statistics of generated speech to those of natural speech, and its phase is kept.  The
specification below is what the kernels and the independent numpy restatement (tests/postfilter_ref.py, with an FFT) implement.  It
uses `modspec`'s constants N = NFFT = 4096, MAX_FRAMES = 2048, MAX_COEF = 128, FLOOR = 1e-12, MIN_FRAMES = 32 and its host-built fp64
table `twiddles()`: the device evaluates no sine or cosine.

Arithmetic.  fp64 whatever the type of the trajectories, as in `modspec`: every sum runs over its terms in ascending order in one
thread with its rounding errors carried in a second word.  No atomics, no reduction across lanes; padding is never read or written;
two runs give the same bytes.

Statistics (`Stats`).  For every coefficient k and bin f = 0 .. N / 2, ms[f] = ln(|X[f]|^2 / T + FLOOR) of the mean-removed trajectory
zero-padded to N, exactly as `modspec` defines it and as its kernel writes it (`logms`).  Over a set of utterances the mean and the
sample standard deviation (n - 1) of ms[f] are kept: mu_n, sd_n over natural mels, mu_g, sd_g over generated ones.  The kernel
fs2_ms_stats_update folds batch after batch into a running (mean, M2) per (k, f) with Welford's update, the rows in ascending order.
An utterance with fewer than MIN_FRAMES or more than MAX_FRAMES frames is left out and counted; a side with fewer than 2 kept
utterances is refused.

Filter (`apply`, kernel fs2_ms_filter).  For a trajectory x[t], t < T, of coefficient k, with the mean m that `modspec.moments` gives:
X[f] = the forward DFT of (x - m) zero-padded to N, f = 0 .. N / 2, and ms[f] as above; r[f] = sd_n[f] / sd_g[f], or 1 where sd_g[f] is
not above 0; target[f] = r[f] (ms[f] - mu_g[f]) + mu_n[f]; ln g[f] = 0.5 k (target[f] - ms[f]) clamped to +- MAX_GAIN_DB (ln 10) / 20;
g[0] = 1;

    y[t] = m + (1 / N) [X[0] + 2 sum_{f = 1}^{N / 2 - 1} Re(g[f] X[f] e^{+2 pi i f t / N}) + g[N / 2] X[N / 2] (-1)^t],   t < T only.

The padded tail of the inverse transform is discarded, as in the paper; the mean is untouched.  MAX_GAIN_DB = 20 is a choice: it keeps
a bin that sits on the floor, whose ms says nothing, from being raised by the whole distance to the natural mean.

Emphasis coefficient.  0 <= k <= 1; k = 1 moves the MS all the way, k = 0 leaves the trajectory alone.  The default 0.85 is the paper's
setting as its reader here recalls it: a choice, not a measurement of this project.

Pass-through.  A row with T < MIN_FRAMES or T > MAX_FRAMES is copied unchanged (`pass_through` counts such rows).  k = 0 runs no
kernel at all.

Files (`Tables.save`, `load`).  One .npz: mu_n, sd_n, mu_g, sd_g (n_mel, N / 2 + 1) float64, n_natural, n_generated, left_out_natural,
left_out_generated, n_mel, sampling_rate, hop_length, nfft, floor, restore_step.  `load` refuses a file whose n_mel, sampling_rate or
hop_length differ from the preprocess config it is given, or whose nfft or floor are not this module's.

What is claimed: the published filter as written above, held against the restatement and against known answers (equal statistics,
a pure gain, a constant, a smoothed noise corpus, the clamp).  Not claimed: any listening result; any number on real speech; the
choices 0.85, 20 dB and 32 frames; that statistics pooled over speakers suit a multi-speaker corpus.
"""
import numpy as np
import torch

from . import _lib, ops
from . import modspec as MS

WHO = "fastspeech2_amd.postfilter"
NFFT, MAX_FRAMES, MAX_COEF, FLOOR, MIN_FRAMES = MS.NFFT, MS.MAX_FRAMES, MS.MAX_COEF, MS.FLOOR, MS.MIN_FRAMES
BINS = NFFT // 2 + 1
MAX_GAIN_DB = 20.0
K_DEFAULT = 0.85
_ONE_BAND = ((1, BINS),)                                   # `modspec` wants a band table; only its logms is used here


def _lens(lens):
    h = [int(v) for v in (lens.tolist() if isinstance(lens, (torch.Tensor, np.ndarray)) else lens)]
    for n in h:
        if n < 1:
            raise ValueError(f"a trajectory of {n} frames: every row needs at least one frame")
    return h


def _kept(n):
    return MIN_FRAMES <= n <= MAX_FRAMES


def pass_through(lens):
    """how many of these rows `apply` copies unchanged: fewer than MIN_FRAMES or more than MAX_FRAMES frames"""
    return sum(1 for n in _lens(lens) if not _kept(n))


def _input(c, lens, K=None):
    """c (B, >= Tmax, K) float32 or float64 on the device with unit stride in k, and its host lengths, checked as `modspec._input`
    checks them but for the frame bound, which is a pass-through case here -> (c, B, K, lens on the host)"""
    h = _lens(lens)
    if not isinstance(c, torch.Tensor) or c.device.type != "cuda":
        raise ValueError(f"the trajectories must be a tensor on the GPU ({WHO} has no CPU fallback)")
    if c.dtype not in (torch.float32, torch.float64) or c.dim() != 3 or (c.numel() and c.stride(-1) != 1):
        raise ValueError(f"the trajectories must be a 3-D float32 or float64 tensor with unit inner stride, got {c.dtype} {tuple(c.shape)}")
    B, width, Kc = c.shape
    if not 1 <= Kc <= MAX_COEF or (K is not None and Kc != K):
        raise ValueError(f"{Kc} coefficients, " + (f"the statistics hold {K}" if K is not None else f"supported are 1..{MAX_COEF}"))
    Tmax = max(h, default=1)
    if len(h) != B or width < Tmax:
        raise ValueError(f"trajectories {tuple(c.shape)} do not hold {len(h)} rows of up to {Tmax} frames")
    if B and (c.stride(1) < Kc or (B > 1 and c.stride(0) < Tmax * c.stride(1))):
        raise ValueError(f"the trajectories have overlapping strides {c.stride()}")
    return c, B, Kc, h


# ------------------------------------------------------------------------------------------------ statistics
class Tables:
    """The finalised statistics: mu_n, sd_n, mu_g, sd_g (n_mel, N / 2 + 1) float64 on the host, what they were taken from, and a
    copy per device made on first use."""

    def __init__(self, mu_n, sd_n, mu_g, sd_g, n_natural, n_generated, left_out_natural, left_out_generated, n_mel, sampling_rate,
                 hop_length, restore_step=0):
        self.mu_n, self.sd_n, self.mu_g, self.sd_g = (np.ascontiguousarray(np.asarray(a, np.float64)) for a in (mu_n, sd_n, mu_g, sd_g))
        self.n_mel, self.sampling_rate, self.hop_length = int(n_mel), int(sampling_rate), int(hop_length)
        self.n_natural, self.n_generated = int(n_natural), int(n_generated)
        self.left_out_natural, self.left_out_generated = int(left_out_natural), int(left_out_generated)
        self.restore_step = int(restore_step)
        if not 1 <= self.n_mel <= MAX_COEF:
            raise ValueError(f"{self.n_mel} coefficients, supported are 1..{MAX_COEF}")
        for name in ("mu_n", "sd_n", "mu_g", "sd_g"):
            a = getattr(self, name)
            if a.shape != (self.n_mel, BINS) or not np.isfinite(a).all():
                raise ValueError(f"{name} must be a finite ({self.n_mel}, {BINS}) table, got {a.shape}")
        if min(self.n_natural, self.n_generated) < 2:
            raise ValueError(f"statistics over {self.n_natural} natural and {self.n_generated} generated utterances: each side needs at least 2")
        self._dev = {}

    def on(self, device):
        """(4, n_mel, N / 2 + 1) float64 on `device`: mu_n, sd_n, mu_g, sd_g"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(np.stack([self.mu_n, self.sd_n, self.mu_g, self.sd_g])).to(device)
        return self._dev[key]

    def check_config(self, preprocess_config):
        pp = preprocess_config["preprocessing"]
        want = (pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"], pp["stft"]["hop_length"])
        have = (self.n_mel, self.sampling_rate, self.hop_length)
        if tuple(int(v) for v in want) != have:
            raise ValueError(f"the statistics were taken at (n_mel, sampling_rate, hop_length) = {have}, the preprocess config says {tuple(want)}")

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, mu_n=self.mu_n, sd_n=self.sd_n, mu_g=self.mu_g, sd_g=self.sd_g, n_natural=self.n_natural, n_generated=self.n_generated,
                     left_out_natural=self.left_out_natural, left_out_generated=self.left_out_generated, n_mel=self.n_mel,
                     sampling_rate=self.sampling_rate, hop_length=self.hop_length, nfft=NFFT, floor=FLOOR, restore_step=self.restore_step)


def load(path, preprocess_config=None):
    """The Tables that `Tables.save` wrote; with a preprocess config, refused unless its n_mel, sampling rate and hop length match."""
    with np.load(path, allow_pickle=False) as z:
        if int(z["nfft"]) != NFFT or float(z["floor"]) != FLOOR:
            raise ValueError(f"{path}: taken with N = {int(z['nfft'])} and floor {float(z['floor'])}, this module has {NFFT} and {FLOOR}")
        t = Tables(z["mu_n"], z["sd_n"], z["mu_g"], z["sd_g"], z["n_natural"], z["n_generated"], z["left_out_natural"],
                   z["left_out_generated"], z["n_mel"], z["sampling_rate"], z["hop_length"], z["restore_step"])
    if preprocess_config is not None:
        t.check_config(preprocess_config)
    return t


class Stats:
    """Accumulates the MS statistics of natural and of generated trajectories on the device, batch by batch.

    s = Stats(n_mel, sampling_rate, hop_length); s.add_natural(c, lens); s.add_generated(c, lens); ...; tables = s.finalize()"""

    def __init__(self, n_mel, sampling_rate, hop_length, restore_step=0):
        if not 1 <= int(n_mel) <= MAX_COEF:
            raise ValueError(f"{n_mel} coefficients, supported are 1..{MAX_COEF}")
        self.n_mel, self.sampling_rate, self.hop_length, self.restore_step = int(n_mel), int(sampling_rate), int(hop_length), int(restore_step)
        self._state = {"natural": None, "generated": None}                 # (K, N / 2 + 1, 2) float64 on the device: mean, M2
        self.count = {"natural": 0, "generated": 0}
        self.left_out = {"natural": 0, "generated": 0}

    def add_natural(self, c, lens):
        return self._add("natural", c, lens)

    def add_generated(self, c, lens):
        return self._add("generated", c, lens)

    def _add(self, side, c, lens):
        """c (B, >= Tmax, n_mel) float32 or float64 on the device, lens frames per row -> how many rows were kept"""
        c, B, K, h = _input(c, lens, self.n_mel)
        keep = [1 if _kept(n) else 0 for n in h]
        if not any(keep):
            self.left_out[side] += B
            return 0
        short = [n if k else 1 for n, k in zip(h, keep)]                    # a row that is left out costs one frame
        c = c[:, :max(short)]
        c = c if c.dtype == torch.float64 else c.double()
        mom = MS.moments(c, short)
        _, logms = MS.modspec(c, short, mom[:, :, 0], _ONE_BAND, logms=True)
        state = self._state[side]
        if state is None:
            state = self._state[side] = torch.empty((K, BINS, 2), dtype=torch.float64, device=c.device)
        elif state.device != c.device:
            raise ValueError(f"the {side} statistics live on {state.device}, this batch on {c.device}")
        keep_d = torch.tensor(keep, dtype=torch.int32, device=c.device)
        _lib.call("fs2_ms_stats_update", logms.data_ptr(), logms.stride(0), logms.stride(1), keep_d.data_ptr(), state.data_ptr(),
                  state.stride(0), self.count[side], B, K, ops._stream())
        self.count[side] += sum(keep)
        self.left_out[side] += B - sum(keep)
        return sum(keep)

    def finalize(self):
        for side in ("natural", "generated"):
            if self.count[side] < 2:
                raise ValueError(f"{self.count[side]} {side} utterances of {MIN_FRAMES}..{MAX_FRAMES} frames ({self.left_out[side]} left out): "
                                 "the statistics need at least 2")
        out = []
        for side in ("natural", "generated"):
            st = self._state[side].cpu().numpy()
            out += [st[:, :, 0], np.sqrt(st[:, :, 1] / (self.count[side] - 1))]
        return Tables(*out, self.count["natural"], self.count["generated"], self.left_out["natural"], self.left_out["generated"],
                      self.n_mel, self.sampling_rate, self.hop_length, self.restore_step)


# ------------------------------------------------------------------------------------------------ filter
def _check_k(k):
    k = float(k)
    if not 0.0 <= k <= 1.0:
        raise ValueError(f"the emphasis coefficient must lie in [0, 1], got {k}")
    return k


def apply(mel, lens, stats, k=K_DEFAULT, out=None):
    """mel (B, >= Tmax, K) float32 or float64 on the device with unit stride in k, lens frames per row on the host, stats the `Tables`
    -> the filtered trajectories in mel's dtype.  Without `out` the result is a copy of mel whose frames t < lens[b] are filtered
    (padding stays what it was); `out` is a buffer of the caller, at least (B, Tmax, K), of which nothing else is written.  k = 0
    launches nothing and returns mel itself (or copies the rows into `out`)."""
    k = _check_k(k)
    if not isinstance(stats, Tables):
        raise ValueError(f"stats must be {WHO}.Tables (Stats.finalize() or load()), got {type(stats).__name__}")
    mel, B, K, h = _input(mel, lens, stats.n_mel)
    Tmax = max(h, default=1)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.device != mel.device or out.dtype != mel.dtype or out.dim() != 3 or out.stride(-1) != 1 \
                or out.shape[0] != B or out.shape[1] < Tmax or out.shape[2] < K or out.stride(1) < K \
                or (B > 1 and out.stride(0) < Tmax * out.stride(1)) or out.data_ptr() == mel.data_ptr():
            raise ValueError(f"out must be another {mel.dtype} tensor on {mel.device} that holds {(B, Tmax, K)} with unit inner stride")
    if k == 0.0 or B == 0:
        if out is None:
            return mel
        for b, n in enumerate(h):
            out[b, :n, :K].copy_(mel[b, :n])
        return out
    dev_lens = [n if n <= MAX_FRAMES else 0 for n in h]                     # the kernel leaves a row of 0 frames alone
    if out is None:
        out = mel.clone(memory_format=torch.contiguous_format)
    else:
        for b, n in enumerate(h):
            if n > MAX_FRAMES:
                out[b, :n, :K].copy_(mel[b, :n])
    if not any(dev_lens):
        return out
    width = min(max(dev_lens), MAX_FRAMES)
    c = mel[:, :width]
    c64 = c if c.dtype == torch.float64 else c.double()
    mom = MS.moments(c64, [max(n, 1) for n in dev_lens])
    lens_d = torch.tensor(dev_lens, dtype=torch.int32, device=mel.device)
    tab = stats.on(mel.device)
    _lib.call("fs2_ms_filter", c.data_ptr(), c.stride(0), c.stride(1), lens_d.data_ptr(), mom.data_ptr(), mom.stride(0), mom.stride(1),
              MS._twiddles_on(mel.device).data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), tab[3].data_ptr(), tab.stride(1),
              k, FLOOR, MAX_GAIN_DB, MIN_FRAMES, out.data_ptr(), out.stride(0), out.stride(1), 1 if mel.dtype == torch.float64 else 0,
              B, width, K, ops._stream())
    return out
