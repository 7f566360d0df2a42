"""Speaker similarity by a GMM-UBM verifier: does a synthesized utterance sound like the speaker it was asked to be?  The algorithm is
that of Reynolds, Quatieri and Dunn (2000), "Speaker verification using adapted Gaussian mixture models": a universal background
model (UBM), one diagonal Gaussian mixture trained on everyone's speech; one model per speaker, MAP-adapted from the UBM's means;
the score, the average per-frame log-likelihood ratio between the two.  The kernels are csrc/fs2_spk.hip; tests/spk_ref.py restates
this specification in numpy.  Every default below that the paper does not fix is a choice and is marked so.

Features.  The log-mel spectrogram is the project's own (wav -> STFT -> mel, as recognize.py and score.py take it).  n_cep + 1
cepstra c0 .. c_n_cep come from fs2_mcep with the rows k = 0 .. n_cep of the orthonormal DCT-II (row 0 is sqrt(1 / n_mel));
n_cep = 19 (a choice).  c0 is dropped from the vector and kept as the frame's energy.  Deltas are appended: sum_k k (c[t + k] -
c[t - k]) / (2 sum_k k^2), k = 1, 2, time indices clamped to the utterance.  D = 2 n_cep (38), D <= 64.  A frame is kept when c0 >=
max_t c0 - energy_floor; the default floor is 1.5 ln 10 sqrt(n_mel), the c0 difference of 30 dB in amplitude (a choice).  Mean and
variance (the mean of the squared differences from that mean) are taken per utterance over the kept frames in ascending order, and
the kept frames are normalised to (f - mean) / sqrt(var).  An utterance with fewer than 2 kept frames keeps none; an utterance
with a variance that is not > 0 in any dimension (a constant utterance) keeps none either.  Kept frames are packed in time order
at row offs[b], the exclusive sum of lens; n_kept[b] is returned.

Model tables.  A mixture (w, mu, var) of M components reaches the kernels expanded: a[m][d] = mu / var, b[m][d] = -1 / (2 var),
c[m] = log w - 1/2 sum_d (log(2 pi var) + mu^2 / var), log 0 = -inf; L[n][m] = c[m] + sum_d (x_d a[m][d] + x_d^2 b[m][d]).  The
host builds them in numpy (`expand`).

UBM training, deterministic.  One Gaussian with the global mean and variance; doubled by splitting every component m into 2 m
(mean + 0.2 sd) and 2 m + 1 (mean - 0.2 sd) with half the weight each, until M (a power of two, default 256, a choice) is reached;
`iters` EM passes after each doubling (default 4, a choice), each updating weights, means and variances (n / N, s1 / n, max(s2 / n
- mean^2, floor)); floor = var_floor (0.01, a choice) times the global variance.  A component whose occupancy is under min_occ
(3, a choice) is re-seeded, in ascending order, from a split of the then heaviest component (the lowest index on ties), and the
weights are renormalised.  Frames are pooled from the training list, at most max_frames_per_speaker per speaker, in file order.

Enrolment.  One pass of posteriors under the UBM over the speaker's pooled frames; means only: mu_s[m] = alpha E_m(x) + (1 - alpha)
mu[m], alpha = n_m / (n_m + r), relevance r = 16 (the paper's); a component with n_m = 0 keeps mu[m].  Weights and variances stay
the UBM's, so a speaker's table differs from the UBM's in a and c only.

Score.  llr[u][g] = the mean over u's kept frames of lse_g(x_t) - lse_ubm(x_t), lse the log-sum-exp of L over all M components, in
fp64.  The paper's top-C fast scoring is an approximation and is not built.  Every utterance is scored against every enrolled
speaker.  Per utterance: `llr` to the claimed speaker; its `rank` = 1 + the speakers scoring strictly higher + the lower-indexed
speakers scoring the same; the best `rival` (the lowest index on ties) and the `margin` to it; `n_kept`.  Per corpus: the mean
target llr, the top-1 accuracy (rank = 1), a per-speaker table of both, and the equal error rate over all (utterance, speaker)
trials: thresholds are the distinct scores ascending and then +inf, a trial is accepted when score >= threshold, FAR = accepted
non-targets / non-targets, FRR = rejected targets / targets, d = FRR - FAR; at the first threshold i with d_i >= 0 the EER is FRR_i
when d_i = 0, else FRR_(i-1) + t (FRR_i - FRR_(i-1)), t = -d_(i-1) / (d_i - d_(i-1)).  Utterances of a speaker the model does not
hold, missing wavs and utterances that keep no frame are listed and not counted.

What is claimed: the published algorithm written down in full, pinned to an independent restatement and to known answers.  Not
claimed: agreement with any toolkit (Kaldi, ALIZE, SIDEKIT), anything about neural speaker-embedding similarity, any number on
real speech.  Only the difference between the score of a synthesized folder and that of the recorded wavs under one model means
anything."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, ops, ragged

WHO = "fastspeech2_amd.speaker"
FORMAT = 1
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ kernels
def max_dim():
    return _lib.load().fs2_spk_max_dim()


def max_components():
    return _lib.load().fs2_spk_max_components()


def dct_table0(n_mel, n_cep):
    """(n_cep + 1, n_mel) float64: rows k = 0 .. n_cep of the orthonormal DCT-II"""
    if not 1 <= n_cep <= max_dim() // 2 or n_cep >= n_mel:
        raise ValueError(f"n_cep must be in [1, {max_dim() // 2}] and below n_mel, got n_cep={n_cep}, n_mel={n_mel}")
    k = np.arange(n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    t = np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (2.0 * m + 1.0) / (2.0 * n_mel))
    t[0] = np.sqrt(1.0 / n_mel)
    return t


def default_energy_floor(n_mel):
    return 1.5 * float(np.log(10.0)) * float(np.sqrt(n_mel))


def _dev(t, dtype, what, dim):
    ragged.require_device(t, WHO)
    if t.dtype != dtype or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _ld(t):
    """row stride of a 2-D tensor, at least its width (a tensor of one row reports any)"""
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else max(t.shape[1], 1)


_tables = {}


def cepstra0(mel, lens, n_cep=19):
    """mel (B, n_mel, frames) float32 log-mel on the device -> c (B, Tmax, n_cep + 1) float64, column 0 the energy c0"""
    ragged.require_device(mel, WHO)
    if mel.dtype != torch.float32 or mel.dim() != 3 or (mel.numel() and mel.stride(2) != 1):
        raise ValueError(f"mel must be a (B, n_mel, frames) float32 tensor with unit inner stride, got {mel.dtype} {tuple(mel.shape)}")
    B, n_mel, F = mel.shape
    lens_h, lens_d = ragged.lengths(lens, B, F, "lens", mel.device)
    key = (str(mel.device), n_mel, n_cep)
    if key not in _tables:
        _tables[key] = torch.from_numpy(dct_table0(n_mel, n_cep)).to(mel.device)
    Tmax = max(lens_h, default=0)
    c = torch.empty(B, Tmax, n_cep + 1, dtype=F64, device=mel.device)
    _lib.call("fs2_mcep", mel.data_ptr(), mel.stride(0), mel.stride(1), lens_d.data_ptr(), _tables[key].data_ptr(), n_cep + 1,
              c.data_ptr(), c.stride(0), c.stride(1), B, n_mel, Tmax, ops._stream())
    return c


def features(cep, lens, energy_floor, out=None):
    """cep (B, Tmax, n_cep + 1) float64 on the device -> (feat (sum lens, >= D) packed, offs (host list), n_kept (B,) int32, mean,
    var (B, D)), all but offs on the device.  `out` may give the packed buffer (a strided view); rows beyond n_kept[b] of an
    utterance's block are not written."""
    cep = _dev(cep, F64, "cep", 3)
    B, Tmax, K = cep.shape
    n_cep = K - 1
    if not 1 <= n_cep <= max_dim() // 2:
        raise ValueError(f"{n_cep} cepstra beside c0, supported are 1..{max_dim() // 2}")
    if not energy_floor >= 0:
        raise ValueError(f"energy_floor must be >= 0, got {energy_floor}")
    lens_h, lens_d = ragged.lengths(lens, B, Tmax, "lens", cep.device)
    offs = [0] * B
    for b in range(1, B):
        offs[b] = offs[b - 1] + lens_h[b - 1]
    N, D = sum(lens_h), 2 * n_cep
    if out is None:
        feat = torch.empty(max(N, 1), D, dtype=F64, device=cep.device)
    else:
        feat = _dev(out, F64, "out", 2)
        if feat.shape[0] < N or feat.shape[1] < D or feat.device != cep.device:
            raise ValueError(f"out {tuple(feat.shape)} is not (>= {N}, >= {D}) on {cep.device}")
    offs_d = torch.tensor(offs, dtype=torch.int32, device=cep.device)
    n_kept = torch.empty(B, dtype=torch.int32, device=cep.device)
    mv = torch.empty(2, B, D, dtype=F64, device=cep.device)
    _lib.call("fs2_spk_feats", cep.data_ptr(), cep.stride(0), cep.stride(1), lens_d.data_ptr(), offs_d.data_ptr(), n_cep,
              float(energy_floor), feat.data_ptr(), _ld(feat), n_kept.data_ptr(), mv[0].data_ptr(), mv[1].data_ptr(), D, B, Tmax,
              ops._stream())
    return feat, offs, n_kept, mv[0], mv[1]


def expand(w, mu, var):
    """(w (M,), mu, var (M, D)) numpy -> the tables a, b (M, D), c (M,) of the module docstring"""
    w, mu, var = np.asarray(w, np.float64), np.asarray(mu, np.float64), np.asarray(var, np.float64)
    with np.errstate(divide="ignore"):
        logw = np.log(w)
    c = logw - 0.5 * (np.log(2.0 * np.pi * var).sum(-1) + (mu * mu / var).sum(-1))
    return mu / var, -0.5 / var, c


def _tables_dev(x, a, b, c, G):
    a, b, c = _dev(a, F64, "a", 2), _dev(b, F64, "b", 2), _dev(c, F64, "c", 1).contiguous()
    D = x.shape[1]
    G = int(G)
    if G < 1 or a.shape[0] % G or a.shape != b.shape or a.shape[1] != D or c.shape[0] != a.shape[0] or _ld(a) != _ld(b):
        raise ValueError(f"a {tuple(a.shape)}, b {tuple(b.shape)}, c {tuple(c.shape)}, G = {G} and D = {D} do not fit together")
    M = a.shape[0] // G
    if not 1 <= D <= max_dim() or not 1 <= M <= max_components() or G * M >= 1 << 31:
        raise ValueError(f"{G} groups of {M} components of {D} dimensions: supported are D <= {max_dim()}, M <= {max_components()}, "
                         "G M < 2^31")
    return a, b, c, M, G


def loglik(x, a, b, c, G=1, post=False, out=None):
    """x (N, D) float64 on the device (any row stride), the tables of G groups of M components (a, b (G M, D) sharing a row stride,
    c (G M,)) -> lse (N, G), and with `post` (G = 1 only; True or a buffer (N, >= M)) also the posteriors (N, M)."""
    x = _dev(x, F64, "x", 2)
    a, b, c, M, G = _tables_dev(x, a, b, c, G)
    N, D = x.shape
    if post is not False and G != 1:
        raise ValueError(f"posteriors are written for one group only, got G = {G}")
    if out is None:
        lse = torch.empty(N, G, dtype=F64, device=x.device)
    else:
        lse = _dev(out, F64, "out", 2)
        if lse.shape[0] != N or lse.shape[1] < G:
            raise ValueError(f"out {tuple(lse.shape)} is not ({N}, >= {G})")
    p = None
    if post is True:
        p = torch.empty(N, M, dtype=F64, device=x.device)
    elif post is not False:
        p = _dev(post, F64, "post", 2)
        if p.shape[0] != N or p.shape[1] < M:
            raise ValueError(f"post {tuple(p.shape)} is not ({N}, >= {M})")
    _lib.call("fs2_spk_loglik", x.data_ptr(), _ld(x), a.data_ptr(), b.data_ptr(), _ld(a), c.data_ptr(), lse.data_ptr(), _ld(lse),
              p.data_ptr() if p is not None and N else None, _ld(p) if p is not None else 0, N, D, M, G, ops._stream())
    return (lse, p) if p is not None else lse


def accum_ws(N, D, M):
    return _lib.load().fs2_spk_accum_ws(N, D, M)


def accumulate(post, x, stats=None, ws=None):
    """stats (M, 1 + 2 D) += sum_n post[n][m] (1, x, x^2); a fresh table starts at zero.  `ws` may give the workspace."""
    post, x = _dev(post, F64, "post", 2), _dev(x, F64, "x", 2)
    N, M = post.shape
    D = x.shape[1]
    if x.shape[0] != N or not 1 <= D <= max_dim() or not 1 <= M <= max_components():
        raise ValueError(f"post {tuple(post.shape)} and x {tuple(x.shape)} do not fit together (D <= {max_dim()}, M <= "
                         f"{max_components()})")
    if stats is None:
        stats = torch.zeros(M, 1 + 2 * D, dtype=F64, device=x.device)
    else:
        stats = _dev(stats, F64, "stats", 2)
        if stats.shape[0] != M or stats.shape[1] < 1 + 2 * D:
            raise ValueError(f"stats {tuple(stats.shape)} is not ({M}, >= {1 + 2 * D})")
    need = accum_ws(N, D, M)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=F64, device=x.device)
    _lib.call("fs2_spk_accum", post.data_ptr(), _ld(post), x.data_ptr(), _ld(x), stats.data_ptr(), _ld(stats), ws.data_ptr(),
              ws.numel(), N, D, M, ops._stream())
    return stats


def mean_rows(lse, ubm, offs, n_kept, out=None):
    """lse (N, G), ubm (N,) on the device, offs / n_kept per utterance -> out (U, G): the mean of lse - ubm over each utterance's
    rows, NaN for n_kept = 0"""
    lse, ubm = _dev(lse, F64, "lse", 2), _dev(ubm, F64, "ubm", 1).contiguous()
    N, G = lse.shape
    oh = [int(v) for v in (offs.tolist() if isinstance(offs, (torch.Tensor, np.ndarray)) else offs)]
    nh = [int(v) for v in (n_kept.tolist() if isinstance(n_kept, (torch.Tensor, np.ndarray)) else n_kept)]
    if len(oh) != len(nh) or ubm.shape[0] != N or G < 1 or any(o < 0 or n < 0 or o + n > N for o, n in zip(oh, nh)):
        raise ValueError(f"lse {tuple(lse.shape)}, ubm {tuple(ubm.shape)}, offs {oh} and n_kept {nh} do not fit together")
    U = len(oh)
    if out is None:
        out = torch.empty(U, G, dtype=F64, device=lse.device)
    else:
        out = _dev(out, F64, "out", 2)
        if out.shape[0] != U or out.shape[1] < G:
            raise ValueError(f"out {tuple(out.shape)} is not ({U}, >= {G})")
    if U == 0:
        return out
    if N == 0:                                                             # nothing to read: every utterance is empty
        out[:, :G] = float("nan")
        return out
    od = torch.tensor(oh, dtype=torch.int32, device=lse.device)
    nd = torch.tensor(nh, dtype=torch.int32, device=lse.device)
    _lib.call("fs2_spk_mean_rows", lse.data_ptr(), _ld(lse), ubm.data_ptr(), od.data_ptr(), nd.data_ptr(), out.data_ptr(), _ld(out), U, G,
              ops._stream())
    return out


# ------------------------------------------------------------------------------------------------ the report
def rank_and_rival(row, claimed):
    """-> (rank of `claimed`, best rival or None, margin or None) by the rules of the module docstring"""
    v = row[claimed]
    rank = 1 + sum(1 for g, s in enumerate(row) if s > v or (s == v and g < claimed))
    rival = None
    for g, s in enumerate(row):
        if g != claimed and (rival is None or s > row[rival]):
            rival = g
    return rank, rival, (None if rival is None else float(v - row[rival]))


def equal_error_rate(target, nontarget):
    """The EER of the module docstring, or None without both kinds of trial."""
    tar, non = np.sort(np.asarray(target, np.float64)), np.sort(np.asarray(nontarget, np.float64))
    if not tar.size or not non.size:
        return None
    th = np.append(np.unique(np.concatenate([tar, non])), np.inf)
    frr = np.searchsorted(tar, th, side="left") / tar.size                 # targets below the threshold
    far = (non.size - np.searchsorted(non, th, side="left")) / non.size    # non-targets at or above it
    d = frr - far
    i = int(np.argmax(d >= 0))
    if d[i] == 0:
        return float(frr[i])
    t = -d[i - 1] / (d[i] - d[i - 1])
    return float(frr[i - 1] + t * (frr[i] - frr[i - 1]))


def summarize(rows, missing, names):
    tar = [r["llr"] for r in rows]
    non = [s for r in rows for g, s in enumerate(r["_row"]) if g != r["_claimed"]]
    per = {}
    for r in rows:
        per.setdefault(r["speaker"], []).append(r)
    return {"utterances": len(rows), "missing": len(missing), "speakers_enrolled": len(names),
            "mean_llr": float(np.mean(tar)) if tar else None,
            "accuracy": float(np.mean([r["rank"] == 1 for r in rows])) if rows else None, "eer": equal_error_rate(tar, non),
            "per_speaker": {s: {"utterances": len(v), "accuracy": float(np.mean([r["rank"] == 1 for r in v])),
                                "mean_llr": float(np.mean([r["llr"] for r in v]))} for s, v in sorted(per.items())}}


# ------------------------------------------------------------------------------------------------ the model
def feature_config(config):
    """The settings of a preprocess config the features depend on (stored in a model file, compared on load)."""
    pp = config["preprocessing"]
    return {"sampling_rate": pp["audio"]["sampling_rate"], "filter_length": pp["stft"]["filter_length"],
            "hop_length": pp["stft"]["hop_length"], "win_length": pp["stft"]["win_length"], "n_mel": pp["mel"]["n_mel_channels"],
            "fmin": pp["mel"]["mel_fmin"], "fmax": pp["mel"]["mel_fmax"]}


class SpeakerModel:
    """A UBM (w, mu, var as numpy arrays), the adapted means of the enrolled speakers (S, M, D) and their names in index order."""

    def __init__(self, device, n_cep=19, components=256, iters=4, relevance=16.0, var_floor=0.01, min_occ=3.0, energy_floor=None,
                 feature_config=None, batch_bytes=1 << 30):
        self.device = ragged.require_device(torch.device(device), WHO)
        M = int(components)
        if M < 1 or M & (M - 1) or M > max_components():
            raise ValueError(f"components must be a power of two in [1, {max_components()}], got {components}")
        if not 1 <= n_cep <= max_dim() // 2 or iters < 0 or not relevance >= 0 or not var_floor > 0:
            raise ValueError(f"bad options n_cep={n_cep} iters={iters} relevance={relevance} var_floor={var_floor}")
        self.n_cep, self.components, self.iters, self.relevance = int(n_cep), M, int(iters), float(relevance)
        self.var_floor, self.min_occ, self.energy_floor = float(var_floor), float(min_occ), energy_floor
        self.feature_config, self.batch_bytes = feature_config, int(batch_bytes)
        self.w = self.mu = self.var = None
        self.means, self.names, self.history = None, [], []
        self._dev_tables = None

    @property
    def D(self):
        return 2 * self.n_cep

    def options(self):
        return {"n_cep": self.n_cep, "components": self.components, "iters": self.iters, "relevance": self.relevance,
                "var_floor": self.var_floor, "min_occ": self.min_occ, "energy_floor": self.energy_floor}

    # ---- passes over pooled frames
    def _frames(self, X):
        X = torch.as_tensor(X)
        if X.dtype != F64 or X.dim() != 2 or X.shape[1] != self.D:
            raise ValueError(f"frames must be (N, {self.D}) float64, got {X.dtype} {tuple(X.shape)}")
        return X

    def _pass(self, X, w, mu, var):
        """posteriors and statistics of X (host or device) under one mixture, in row batches -> (stats numpy, sum of lse)"""
        M = len(w)
        a, b, c = (torch.from_numpy(np.ascontiguousarray(t)).to(self.device) for t in expand(w, mu, var))
        stats = torch.zeros(M, 1 + 2 * self.D, dtype=F64, device=self.device)
        rows = max(64, self.batch_bytes // (8 * (self.D + M + 2) + 1))
        total = 0.0
        for i in range(0, X.shape[0], rows):
            x = X[i:i + rows].to(self.device)
            lse, post = loglik(x, a, b, c, 1, post=True)
            accumulate(post, x, stats)
            total += float(lse.cpu().numpy().sum())
        return stats.cpu().numpy(), total

    def fit_ubm(self, X):
        """The training schedule of the module docstring on pooled frames X (N, D) -> history, a list per doubling of the
        log-likelihood per frame each pass saw; the last list ends with the final model's."""
        X = self._frames(X)
        N, D = X.shape
        if N < 2:
            raise ValueError(f"{N} frames are too few to train on")
        Xh = X.cpu().numpy()
        mean = Xh.sum(0) / N
        gvar = ((Xh - mean) ** 2).sum(0) / N
        floor = self.var_floor * gvar
        w, mu, var = np.ones(1), mean[None].copy(), np.maximum(gvar, floor)[None]
        history = []
        while len(w) < self.components:
            sd = np.sqrt(var)
            w = np.repeat(w, 2) / 2.0
            mu = np.stack([mu + 0.2 * sd, mu - 0.2 * sd], 1).reshape(-1, D)
            var = np.repeat(var, 2, 0)
            stage = []
            for _ in range(self.iters):
                stats, total = self._pass(X, w, mu, var)
                stage.append(total / N)
                w, mu, var = self._m_step(stats, N, w, mu, var, floor)
            history.append(stage)
        _, total = self._pass(X, w, mu, var)
        if history:
            history[-1].append(total / N)
        else:
            history.append([total / N])
        self.w, self.mu, self.var, self.history = w, mu, var, history
        self.means, self.names, self._dev_tables = np.zeros((0,) + mu.shape), [], None
        return history

    def _m_step(self, stats, N, w, mu, var, floor):
        D = self.D
        n = stats[:, 0]
        ok = n >= self.min_occ
        safe = np.where(ok, n, 1.0)[:, None]
        m1 = stats[:, 1:1 + D] / safe
        w = np.where(ok, n / N, 0.0)
        mu = np.where(ok[:, None], m1, mu)
        var = np.where(ok[:, None], np.maximum(stats[:, 1 + D:1 + 2 * D] / safe - m1 * m1, floor), var)
        for m in np.nonzero(~ok)[0]:
            h = int(np.argmax(w))
            sd = np.sqrt(var[h])
            mu[m], mu[h] = mu[h] - 0.2 * sd, mu[h] + 0.2 * sd
            var[m] = var[h]
            w[m] = w[h] = w[h] / 2.0
        return w / w.sum(), mu, var

    def enrol(self, speakers):
        """speakers: [(name, frames (N_s, D))] -> the adapted means (S, M, D); replaces earlier enrolments"""
        if self.w is None:
            raise ValueError("enrol needs a trained UBM (fit_ubm or load)")
        means, names = [], []
        for name, X in speakers:
            stats, _ = self._pass(self._frames(X), self.w, self.mu, self.var)
            n = stats[:, :1]
            ex = np.where(n > 0, stats[:, 1:1 + self.D] / np.where(n > 0, n, 1.0), self.mu)
            alpha = n / (n + self.relevance) if self.relevance > 0 else (n > 0).astype(np.float64)
            means.append(alpha * ex + (1.0 - alpha) * self.mu)
            names.append(str(name))
        if len(set(names)) != len(names):
            raise ValueError("a speaker is enrolled twice")
        self.means, self.names, self._dev_tables = np.stack(means) if means else np.zeros((0,) + self.mu.shape), names, None
        return self.means

    def _scoring_tables(self):
        if self._dev_tables is None:
            ua, ub, uc = expand(self.w, self.mu, self.var)
            S = len(self.names)
            sa, _, sc = expand(self.w[None], self.means, self.var[None])
            up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(self.device)           # noqa: E731
            self._dev_tables = (up(ua), up(ub), up(uc), up(sa.reshape(-1, self.D)), up(np.tile(ub, (S, 1))), up(sc.reshape(-1)))
        return self._dev_tables

    def score(self, utterances):
        """utterances: [kept frames (n_u, D)] -> llr (U, S) numpy float64, a row of NaN for an utterance without frames"""
        S, M = len(self.names), self.components
        if not S:
            raise ValueError("no speaker is enrolled")
        ua, ub, uc, sa, sb, sc = self._scoring_tables()
        xs = [self._frames(x) for x in utterances]
        out = np.full((len(xs), S), np.nan)
        cost = lambda n, T: n * T * 8 * (self.D + S + 2)                                       # noqa: E731
        for batch in ragged.greedy_batches([(x.shape[0],) for x in xs], self.batch_bytes, cost):
            lens = [xs[i].shape[0] for i in batch]
            offs = [0] + list(np.cumsum(lens)[:-1])
            N = sum(lens)
            if N == 0:
                continue
            x = torch.cat([xs[i] for i in batch]).to(self.device)
            ubm = loglik(x, ua, ub, uc, 1)
            lse = loglik(x, sa, sb, sc, S)
            out[batch] = mean_rows(lse, ubm[:, 0], offs, lens).cpu().numpy()
        return out

    # ---- the file
    def save(self, path):
        if self.w is None:
            raise ValueError("nothing to save: no UBM has been trained")
        with open(path, "wb") as f:
            np.savez(f, format=np.int64(FORMAT), feature_config=np.array(json.dumps(self.feature_config, sort_keys=True)),
                     options=np.array(json.dumps(self.options(), sort_keys=True)), w=self.w, mu=self.mu, var=self.var,
                     means=self.means, names=np.array(self.names, dtype=np.str_),
                     history=np.array(json.dumps(self.history)))

    @classmethod
    def load(cls, path, device, feature_config=None, batch_bytes=1 << 30):
        """`feature_config`, when given, must be the model's: a model scores only the features it was trained on."""
        with np.load(path, allow_pickle=False) as z:
            if int(z["format"]) != FORMAT:
                raise ValueError(f"{path}: format {int(z['format'])}, this reader knows {FORMAT}")
            fc, opt = json.loads(str(z["feature_config"])), json.loads(str(z["options"]))
            if feature_config is not None and fc != feature_config:
                diff = ", ".join(f"{k} {feature_config.get(k)} (model: {(fc or {}).get(k)})" for k in sorted(set(feature_config) | set(fc or {}))
                                 if feature_config.get(k) != (fc or {}).get(k))
                raise ValueError(f"the config's feature settings are not the model's: {diff}")
            self = cls(device, feature_config=fc, batch_bytes=batch_bytes, **opt)
            self.w, self.mu, self.var, self.means = z["w"], z["mu"], z["var"], z["means"]
            self.names, self.history = [str(s) for s in z["names"]], json.loads(str(z["history"]))
        return self


# ------------------------------------------------------------------------------------------------ the corpus passes
def read_source(source):
    """`basename|speaker|...` lines -> [(basename, speaker)]"""
    out = []
    with open(source, encoding="utf-8") as f:
        for no, ln in enumerate(f, 1):
            if not ln.strip():
                continue
            parts = ln.strip("\n").split("|")
            if len(parts) < 2:
                raise ValueError(f"{source}:{no}: no speaker field")
            out.append((parts[0], parts[1]))
    return out


def wav_features(paths, fc, n_cep, energy_floor, device, batch_seconds=1800.0, num_workers=8):
    """[wav path] -> [kept normalised frames (n, D) float64 on the host, or None for a wav too short to frame]"""
    from . import audio as Audio
    from .preprocess import load_wav
    sr = fc["sampling_rate"]
    stft = Audio.TacotronSTFT(fc["filter_length"], fc["hop_length"], fc["win_length"], fc["n_mel"], sr, fc["fmin"], fc["fmax"])
    floor = default_energy_floor(fc["n_mel"]) if energy_floor is None else energy_floor

    def read(p):
        return np.clip(load_wav(p, sr), -1.0, 1.0).astype(np.float32)
    with ThreadPoolExecutor(max_workers=max(1, num_workers)) as pool:
        wavs = list(pool.map(read, paths))
    out = [None] * len(paths)
    ok = [i for i, w in enumerate(wavs) if len(w) > fc["filter_length"] // 2]
    staging = ragged.Staging()
    for batch in ragged.greedy_batches([(len(wavs[i]),) for i in ok], int(batch_seconds * sr), ragged.padded_samples):
        idx = [ok[i] for i in batch]
        staging.pack([wavs[i] for i in idx])
        mel, _, fr = stft.mel_spectrogram_ragged(staging.to(device), [len(wavs[i]) for i in idx])
        feat, offs, n_kept, _, _ = features(cepstra0(mel.contiguous(), fr.tolist(), n_cep), fr.tolist(), floor)
        feat, n_kept = feat.cpu(), n_kept.tolist()
        for r, i in enumerate(idx):
            out[i] = feat[offs[r]:offs[r] + n_kept[r]].clone()
    return out


def train(config, model_path, source, components=256, iters=4, relevance=16.0, n_cep=19, max_frames_per_speaker=20000, var_floor=0.01,
          min_occ=3.0, energy_floor=None, device="cuda", batch_bytes=1 << 30):
    """Train the UBM on `{raw_path}/{speaker}/{basename}.wav` for every line of `source`, enrol every speaker on the same pooled
    frames and write the model file -> (model, skipped [(basename, reason)])."""
    dev = ragged.require_device(torch.device(device), WHO)
    fc = feature_config(config)
    entries = read_source(source)
    order = []
    for _, s in entries:
        if s not in order:
            order.append(s)
    if len(order) < 2:
        raise ValueError(f"{source} names {len(order)} speaker(s): a UBM of a single speaker is that speaker, at least two are needed")
    raw = config["path"]["raw_path"]
    paths = [os.path.join(raw, s, n + ".wav") for n, s in entries]
    have = [i for i, p in enumerate(paths) if os.path.exists(p)]
    skipped = [(entries[i][0], "missing " + paths[i]) for i in range(len(entries)) if i not in set(have)]
    feats = wav_features([paths[i] for i in have], fc, n_cep, energy_floor, dev)
    pooled = {s: [] for s in order}
    for i, x in zip(have, feats):
        name, s = entries[i]
        if x is None or x.shape[0] == 0:
            skipped.append((name, "no frames kept"))
            continue
        room = max_frames_per_speaker - sum(t.shape[0] for t in pooled[s])
        if room > 0:
            pooled[s].append(x[:room])
    speakers = [(s, torch.cat(v)) for s, v in pooled.items() if v]
    if len(speakers) < 2:
        raise ValueError(f"only {len(speakers)} speaker(s) have frames: at least two are needed")
    model = SpeakerModel(dev, n_cep, components, iters, relevance, var_floor, min_occ, energy_floor, fc, batch_bytes)
    model.fit_ubm(torch.cat([x for _, x in speakers]))
    model.enrol(speakers)
    model.save(model_path)
    return model, skipped


def score(model_path, config, source, wav_dir, out_path=None, device="cuda", batch_bytes=1 << 30):
    """Score `{wav_dir}/{basename}.wav` for every line of `source` against the line's speaker -> (rows, missing, summary)."""
    dev = ragged.require_device(torch.device(device), WHO)
    model = SpeakerModel.load(model_path, dev, feature_config(config), batch_bytes)
    index = {s: g for g, s in enumerate(model.names)}
    entries, missing = [], []
    for name, s in read_source(source):
        path = os.path.join(wav_dir, name + ".wav")
        if s not in index:
            missing.append((name, f"speaker {s} is not in the model"))
        elif not os.path.exists(path):
            missing.append((name, "missing " + path))
        else:
            entries.append((name, s, path))
    feats = wav_features([e[2] for e in entries], model.feature_config, model.n_cep, model.energy_floor, dev)
    kept = [i for i, x in enumerate(feats) if x is not None and x.shape[0] > 0]
    missing += [(entries[i][0], "no frames kept") for i in range(len(entries)) if i not in set(kept)]
    llr = model.score([feats[i] for i in kept]) if kept else np.zeros((0, len(model.names)))
    rows = []
    for r, i in enumerate(kept):
        name, s, _ = entries[i]
        g = index[s]
        rank, rival, margin = rank_and_rival(llr[r], g)
        rows.append({"basename": name, "speaker": s, "llr": float(llr[r, g]), "rank": rank,
                     "rival": None if rival is None else model.names[rival], "margin": margin, "n_kept": int(feats[i].shape[0]),
                     "_row": llr[r], "_claimed": g})
    summary = summarize(rows, missing, model.names)
    for r in rows:
        del r["_row"], r["_claimed"]
    if out_path is not None:
        with open(out_path, "w", encoding="utf-8") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return rows, missing, summary
