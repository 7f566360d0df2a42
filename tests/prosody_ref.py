"""float64 numpy oracle of the prosody scores, written from the 'Prosody' section of fastspeech2_amd/metrics.py's docstring (not from
the kernels): the voiced contour and its moments, the sums along a warping path, the pitch-contour DTW (through tests/dtw_ref.py),
the per-pair scores, the pairwise merge of the moments and the corpus summary.  One pair at a time, plain loops."""
import math

import numpy as np

from tests import dtw_ref as R

NAN = float("nan")
CORR_FLOOR = 1e-24
SCORES = ("gpe", "ffe", "f0_corr", "f0_dtw_hz", "energy_mae", "energy_mae_rel")
WEIGHT = {"gpe": "n_voiced_pairs", "f0_corr": "n_voiced_pairs", "ffe": "path_len", "energy_mae": "path_len",
          "energy_mae_rel": "path_len", "f0_dtw_hz": "f0_dtw_path_len"}


def voiced(f0):
    """the frames with f0 > 0, in order"""
    f0 = np.asarray(f0, np.float64)
    return f0[f0 > 0.0]


def moments(u):
    """(n, mean, M2, M3, M4) of the values u: the mean first, then the central sums in a second pass; all 0 when there is none"""
    u = np.asarray(u, np.float64)
    n = len(u)
    if n == 0:
        return 0, 0.0, 0.0, 0.0, 0.0
    mean = float(np.sum(u)) / n
    d = u - mean
    return n, mean, float(np.sum(d ** 2)), float(np.sum(d ** 3)), float(np.sum(d ** 4))


def m3_scale(u):
    """sum |u - mean|^3: what the signed M3 is compared against"""
    u = np.asarray(u, np.float64)
    return float(np.sum(np.abs(u - np.mean(u)) ** 3)) if len(u) else 0.0


def merge(a, b):
    """Pebay's pairwise update: the (n, mean, M2, M3, M4) of the union of two disjoint sets"""
    (na, ma, a2, a3, a4), (nb, mb, b2, b3, b4) = a, b
    if na == 0 or nb == 0:
        return b if na == 0 else a
    n, delta = na + nb, mb - ma
    mean = ma + delta * nb / n
    m2 = a2 + b2 + delta ** 2 * na * nb / n
    m3 = a3 + b3 + delta ** 3 * na * nb * (na - nb) / n ** 2 + 3 * delta * (na * b2 - nb * a2) / n
    m4 = (a4 + b4 + delta ** 4 * na * nb * (na ** 2 - na * nb + nb ** 2) / n ** 3
          + 6 * delta ** 2 * (na ** 2 * b2 + nb ** 2 * a2) / n ** 2 + 4 * delta * (na * b3 - nb * a3) / n)
    return n, mean, m2, m3, m4


def merge_all(parts):
    acc = (0, 0.0, 0.0, 0.0, 0.0)
    for q in parts:
        acc = merge(acc, q)
    return acc


def shape(mom):
    """(n, mean, M2, M3, M4) -> (sigma, skewness, excess kurtosis): population moments"""
    n, _, m2, m3, m4 = mom
    if n == 0:
        return NAN, NAN, NAN
    sigma = math.sqrt(m2 / n)
    if sigma == 0.0:
        return 0.0, NAN, NAN
    return sigma, (m3 / n) / sigma ** 3, (m4 / n) / sigma ** 4 - 3.0


def path_sums(pi, pj, f0_ref, f0_syn, e_ref, e_syn):
    """the sums of one pair along its path"""
    f0_ref, f0_syn = np.asarray(f0_ref, np.float64), np.asarray(f0_syn, np.float64)
    r, s = f0_ref[np.asarray(pi)], f0_syn[np.asarray(pj)]
    a, b = np.asarray(e_ref)[np.asarray(pi)].astype(np.float64), np.asarray(e_syn)[np.asarray(pj)].astype(np.float64)
    both = (r > 0.0) & (s > 0.0)
    rv, sv = r[both], s[both]
    out = {"gross": int(np.sum(np.abs(sv - rv) > 0.2 * rv)), "n": int(both.sum()), "mism": int(np.sum((r == 0.0) != (s == 0.0))),
           "sxx": 0.0, "syy": 0.0, "sxy": 0.0, "de": float(np.sum(np.abs(a - b))), "se": float(np.sum(a))}
    if out["n"]:
        x, y = np.log(rv), np.log(sv)
        dx, dy = x - np.sum(x) / out["n"], y - np.sum(y) / out["n"]
        out["sxx"], out["syy"], out["sxy"] = float(np.sum(dx * dx)), float(np.sum(dy * dy)), float(np.sum(dx * dy))
    return out


def path_scores(q, P):
    n = q["n"]
    corr = n >= 2 and q["sxx"] > CORR_FLOOR * n and q["syy"] > CORR_FLOOR * n
    return {"gpe": q["gross"] / n if n else NAN, "ffe": (q["gross"] + q["mism"]) / P,
            "f0_corr": q["sxy"] / math.sqrt(q["sxx"] * q["syy"]) if corr else NAN, "energy_mae": q["de"] / P,
            "energy_mae_rel": q["de"] / q["se"] if q["se"] != 0.0 else NAN}


def contour_dtw(u, w):
    """-> (total, pi, pj) of the K = 1 DTW of two contours, (NaN, empty, empty) when one is empty"""
    u, w = np.asarray(u, np.float64), np.asarray(w, np.float64)
    if len(u) == 0 or len(w) == 0:
        return NAN, np.zeros(0, np.int32), np.zeros(0, np.int32)
    return R.dtw(u[:, None], w[:, None])


def stats_dict(mom):
    return dict(zip(("n", "mean", "m2", "m3", "m4"), mom))


def prosody(pi, pj, f0_ref, f0_syn, e_ref, e_syn):
    """the prosody keys of one pair's row from its path, F0 tracks and energies (all already cut to the pair's frame counts)"""
    row = path_scores(path_sums(pi, pj, f0_ref, f0_syn, e_ref, e_syn), len(pi))
    u, w = voiced(f0_ref), voiced(f0_syn)
    total, ci, _ = contour_dtw(u, w)
    row["f0_dtw_hz"] = total / len(ci) if len(ci) else NAN
    row["f0_dtw_path_len"] = len(ci)
    row["f0_stats_ref"], row["f0_stats_syn"] = stats_dict(moments(u)), stats_dict(moments(w))
    return row


def score_pair(mel_ref, mel_syn, f0_ref, f0_syn, e_ref, e_syn, K=13):
    """the whole row of one pair from its features; both sides are cut to min(mel frames, F0 frames) as dtw_ref.score_pair does"""
    T1, T2 = min(mel_ref.shape[1], len(f0_ref)), min(mel_syn.shape[1], len(f0_syn))
    total, pi, pj = R.dtw(R.cepstra(mel_ref[:, :T1], K), R.cepstra(mel_syn[:, :T2], K))
    row = R.scores(total, pi, pj, T1, T2, f0_ref[:T1], f0_syn[:T2])
    row.update(prosody(pi, pj, f0_ref[:T1], f0_syn[:T2], e_ref[:T1], e_syn[:T2]))
    return row


def summarize(rows):
    out = R.summarize(rows)
    if not rows or "gpe" not in rows[0]:
        return out
    for key in SCORES:
        good = [r for r in rows if not math.isnan(r[key])]
        out[key + "_nan_utterances"] = len(rows) - len(good)
        wsum = sum(float(r[WEIGHT[key]]) for r in good)
        out[key + "_mean"] = sum(r[key] for r in good) / len(good) if good else NAN
        out[key + "_weighted"] = sum(r[key] * float(r[WEIGHT[key]]) for r in good) / wsum if good and wsum > 0 else NAN
    for side in ("ref", "syn"):
        mom = merge_all([tuple(r["f0_stats_" + side][k] for k in ("n", "mean", "m2", "m3", "m4")) for r in rows])
        sigma, skew, kurt = shape(mom)
        out["f0_voiced_frames_" + side], out["f0_std_hz_" + side] = mom[0], sigma
        out["f0_skew_" + side], out["f0_kurt_" + side] = skew, kurt
    return out


# ------------------------------------------------------------------------------------------------ the end-to-end signals
FACTORS = (1.10, 1.30)
TONE_F0, TONE_DUR, TONE_GAP = (200.0, 170.0, 240.0, 140.0), (0.45, 0.3, 0.5, 0.35), 0.12


def tones(f0s, durs=TONE_DUR, gap=TONE_GAP):
    from tests import f0_signals as S
    parts = []
    for k, (f, d) in enumerate(zip(f0s, durs)):
        if k:
            parts.append(np.zeros(int(gap * S.FS), np.float32))
        parts.append(S.tone(f, d))
    return np.concatenate(parts)


def tone_pairs():
    """name -> (recorded, synthesized): an identical pair, and copies with every tone at 1.10 and at 1.30 times the frequency"""
    base = tones(TONE_F0)
    pairs = {"same": (base, base.copy())}
    for f in FACTORS:
        pairs["x%.2f" % f] = (base, tones([t * f for t in TONE_F0]))
    return pairs


def chain_features(wav):
    """(log-mel (n_mel, frames), F0 (frames,), energy (frames,) float32) of one waveform without the GPU: the oracle's STFT of the
    clamped audio, tests/f0_ref.py's DIO + StoneMask of the unclamped"""
    import torch
    from oracle.fs2_oracle import mel_spectrogram
    from tests import f0_ref, f0_signals as S
    mel, energy = mel_spectrogram(torch.from_numpy(np.clip(wav, -1.0, 1.0))[None])
    f0 = f0_ref.dio_stonemask(wav.astype(np.float64), S.FS, S.FRAME_PERIOD)[0]
    return mel[0].numpy().astype(np.float64), f0, energy[0].numpy().astype(np.float32)
