"""Seeded inputs of the per-kernel Griffin-Lim tests (tests/test_griffin_lim_kernels_gpu.py), shared with the script that measures
their bars (tests/golden/make_gl_kernel_bars.py) and with tests/test_griffin_lim_cpu.py, which regenerates them.  numpy only.

A bar is FACTOR x the largest distance, over a case's inputs, between tests/gl_ref.py evaluated in float32 and in fp64, normalised
as the GPU test normalises its own error:
    recombine, project   |dG| / |m|                   per unit of the entry's magnitude
    mag_phase            |dmag| / mag and |dphase|    relative, and radians
    ola                  |d| / ola(|seg|)             per unit of the same overlap-add of the absolute values (the samples just
                                                      inside a window's edge divide by an envelope of 1e-5 and are 1e5 x larger)
and written with 4 significant digits, so that the last bits of a platform's fp64 cos do not reach the file."""
import json
import os

import numpy as np

from tests import gl_ref

BARS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gl_kernel_bars.json")
FACTOR = 4
SIZES = [(16, 4), (256, 64), (1024, 256)]                           # NF = 9, 129, 513: ldg below one block, just over one, over four
FMAX = 6
FRAMES = [0, 1, FMAX, FMAX + 3, 2]
OLA_SETTINGS = [(1024, 256, 1024), (1024, 256, 256), (256, 64, 200), (64, 64, 64), (16, 4, 16), (24, 10, 24)]
BIG_ROWS, BIG_NF = 65540, 9
PI32 = np.float32(np.pi)


def bars():
    with open(BARS_PATH) as f:
        return json.load(f)


def nf_of(filt):
    return filt // 2 + 1


# ---------------------------------------------------------------------------------------------- mag_phase
# (re, im) planted at bins 0 .. 8 of two frames, and what the kernel must make of the exact ones
PLANTED = [(0.0, 0.0), (-3.5, 0.0), (-3.5, -0.0), (0.0, 2.25), (0.0, -2.25), (1e-15, 0.0), (6e14, -8e14), (-6e-16, 8e-16), (0.0, 1e15)]


def mag_phase_case(NF, B=2, F=7):
    """ft values (B, F, 2 NF) float32: normal x 10^U(-3, 3), with PLANTED at bins 0 .. 8 of frame (0, 0) and of frame (B-1, F-1)"""
    rng = np.random.RandomState(100 + NF)
    ft = (rng.standard_normal((B, F, 2 * NF)) * 10.0 ** rng.uniform(-3, 3, (B, F, 2 * NF))).astype(np.float32)
    for b, f in ((0, 0), (B - 1, F - 1)):
        for k, (re, im) in enumerate(PLANTED):
            ft[b, f, k], ft[b, f, NF + k] = re, im
    return ft


# ---------------------------------------------------------------------------------------------- recombine / project
def mag_case(NF, B=len(FRAMES), Fmax=FMAX, seed=0):
    rng = np.random.RandomState(200 + NF + seed)
    mag = np.exp(rng.standard_normal((B, Fmax, NF))).astype(np.float32)
    mag[:, 0, 5] = 0.0
    return mag


def phase_case(NF, B=len(FRAMES), Fmax=FMAX):
    """uniform in [-pi, pi]; bins 0 .. 4 of every utterance's first frame hold 20, -20, pi, -pi, 0"""
    rng = np.random.RandomState(300 + NF)
    ph = rng.uniform(-np.pi, np.pi, (B, Fmax, NF)).astype(np.float32)
    ph = np.clip(ph, -PI32, PI32)
    ph[:, 0, :5] = [20.0, -20.0, PI32, -PI32, 0.0]
    return ph


def ft_case(NF, B=len(FRAMES), Fmax=FMAX):
    """forward-DFT rows (B, S = Fmax + 2, 2 NF) for project; bins 0 .. 2 of every utterance's first frame are (0, 0), (-x, +0), (0, y)"""
    rng = np.random.RandomState(400 + NF)
    ft = rng.standard_normal((B, Fmax + 2, 2 * NF)).astype(np.float32)
    ft[:, 0, :3] = [0.0, -1.5, 0.0]
    ft[:, 0, NF:NF + 3] = [0.0, 0.0, 0.75]
    return ft


def big_case():
    """BIG_ROWS rows of NF = 9: (mag, phase, ft) as (1, BIG_ROWS, .) and the rows compared (first, last, 100 seeded)"""
    rng = np.random.RandomState(65540)
    mag = np.exp(rng.standard_normal((1, BIG_ROWS, BIG_NF))).astype(np.float32)
    ph = np.clip(rng.uniform(-np.pi, np.pi, (1, BIG_ROWS, BIG_NF)).astype(np.float32), -PI32, PI32)
    ft = rng.standard_normal((1, BIG_ROWS, 2 * BIG_NF)).astype(np.float32)
    rows = np.unique(np.concatenate([[0, BIG_ROWS - 1], rng.randint(0, BIG_ROWS, 100)]))
    return mag, ph, ft, rows


# ---------------------------------------------------------------------------------------------- ola
def ola_case(filt, hop, win):
    """seg (B, Fmax, filt) float32 normal, one row per frame count of: 0, 1, 2, the largest F with hop (F - 1) <= filt / 2, the
    smallest with hop (F - 1) > filt / 2, Fmax, and one above Fmax (clamped); leading dimensions larger than they have to be"""
    Fs = (filt // 2) // hop + 1
    Fmax = Fs + 6
    frames = [0, 1, 2, Fs, Fs + 1, Fmax, Fmax + 2]
    rng = np.random.RandomState(filt * 7 + hop * 3 + win)
    seg = rng.standard_normal((len(frames), Fmax, filt)).astype(np.float32)
    return {"seg": seg, "frames": frames, "Fmax": Fmax, "win_sq": gl_ref.window(win, filt) ** 2, "lds": filt + 4,
            "row_len": hop * (Fmax - 1) + filt + 5, "ldy": hop * (Fmax - 1) + 3}


def ola_ref(c, filt, hop, dtype=np.float64, absolute=False):
    seg = np.abs(c["seg"]) if absolute else c["seg"]
    return gl_ref.ola(seg, c["frames"], c["win_sq"], filt, hop, c["row_len"], c["ldy"], dtype=dtype)


# ---------------------------------------------------------------------------------------------- mel -> magnitude
def mel_case(n_mel, NF, T):
    """log-mel (4, n_mel, T) float32 for mel_lens = [0, 1, 2, T], a filterbank (n_mel, NF) whose filter j is non-zero on
    span[j] = [lo, hi) and holds 7 outside it (a kernel that ignored the spans would add that), bins 0 and NF - 2 .. NF - 1 inside
    no span.  -> (mel, lens, basis, span)"""
    rng = np.random.RandomState(500 + n_mel)
    mel = rng.normal(-2.0, 2.0, (4, n_mel, T)).astype(np.float32)
    lo = rng.randint(1, NF - 3, n_mel)
    hi = np.minimum(lo + rng.randint(0, 6, n_mel), NF - 2)                  # some spans are empty
    basis = np.full((n_mel, NF), 7.0, dtype=np.float32)
    for j in range(n_mel):
        basis[j, lo[j]:hi[j]] = rng.uniform(0.0, 0.05, hi[j] - lo[j])
    return mel, [0, 1, 2, T], basis, np.stack([lo, hi], axis=1).astype(np.int32)


def mel_ref(mel, lens, basis, span):
    """-> (mag (B, Fmax, NF) fp64, bound (B, Fmax, NF)).  A bin's sum has n terms, one per filter whose span holds it, added by
    fmaf in any order: within n u of sum |e_j w_jk| (u = 2^-24); each e_j = expf(mel) is within 2 ulp = 4 u of exp (HIP's stated
    accuracy is 1 ulp), the x 1000 rounds once more: (n + 6) u * 1000 * sum e_j w_jk, all terms non-negative."""
    mel, basis = np.asarray(mel, np.float64), np.asarray(basis, np.float64)
    B, n_mel, T = mel.shape
    NF = basis.shape[1]
    k = np.arange(NF)
    inside = (k[None, :] >= span[:, :1]) & (k[None, :] < span[:, 1:])        # (n_mel, NF)
    w = np.where(inside, basis, 0.0)
    mag = np.zeros((B, T - 1, NF))
    for b, n in enumerate(lens):
        F = min(max(n - 1, 0), T - 1)
        mag[b, :F] = 1000.0 * np.exp(mel[b, :, :F]).T @ w
    return mag, (inside.sum(0)[None, None, :] + 6) * 2.0 ** -24 * mag


# ---------------------------------------------------------------------------------------------- the bars
def _r(x):
    return float(f"{FACTOR * float(x):.4g}")


def _per_unit(d, unit):
    keep = unit > 0
    return np.abs(d)[keep] / unit[keep]


def measure():
    """what tests/golden/gl_kernel_bars.json holds"""
    out = {"factor": FACTOR, "mag_rel": {}, "phase": {}, "recombine": {}, "project": {}, "ola": {}}
    for filt, _ in SIZES:
        NF = nf_of(filt)
        ft = mag_phase_case(NF)
        (m32, p32), (m64, p64) = gl_ref.mag_phase(ft, np.float32), gl_ref.mag_phase(ft)
        out["mag_rel"][str(NF)] = _r(_per_unit(m32 - m64, m64).max())
        out["phase"][str(NF)] = _r(np.abs(p32 - p64).max())
        mag, ph, ftp = mag_case(NF), phase_case(NF), ft_case(NF)
        unit = np.concatenate([mag, mag], axis=2).astype(np.float64)
        out["recombine"][str(NF)] = _r(_per_unit(gl_ref.recombine(mag, ph, dtype=np.float32) - gl_ref.recombine(mag, ph), unit).max())
        out["project"][str(NF)] = _r(_per_unit(gl_ref.project(ftp, mag, dtype=np.float32) - gl_ref.project(ftp, mag), unit).max())
    mag, ph, ft, _ = big_case()
    unit = np.concatenate([mag, mag], axis=2).astype(np.float64)
    out["recombine"]["big"] = _r(_per_unit(gl_ref.recombine(mag, ph, dtype=np.float32) - gl_ref.recombine(mag, ph), unit).max())
    out["project"]["big"] = _r(_per_unit(gl_ref.project(ft, mag, dtype=np.float32) - gl_ref.project(ft, mag), unit).max())
    (m32, p32), (m64, p64) = gl_ref.mag_phase(ft, np.float32), gl_ref.mag_phase(ft)
    out["mag_rel"]["big"], out["phase"]["big"] = _r(_per_unit(m32 - m64, m64).max()), _r(np.abs(p32 - p64).max())
    for filt, hop, win in OLA_SETTINGS:
        c = ola_case(filt, hop, win)
        o32, o64, unit = ola_ref(c, filt, hop, np.float32), ola_ref(c, filt, hop), ola_ref(c, filt, hop, absolute=True)
        out["ola"][f"{filt},{hop},{win}"] = _r(max(_per_unit(a - b, u).max() for a, b, u in zip(o32, o64, unit)))
    return out
