"""Known-answer signals of the F0 tests (tests/test_f0_cpu.py, tests/test_f0_gpu.py)."""
import os

import numpy as np

FS, HOP = 22050, 256
FRAME_PERIOD = HOP / FS * 1000
TONE_F0 = (80, 110, 150, 200, 260, 330, 450, 600)


def tone(f0, dur=1.0, amp=0.5, fs=FS):
    """5 harmonics, amplitude 1/k, constant F0"""
    t = np.arange(int(dur * fs)) / fs
    return (amp / 2 * sum(np.sin(2 * np.pi * f0 * k * t + 0.3 * k) / k for k in range(1, 6))).astype(np.float32)


def glide(f_start=110.0, f_end=220.0, dur=1.5, fs=FS):
    """exponential glide: (signal, true F0 at each sample time)"""
    t = np.arange(int(dur * fs)) / fs
    k = np.log(f_end / f_start) / dur
    phase = 2 * np.pi * f_start * (np.exp(k * t) - 1) / k
    x = 0.25 * sum(np.sin(h * phase) / h for h in range(1, 6))
    return x.astype(np.float32), lambda tt: f_start * np.exp(k * tt)


def tones_with_silence(f0s=(200, 260, 150), gap=0.3):
    parts = []
    for i, f in enumerate(f0s):
        if i:
            parts.append(np.zeros(int(gap * FS), np.float32))
        parts.append(tone(f))
    return np.concatenate(parts)


def interior(t, n, margin=0.05, fs=FS):
    return (t >= margin) & (t <= n / fs - margin)


def far_from_signal(x, t, dist=0.06, fs=FS):
    """frames whose centre is more than `dist` s from any non-zero sample"""
    nz = np.nonzero(x)[0] / fs
    return np.array([np.min(np.abs(nz - ti)) > dist for ti in t])


def speech():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f0_speech.npz"))
    return (d["wav"].astype(np.float32) / 32768.0), int(d["sr"])
