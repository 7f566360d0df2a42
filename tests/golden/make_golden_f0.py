"""Writes tests/golden/f0_speech.npz: a 3 s int16 excerpt of an LJSpeech ground-truth demo wav of the reference
(demo/LJSpeech/LJ001-0012_ground-truth.wav), the real-speech input of tests/test_f0_gpu.py.  Run from the repository root with
the reference tree's path: `python tests/golden/make_golden_f0.py <reference root>`.  The GPU test reads only the fixture."""
import os
import sys

import numpy as np
from scipy.io import wavfile

if __name__ == "__main__":
    sr, w = wavfile.read(os.path.join(sys.argv[1], "demo", "LJSpeech", "LJ001-0012_ground-truth.wav"))
    if w.dtype != np.int16:
        w = np.clip(np.round(w.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    start = int(0.5 * sr)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "f0_speech.npz"),
                        wav=w[start:start + 3 * sr], sr=np.int64(sr))
