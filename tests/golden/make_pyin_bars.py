"""Writes tests/golden/pyin_bars.json: what the numpy oracle tests/pyin_ref.py measures on the known-answer signals of
tests/f0_signals.py, for tests/test_pyin_cpu.py (pins on the oracle) and tests/test_pyin_gpu.py (bars for the kernels).  Nothing here
touches the shared library.

    python tests/golden/make_pyin_bars.py

- bin_width: 2^(1 / 240) - 1, the relative width of one pitch bin: what the quantisation of the output alone allows.
- oracle_error[signal]: the oracle's worst relative F0 error over the signal's interior frames (all of which it must find voiced).
- bar[signal]: bin_width where the oracle is within it, else oracle_error + bin_width.
- silence_voiced[signal]: the oracle's voiced / unvoiced decision on every frame of the signals that hold digital silence:
  `tones_with_silence` (0.3 s gaps), `long_gap` (a 1 s gap) and `trailing_zeros` (a tone followed by 1.5 s of zeros).  Exact zeros
  give a flat d', which by the specification carries no candidate: however long the silence, it stays unvoiced."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import f0_signals as S                                           # noqa: E402

BARS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pyin_bars.json")
BIN_WIDTH = 2.0 ** (1.0 / 240.0) - 1.0
SILENCE_F0, SILENCE_GAP = (200, 260, 150), 0.3
LONG_F0, LONG_GAP, TRAILING_F0, TRAILING_ZEROS = (200, 260), 1.0, 200, 1.5
SILENT = ("tones_with_silence", "long_gap", "trailing_zeros")


def known_answers():
    """[(name, waveform, truth)]: truth(t) -> the true F0 at the frame times t, 0 where the frame is not an interior one"""
    out = []
    for f in S.TONE_F0:
        x = S.tone(f)
        out.append((f"tone{f}", x, lambda t, f=f, n=len(x): np.where(S.interior(t, n), float(f), 0.0)))
    x, true = S.glide()
    out.append(("glide", x, lambda t, n=len(x), true=true: np.where(S.interior(t, n), true(t), 0.0)))

    def segments(f0s, gap):
        def truth(t):
            v = np.zeros(len(t))
            for i, f in enumerate(f0s):
                a = i * (1.0 + gap)
                v[(t >= a + 0.05) & (t <= a + 1.0 - 0.05)] = f
            return v
        return truth
    out.append(("tones_with_silence", S.tones_with_silence(SILENCE_F0, SILENCE_GAP), segments(SILENCE_F0, SILENCE_GAP)))
    out.append(("long_gap", S.tones_with_silence(LONG_F0, LONG_GAP), segments(LONG_F0, LONG_GAP)))
    x = np.concatenate([S.tone(TRAILING_F0), np.zeros(int(TRAILING_ZEROS * S.FS), np.float32)])
    out.append(("trailing_zeros", x, segments((TRAILING_F0,), 0.0)))
    return out


def worst_error(f0, truth):
    """(every interior frame voiced, worst relative error over them)"""
    m = truth > 0
    return bool(np.all(f0[m] > 0)), float(np.abs(f0[m] / truth[m] - 1).max())


def load_bars():
    with open(BARS_PATH) as f:
        return json.load(f)


def main():
    from tests import pyin_ref as R
    out = {"bin_width": BIN_WIDTH, "oracle_error": {}, "bar": {}, "silence_voiced": {}}
    for name, x, truth in known_answers():
        f0, _, t = R.pyin(x, S.FS, S.FRAME_PERIOD)
        voiced, err = worst_error(f0, truth(t))
        assert voiced, name
        out["oracle_error"][name] = err
        out["bar"][name] = BIN_WIDTH if err <= BIN_WIDTH else err + BIN_WIDTH
        if name in SILENT:
            out["silence_voiced"][name] = "".join(str(int(v > 0)) for v in f0)
    with open(BARS_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "silence_voiced"}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
