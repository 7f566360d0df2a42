"""Writes tests/golden/world_bars.json: what the numpy oracle tests/world_ref.py measures on the CPU, for tests/test_world_cpu.py
(regression pins on the oracle) and tests/test_world_gpu.py (bars for the kernels).  Nothing here touches the shared library.

    python tests/golden/make_world_bars.py

- envelope_rms_db: the oracle's RMS distance in dB from the known filter, per pitch (tests/world_cases.envelope_error_db).
- mcd_world_db / mcd_mel_db: the 120 / 220 Hz same-filter pair scored on spectral-envelope mel-cepstra and on the mel-DCT.
- ln_envelope_bar[case]: FACTOR x the largest elementwise distance in ln(envelope), over every frame of the GPU test's inputs,
  between the oracle run with np.fft and the same oracle run with explicit DFT-matrix products: two summation orders of the same
  fp64 quantity.  mcep_bar[case][K, alpha]: the same for the mel-cepstra c~_1 .. c~_K."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import world_cases as C                                          # noqa: E402
from tests import world_ref as W                                            # noqa: E402

FACTOR = 16
MCEP_CASES = [(24, 0.455), (40, 0.455), (24, 0.0), (40, 0.0)]


def distances(fs, frame_period, rows, f0):
    mat = W.MatrixFft()
    env_d, cep_d = 0.0, {f"{K},{a}": 0.0 for K, a in MCEP_CASES}
    for x, f in zip(rows, f0):
        e1, e2 = W.envelope(x, f, fs, frame_period), W.envelope(x, f, fs, frame_period, mat)
        env_d = max(env_d, float(np.abs(np.log(e1) - np.log(e2)).max()))
        for K, a in MCEP_CASES:
            d = np.abs(W.mel_cepstra(e1, K, a) - W.mel_cepstra(e2, K, a, fft=mat)).max()
            cep_d[f"{K},{a}"] = max(cep_d[f"{K},{a}"], float(d))
    return env_d, cep_d


def main():
    out = {"factor": FACTOR, "envelope_rms_db": {str(int(f)): C.envelope_error_db(f) for f in C.PITCHES}}
    world, mel, F, P = C.pair_mcds()
    out.update(mcd_world_db=world, mcd_mel_db=mel, pair_frames=F, pair_path_len=P)
    out["ln_envelope_distance"], out["ln_envelope_bar"], out["mcep_distance"], out["mcep_bar"] = {}, {}, {}, {}
    rows, f0 = C.ragged_case()
    fs, fp, wrows, wf0 = C.wide_case()
    for name, args in (("22050", (C.FS, C.FRAME_PERIOD, rows, f0)), ("48000", (fs, fp, wrows, wf0))):
        env_d, cep_d = distances(*args)
        out["ln_envelope_distance"][name], out["ln_envelope_bar"][name] = env_d, FACTOR * env_d
        out["mcep_distance"][name], out["mcep_bar"][name] = cep_d, {k: FACTOR * v for k, v in cep_d.items()}
    with open(C.BARS_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
