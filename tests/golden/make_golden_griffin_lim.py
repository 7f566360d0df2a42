"""Generate tests/golden/griffin_lim.npz by running the LIVE reference's Griffin-Lim mel inversion (audio/stft.py STFT,
audio/audio_processing.py griffin_lim / window_sumsquare, audio/tools.py inv_mel_spec) on the CPU.  Run in the build
container only (the GPU box has no reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_griffin_lim.py

librosa (absent here) is stubbed as in make_golden.case_stft: pad_center, tiny, util.normalize(norm=None) = identity, and
filters.mel = the Slaney table whose checksum tests/golden/mel_filterbank.json records.  `.cuda()` is neutralised and
scipy's wavfile.write is captured.  Nothing is copied from the reference: it is imported and executed.

Three utterances, mel frames T = 5 / 18 / 101 (F = T - 1 = 4, the minimum / 17, odd / 100 Griffin-Lim frames), log-mels of
the reference's own TacotronSTFT.mel_spectrogram over the LJSpeech demo clip.  Per utterance u<i>_*: mel, seed (numpy's
global generator is seeded with it right before the reference draws its initial angles), spec (spec_from_mel[:, :, :-1]:
the Griffin-Lim target), sig0 (the signal after 0 iterations = STFT.inverse(spec, angles)) and sc60 (spectral convergence of
the 60-iteration signal, measured with tests/gl_ref.py's fp64 STFT).  The two shorter utterances also carry their angles,
sig1 / sig2 (after 1, 2 iterations) and transform (magnitude, phase) of sig0; the longest one's angles are regenerated from
its seed (the size budget: ~500 KB).  inv_wav: inv_mel_spec(u1 mel, griffin_iters=2) as written.  inverse_basis_rows: every 101st row.
bar_<quantity>: 4 x max |reference fp32 - gl_ref fp64| + a floor of 2^-20 max |fp64|."""
import hashlib
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fastspeech2_amd.audio import slaney_mel_filterbank  # noqa: E402
from tests import gl_ref  # noqa: E402

torch.set_num_threads(8)
FRAMES = (5, 18, 101)
SEEDS = (11, 12, 13)
OFFSETS = (20000, 40000, 60000)


def _stub_librosa():
    table = slaney_mel_filterbank(22050, 1024, 80, 0, 8000)
    ref = json.load(open(os.path.join(HERE, "mel_filterbank.json")))
    assert hashlib.sha256((table + np.float32(0)).tobytes()).hexdigest() == ref["sha256_float32_le"]
    lib = types.ModuleType("librosa")
    util = types.ModuleType("librosa.util")
    filt = types.ModuleType("librosa.filters")

    def pad_center(data, size, axis=-1):
        n = data.shape[axis]
        lpad = (size - n) // 2
        return np.pad(data, (lpad, size - n - lpad))
    util.pad_center = pad_center
    util.tiny = lambda x: np.finfo(np.float32).tiny
    util.normalize = lambda x, norm=None: x
    filt.mel = lambda sr, n_fft, n_mels, fmin, fmax: table
    lib.util, lib.filters = util, filt
    sys.modules.update({"librosa": lib, "librosa.util": util, "librosa.filters": filt})


def _bar(ref32, ref64, dist=None):
    d = np.abs(np.asarray(ref32, np.float64) - ref64) if dist is None else dist
    return float(4.0 * d.max() + 2.0 ** -20 * np.abs(ref64).max())


def main():
    _stub_librosa()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    written = {}
    try:
        from audio import tools
        from audio.audio_processing import griffin_lim
        from audio.audio_processing import window_sumsquare
        from audio.stft import TacotronSTFT
        from scipy.io import wavfile

        tools.write = lambda path, rate, data: written.update(path=path, rate=rate, data=np.array(data))
        stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
        stft._stft_fn = stft.stft_fn                        # tools.py:28 reads `_stft_fn`; the class defines `stft_fn`
        fn = stft.stft_fn
        g64 = gl_ref.STFT(1024, 256, 1024)
        mel_basis = stft.mel_basis.numpy()
        sr, wav = wavfile.read(os.path.join(REF, "demo", "LJSpeech", "LJ001-0012_ground-truth.wav"))
        assert sr == 22050
        out = {"inverse_basis_rows": fn.inverse_basis[::101, 0, :].numpy()}
        out["window_sum_17"] = window_sumsquare("hann", 17, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
        for i, (T, seed, off) in enumerate(zip(FRAMES, SEEDS, OFFSETS)):
            u = f"u{i}_"
            y = torch.from_numpy(wav[off:off + 256 * (T - 1)].astype(np.float32) / 32768.0).unsqueeze(0)
            mel, _ = stft.mel_spectrogram(y)
            mel = mel[0]
            assert mel.shape == (80, T)
            spec = (torch.mm(stft.spectral_de_normalize(mel.unsqueeze(0)).transpose(1, 2)[0], stft.mel_basis).t().unsqueeze(0)
                    * 1000)[:, :, :-1]                        # tools.py:19-26 + the [:, :, :-1] of tools.py:27
            spec64 = gl_ref.spec_from_mel(mel.numpy(), mel_basis)[None, :, :-1]
            F = T - 1
            np.random.seed(seed)
            angles = np.angle(np.exp(2j * np.pi * np.random.rand(1, 513, F))).astype(np.float32)
            sigs = {}
            for n in (0, 1, 2, 60):
                np.random.seed(seed)
                sigs[n] = griffin_lim(spec, fn, n).numpy()
            mag, phase = fn.transform(torch.from_numpy(sigs[0]))
            mag64, phase64 = g64.transform(sigs[0])
            out.update({u + "mel": mel.numpy(), u + "seed": np.int64(seed), u + "spec": spec.numpy(),
                        u + "sc60": gl_ref.spectral_convergence(sigs[60], spec.numpy(), g64),
                        f"bar_spec_{i}": _bar(spec.numpy(), spec64)})
            for n in ((0, 1, 2) if i < 2 else (0,)):
                out[u + f"sig{n}"] = sigs[n]
                out[f"bar_sig{n}_{i}"] = _bar(sigs[n], gl_ref.griffin_lim(spec.numpy(), g64, n, angles))
            if i < 2:
                keep = mag64 > 1e-3 * mag64.max()
                out.update({u + "angles": angles, u + "mag": mag.numpy(), u + "phase": phase.numpy(),
                            f"bar_mag_{i}": _bar(mag.numpy(), mag64),
                            f"bar_phase_{i}": _bar(None, phase64, gl_ref.phase_distance(phase.numpy(), phase64)[keep])})
            print(f"u{i}: F={F} spec max {float(spec.max()):.3g} sig0 max {np.abs(sigs[0]).max():.3g} sc60 {out[u + 'sc60']:.4f} "
                  f"bar sig0 {out[f'bar_sig0_{i}']:.3g}")
        np.random.seed(SEEDS[1])
        tools.inv_mel_spec(torch.from_numpy(out["u1_mel"]), "inv.wav", stft, griffin_iters=2)
        assert written["rate"] == 22050 and written["data"].dtype == np.float32
        out["inv_wav"] = written["data"]
    finally:
        torch.Tensor.cuda = real_cuda
    path = os.path.join(HERE, "griffin_lim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    os.chdir(REF)
    main()
