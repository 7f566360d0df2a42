"""CPU: Griffin-Lim mel inversion's host side.  tests/gl_ref.py (fp64) against the live reference's fp32 results
(tests/golden/griffin_lim.npz, made by tests/golden/make_golden_griffin_lim.py), the host-built bases and envelope against
the reference's, and the length limit enforced before anything reaches a device."""
import numpy as np
import pytest
import torch

from tests import gl_ref
from tests.helpers import load_golden

G64 = gl_ref.STFT(1024, 256, 1024)


def _angles(g, i):
    F = g[f"u{i}_spec"].shape[-1]
    np.random.seed(int(g[f"u{i}_seed"]))
    return np.angle(np.exp(2j * np.pi * np.random.rand(1, 513, F))).astype(np.float32)


def test_gl_ref_reproduces_the_reference_within_its_bars():
    from fastspeech2_amd.audio import slaney_mel_filterbank
    g = load_golden("griffin_lim")
    mel_basis = slaney_mel_filterbank(22050, 1024, 80, 0, 8000)
    for i in range(3):
        u = f"u{i}_"
        spec = g[u + "spec"]
        assert np.abs(gl_ref.spec_from_mel(g[u + "mel"], mel_basis)[None, :, :-1] - spec).max() <= g[f"bar_spec_{i}"]
        ang = _angles(g, i)
        if u + "angles" in g:
            assert np.array_equal(ang, g[u + "angles"])                 # the seeded draw is the reference's
        for n in (0, 1, 2):
            if u + f"sig{n}" in g:
                ref = g[u + f"sig{n}"]
                got = gl_ref.griffin_lim(spec, G64, n, ang)
                assert got.shape == ref.shape == (1, 256 * (spec.shape[-1] - 1))
                assert np.abs(got - ref).max() <= g[f"bar_sig{n}_{i}"], (i, n)
        if u + "mag" in g:
            mag, phase = G64.transform(g[u + "sig0"])
            assert np.abs(mag - g[u + "mag"]).max() <= g[f"bar_mag_{i}"]
            keep = mag > 1e-3 * mag.max()
            assert gl_ref.phase_distance(phase, g[u + "phase"])[keep].max() <= g[f"bar_phase_{i}"]
        assert 0.05 < float(g[u + "sc60"]) < 0.5


def test_host_bases_and_envelope_equal_the_reference():
    from fastspeech2_amd.audio import STFT, dft_basis, inverse_basis, window_sumsquare
    g = load_golden("griffin_lim")
    inv = inverse_basis(1024, 256, 1024)
    assert inv.dtype == torch.float32 and inv.shape == (1026, 1024)
    np.testing.assert_allclose(inv[::101].numpy(), g["inverse_basis_rows"], rtol=0, atol=1e-9)
    assert np.array_equal(window_sumsquare("hann", 17, 256, 1024, 1024), g["window_sum_17"])
    # the kernels rebuild the envelope per sample: frames in increasing order, each add in double rounded to float32
    s = STFT(1024, 256, 1024)
    w2 = s.win_sq.numpy()
    env = np.zeros(256 * 16 + 1024, dtype=np.float32)
    for t in range(env.size):
        for f in range(max(0, (t - 1024) // 256 + 1), min(16, t // 256) + 1):
            env[t] = np.float32(np.float64(env[t]) + w2[t - 256 * f])
    assert np.array_equal(env, g["window_sum_17"])
    # packed operands: forward (2*cutoff, taps, hop) of the mel path's basis, inverse W[n][0][c] = inverse_basis[c][n], zero K pad
    assert torch.equal(s.forward_basis.view(1026, 1024), dft_basis(1024, 1024))
    assert s.inverse_weight.shape == (1024, 1, 1028)
    assert torch.equal(s.inverse_weight[:, 0, :1026], inv.t()) and not s.inverse_weight[:, 0, 1026:].any()


def test_too_short_is_rejected_before_any_device_call(tmp_path):
    from fastspeech2_amd.audio import STFT, TacotronSTFT, griffin_lim, inv_mel_spec, mels_to_wavs_griffin_lim
    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    assert stft._stft_fn is stft.stft_fn and isinstance(stft.stft_fn, STFT)
    with pytest.raises(ValueError):
        griffin_lim(torch.zeros(1, 513, 3), stft.stft_fn, 2)                    # F = 3: hop*(F-1) = 512 is not > 512
    with pytest.raises(ValueError):
        mels_to_wavs_griffin_lim(torch.zeros(2, 80, 12), [12, 4], stft, 2)      # mel_len 4 -> F = 3
    with pytest.raises(ValueError):
        inv_mel_spec(torch.zeros(80, 4), str(tmp_path / "x.wav"), stft, 2)
    assert not (tmp_path / "x.wav").exists()
    with pytest.raises(RuntimeError, match="AMD GPU only"):                     # long enough: CPU tensors are refused
        griffin_lim(torch.zeros(1, 513, 4), stft.stft_fn, 2)
