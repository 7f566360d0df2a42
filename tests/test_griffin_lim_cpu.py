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


# ---------------------------------------------------------------------------------------------- the per-kernel oracle
@pytest.mark.parametrize("setting", [(256, 64, 200), (1024, 256, 1024)])
def test_kernel_contracts_compose_to_the_reference_functions(setting):
    """ola(recombine(...) @ inverse_basis) is STFT.inverse and mag_phase(frames @ forward_basis^T) is STFT.transform, in fp64"""
    filt, hop, win = setting
    s = gl_ref.STFT(filt, hop, win)
    rng = np.random.RandomState(filt + win)
    B, F, NF = 2, 9, filt // 2 + 1
    mag, ph = np.exp(rng.standard_normal((B, NF, F))), rng.uniform(-np.pi, np.pi, (B, NF, F))
    want = s.inverse(mag, ph)
    G = gl_ref.recombine(mag.transpose(0, 2, 1), ph.transpose(0, 2, 1), ldg=2 * NF + 2)
    assert not G[..., 2 * NF:].any()
    N = hop * (F - 1)
    xp, y = gl_ref.ola(G[..., :2 * NF] @ s.inverse_basis, None, gl_ref.window(win, filt) ** 2, filt, hop, N + filt + 3, N + 2)
    assert np.abs(y[:, :N] - want).max() <= 1e-12 * np.abs(want).max() and not y[:, N:].any()
    assert np.array_equal(xp[:, :N + filt], np.pad(y[:, :N], ((0, 0), (filt // 2, filt // 2)), mode="reflect")) and not xp[:, N + filt:].any()
    x = rng.standard_normal((B, N))
    wm, wp = s.transform(x)
    gm, gp = gl_ref.mag_phase(s.frames_of(x) @ s.forward_basis.T)
    assert gm.shape == wm.shape == (B, NF, F)
    assert np.abs(gm - wm).max() <= 1e-12 * np.abs(wm).max() and np.abs(gp - wp).max() <= 1e-12 * np.pi
    # project = recombine of the transform's phase, and ragged rows are zero whatever lies there
    ft = s.frames_of(x) @ s.forward_basis.T
    m = mag.transpose(0, 2, 1)
    assert np.array_equal(gl_ref.project(ft, m), gl_ref.recombine(m, gp.transpose(0, 2, 1)))
    poisoned = m.copy()
    poisoned[1, 4:] = np.nan
    Gr = gl_ref.project(ft, poisoned, frames=[F + 3, 4])
    assert np.array_equal(Gr[0], gl_ref.project(ft, m)[0]) and np.array_equal(Gr[1, :4], gl_ref.project(ft, m)[1, :4]) and not Gr[1, 4:].any()
    # the float32 evaluation: the reference's casts, a float32 result, within float32 rounding of the fp64 one
    s32 = gl_ref.STFT(filt, hop, win, dtype=np.float32)
    assert s32.forward_basis.dtype == s32.inverse_basis.dtype == np.float32
    y32 = s32.inverse(mag, ph)
    m32, _ = s32.transform(x)
    assert y32.dtype == m32.dtype == np.float32 and y32.shape == want.shape and m32.shape == wm.shape
    assert 0 < np.abs(y32 - want).max() <= 1e-4 * np.abs(want).max() and 0 < np.abs(m32 - wm).max() <= 1e-4 * np.abs(wm).max()


def test_float32_envelope_of_the_oracle_is_the_hosts():
    """gl_ref.ola in float32 divides by the envelope audio.window_sumsquare builds (given the same window), bit for bit"""
    from fastspeech2_amd.audio import _window, window_sumsquare
    for filt, hop, win in [(1024, 256, 256), (256, 64, 200), (64, 64, 64)]:
        F = 7
        w2 = _window("hann", win, filt) ** 2
        env = window_sumsquare("hann", F, hop, win, filt)
        N = hop * (F - 1)
        _, y = gl_ref.ola(np.ones((1, F, filt), np.float32), None, w2, filt, hop, 0, N, dtype=np.float32)
        count = np.zeros(N + filt, np.float32)
        for f in range(F):
            count[f * hop:f * hop + filt] += 1
        want = np.where(env > gl_ref.TINY32, count / np.where(env > gl_ref.TINY32, env, 1), count) * np.float32(filt / hop)
        assert y.dtype == want.dtype == np.float32 and np.array_equal(y[0], want[filt // 2:filt // 2 + N])
        assert win == filt or (env == 0).any()                     # a zero-padded window: the envelope reaches exact zeros


def test_kernel_bars_are_what_the_generator_writes():
    from tests import gl_cases
    rec, now = gl_cases.bars(), gl_cases.measure()
    assert rec == now, {k: (rec.get(k), now.get(k)) for k in set(rec) | set(now) if rec.get(k) != now.get(k)}
    assert rec["factor"] == 4
    n = 0
    for group in ("mag_rel", "phase", "recombine", "project", "ola"):
        for key, bar in rec[group].items():
            assert np.isfinite(bar) and 0 < bar < 1e-5, (group, key, bar)          # a few float32 roundings, in every normalisation
            n += 1
    assert n == 4 * 4 + len(gl_cases.OLA_SETTINGS)
