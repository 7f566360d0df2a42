"""The vocoder and mel front-end kernels (csrc/fs2_vocoder.hip), the polyphase transposed convolution and the fused residual block
(csrc/fs2_resblock.hip) element by element against tests/vocoder_ref.py: bit-exact where a kernel only moves or rounds values, within
the derived per-element bounds elsewhere.  Poison convention: whatever a kernel must not read holds NaN (row padding, rows past
`frames`, samples past lens[b], filter entries outside a span); whatever it must not write holds a sentinel that is compared
bit for bit afterwards.  Each test prints the largest err / bound it saw ("[voc] ..." lines, shown with -s)."""
import math

import numpy as np
import pytest
import torch

from tests import elem_ref as R
from tests import gemm_ref as G
from tests import vocoder_ref as V

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = -12345.671875                                       # what a kernel must not overwrite (int16 buffers: 0x5A5A)


def _mods():
    from fastspeech2_amd import _lib, ops
    return _lib, ops


def _eq(got, ref, what):
    g, r = R.bits(got), R.bits(ref)
    n = int((g != r).sum())
    assert g.shape == r.shape and n == 0, f"{what}: {n} of {g.numel()} elements differ"


# ------------------------------------------------------------------------------------------------------- bit-exact kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 3])
def test_chan_to_rows_bit_exact(dev, dtype, B):
    _lib, ops = _mods()
    g = torch.Generator().manual_seed(B)
    sp = V.special_values()
    for C in (1, 31, 32, 33, 80):
        for T in (1, 31, 32, 33, 65):
            x = torch.randn(B, C, T, generator=g)
            flat = x.view(-1)
            pos = torch.randperm(flat.numel(), generator=g)[:sp.numel()]
            flat[pos] = sp[:pos.numel()]
            out, xd = torch.full((B * T * C + 64,), SENTINEL).to(dtype).to(dev), x.to(dev)
            _lib.call("fs2_chan_to_rows", xd.data_ptr(), out.data_ptr(), B, C, T, ops.dt(dtype), ops._stream())
            torch.cuda.synchronize()
            _eq(out[:B * T * C].view(B * T, C), V.chan_to_rows(x, dtype), f"chan_to_rows {dtype} B={B} C={C} T={T}")
            _eq(out[B * T * C:], torch.full((64,), SENTINEL).to(dtype), "chan_to_rows wrote past the end")


@pytest.mark.parametrize("B", [1, 3])
def test_reflect_pad_bit_exact(dev, B):
    _lib, ops = _mods()
    P = 8
    g = torch.Generator().manual_seed(B)
    for N in (9, 16, 17, 100):
        for row_len in (N + 2 * P, N + 2 * P + 29, 300):
            y = torch.randn(B, N, generator=g)
            y[0, 0], y[0, N - 1] = -0.0, V.special_values()[1]
            xp, yd = torch.full((B * row_len + 32,), SENTINEL).to(dev), y.to(dev)
            _lib.call("fs2_reflect_pad", yd.data_ptr(), xp.data_ptr(), B, N, P, row_len, ops._stream())
            torch.cuda.synchronize()
            _eq(xp[:B * row_len].view(B, row_len), V.reflect_pad(y, P, row_len), f"reflect_pad B={B} N={N} row_len={row_len}")
            _eq(xp[B * row_len:], torch.full((32,), SENTINEL), "reflect_pad wrote past the end")
    y = torch.randn(B, P).to(dev)
    xp = torch.full((B, 3 * P), SENTINEL).to(dev)
    with pytest.raises(ValueError):                              # N == P: an argument error, nothing launched
        _lib.call("fs2_reflect_pad", y.data_ptr(), xp.data_ptr(), B, P, P, 3 * P, ops._stream())
    torch.cuda.synchronize()
    _eq(xp, torch.full((B, 3 * P), SENTINEL), "reflect_pad launched on N == P")


def test_reflect_pad_ragged_rows_equal_single_utterances(dev):
    _lib, ops = _mods()
    B, P, ldy = 5, 8, 40
    lens = [40, 9, 8, 1, 23]
    g = torch.Generator().manual_seed(7)
    y = torch.full((B, ldy), float("nan"))
    for b, n in enumerate(lens):
        if n > P:
            y[b, :n] = torch.randn(n, generator=g)              # rows with lens <= P stay NaN entirely: nothing of them may be read
    yd, ld = y.to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
    for row_len in (ldy + 2 * P, 100):
        xp = torch.full((B * row_len + 32,), SENTINEL).to(dev)
        _lib.call("fs2_reflect_pad_ragged", yd.data_ptr(), ldy, ld.data_ptr(), xp.data_ptr(), B, P, row_len, ops._stream())
        torch.cuda.synchronize()
        got = xp[:B * row_len].view(B, row_len)
        _eq(got, V.reflect_pad_ragged(y, lens, P, row_len), f"reflect_pad_ragged row_len={row_len}")
        _eq(xp[B * row_len:], torch.full((32,), SENTINEL), "reflect_pad_ragged wrote past the end")
        for b, n in enumerate(lens):
            if n <= P:
                assert int((got[b] != 0).sum()) == 0
                continue
            alone, yb = torch.empty(1, row_len, device=dev), yd[b, :n].contiguous()
            _lib.call("fs2_reflect_pad", yb.data_ptr(), alone.data_ptr(), 1, n, P, row_len, ops._stream())
            torch.cuda.synchronize()
            _eq(got[b:b + 1], alone, f"ragged row {b} against the utterance alone")


# -------------------------------------------------------------------------------------------------------------- conv_post
def _conv_post(dev, x, ldx, w, bias, slope, M, S, C, taps, pad, want_wav, want_pcm):
    _lib, ops = _mods()
    wav = torch.full((M + 8,), SENTINEL).to(dev)
    pcm = torch.full((M + 8,), 0x5A5A, dtype=torch.int16).to(dev)
    xd, wd = x.to(dev), w.to(dev)
    bd = bias.to(dev) if bias is not None else None
    _lib.call("fs2_conv_post_pcm", xd.data_ptr(), ldx, wd.data_ptr(), ops._p(bd), slope, wav.data_ptr() if want_wav else None,
              pcm.data_ptr() if want_pcm else None, 32768.0, M, S, C, taps, pad, ops.dt(x), ops._stream())
    torch.cuda.synchronize()
    wav, pcm = wav.cpu(), pcm.cpu()
    _eq(wav[M if want_wav else 0:], torch.full((M + 8,), SENTINEL)[M if want_wav else 0:], "conv_post wrote wav it must not")
    assert (pcm[M if want_pcm else 0:] == 0x5A5A).all(), "conv_post wrote pcm it must not"
    return wav[:M], pcm[:M].numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [4, 32])
@pytest.mark.parametrize("taps", [7, 1])
def test_conv_post_pcm_elementwise(dev, dtype, C, taps):
    pad = (taps - 1) // 2
    worst = 0.0
    for B, S in V.POST_LENGTHS:
        for slope in (0.01, 1.0):
            for has_bias in (True, False):
                for ldx in (C, C + 8):
                    x, w, bias = V.conv_post_case(dtype, C, taps, slope, has_bias, ldx, B, S, seed=B * 1000 + S + C + taps)
                    M = B * S
                    pre, mag, c = V.conv_post(x[:, :C], w, bias, slope, S, taps, pad)
                    ref = torch.tanh(pre)
                    assert float(ref.abs().max()) <= 0.98
                    lim = V.conv_post_bound(pre, mag, c)
                    what = f"conv_post {dtype} C={C} taps={taps} B={B} S={S} slope={slope} bias={has_bias} ldx={ldx}"
                    wav, pcm = _conv_post(dev, x, ldx, w, bias, slope, M, S, C, taps, pad, True, True)
                    worst = max(worst, V.assert_within(wav, ref, lim, what))
                    assert np.array_equal(pcm, V.pcm_trunc(wav)), what + ": pcm is not the truncation of wav"
                    want = np.trunc(ref.numpy() * 32768.0).astype(np.int64)
                    steps = np.ceil(lim.numpy() * 32768.0).astype(np.int64) + 1
                    assert (np.abs(pcm.astype(np.int64) - want) <= steps).all(), what + ": pcm against the reference"
                    wav1, _ = _conv_post(dev, x, ldx, w, bias, slope, M, S, C, taps, pad, True, False)
                    _, pcm1 = _conv_post(dev, x, ldx, w, bias, slope, M, S, C, taps, pad, False, True)
                    _eq(wav1, wav, what + ": wav only")
                    assert np.array_equal(pcm1, pcm), what + ": pcm only"
    print(f"[voc] conv_post {dtype} C={C} taps={taps}: max err/bound = {worst:.3f}")


def _sweep_tanh():
    g = torch.Generator().manual_seed(11)
    n = 1 << 20
    a = torch.cat([(torch.rand(n // 2, generator=g) * 4.6 - 2.3), torch.randn(n // 4, generator=g) * 0.05,
                   torch.exp(torch.rand(n // 4, generator=g) * -20.0) * torch.sign(torch.randn(n // 4, generator=g))])
    return a.float()


def _sweep_log():
    g = torch.Generator().manual_seed(12)
    n = 1 << 20
    return torch.cat([torch.exp(torch.rand(n // 2, generator=g) * (math.log(1e4) - math.log(2e-5)) + math.log(2e-5)),
                      1.0 + torch.randn(n // 2, generator=g) * 0.2]).abs().clamp_min(2e-5).float()


def test_tanhf_logf_measured(dev):
    """the device library's tanhf / logf against fp64 on the same fp32 arguments, through the kernels that use them: a 1-tap identity
    conv_post launch, and stft_mel with unit one-bin filters (acc = fmaf(1, |re|, 0) = |re| exactly).  Twice the maximum recorded
    in tests/vocoder_ref.py is allowed."""
    _lib, ops = _mods()
    a = _sweep_tanh()
    M, C = a.numel(), 4
    x = torch.zeros(M, C)
    x[:, 0] = a
    w = torch.zeros(1, C)
    w[0, 0] = 1.0
    wav, _ = _conv_post(dev, x, C, w, None, 1.0, M, M, C, 1, 0, True, False)
    ref = torch.tanh(a.to(F64))
    r_t = float(((wav.to(F64) - ref).abs() / (R.U32 * ref.abs())).max())
    v = _sweep_log()
    NF, frames = 64, v.numel() // 64
    ft = torch.zeros(1, frames, 2 * NF)
    ft[0, :, :NF] = v.view(frames, NF)
    melb = torch.eye(NF)
    span = torch.stack([torch.arange(NF), torch.arange(NF) + 1], 1).to(torch.int32)
    mel = torch.empty(1, NF, frames, device=dev)
    energy = torch.empty(1, frames, device=dev)
    ftd, mbd, spd = ft.to(dev), melb.to(dev), span.to(dev)
    _lib.call("fs2_stft_mel_epilogue", ftd.data_ptr(), 2 * NF, mbd.data_ptr(), spd.data_ptr(), mel.data_ptr(),
              energy.data_ptr(), 1, frames, frames, NF, NF, 1e-5, ops._stream())
    torch.cuda.synchronize()
    refl = torch.log(v.to(F64)).view(frames, NF).t()
    errl = (mel[0].cpu().to(F64) - refl).abs()
    r_l = float(torch.where(refl == 0, torch.zeros_like(errl), errl / (R.U32 * refl.abs().clamp_min(1e-300))).max())
    assert float(errl[refl == 0].max() if (refl == 0).any() else 0.0) == 0.0
    print(f"[voc] tanhf: max err/(u |tanh|) = {r_t:.3f} (recorded {V.TANHF_SEEN});  logf: max err/(u |log|) = {r_l:.3f} (recorded {V.LOGF_SEEN})")
    assert r_t <= V.TANHF_ULPS and r_l <= V.LOGF_ULPS


# --------------------------------------------------------------------------------------------------------------- stft_mel
def _stft_mel(dev, ft, ldft, melb, span, B, S, frames, NF, n_mel):
    _lib, ops = _mods()
    mel = torch.full((B * n_mel * frames + 16,), SENTINEL).to(dev)
    energy = torch.full((B * frames + 16,), SENTINEL).to(dev)
    ftd, mbd, spd = ft.to(dev), melb.to(dev), span.to(dev)
    _lib.call("fs2_stft_mel_epilogue", ftd.data_ptr(), ldft, mbd.data_ptr(), spd.data_ptr(), mel.data_ptr(),
              energy.data_ptr(), B, S, frames, NF, n_mel, 1e-5, ops._stream())
    torch.cuda.synchronize()
    mel, energy = mel.cpu(), energy.cpu()
    _eq(mel[B * n_mel * frames:], torch.full((16,), SENTINEL), "stft_mel wrote past mel")
    _eq(energy[B * frames:], torch.full((16,), SENTINEL), "stft_mel wrote past energy")
    return mel[:B * n_mel * frames].view(B, n_mel, frames), energy[:B * frames].view(B, frames)


@pytest.mark.parametrize("NF", [5, 64, 65, 513])
@pytest.mark.parametrize("n_mel", [3, 80])
def test_stft_mel_epilogue_elementwise(dev, NF, n_mel):
    worst_m = worst_e = 0.0
    log_clamp = math.log(float(torch.tensor(1e-5)))
    for frames in (1, 15, 16, 17, 33):
        for S in (frames, frames + 3):
            for ldft in (2 * NF, 2 * NF + 4):
                for B in (1, 2):
                    ft, melb, span = V.stft_mel_case(NF, n_mel, frames, S, ldft, B, seed=NF * 100 + frames + S + ldft + B)
                    out = V.stft_mel(ft, NF, frames, melb, span, 1e-5)          # (asserts that no sum lies in (0, 2 clamp_min))
                    assert out["clamped"][:, 0].all() and out["clamped"][:, 1, 0].all()
                    mel, energy = _stft_mel(dev, ft, ldft, melb, span, B, S, frames, NF, n_mel)
                    what = f"stft_mel NF={NF} n_mel={n_mel} frames={frames} S={S} ldft={ldft} B={B}"
                    worst_m = max(worst_m, V.assert_within(mel, *out["mel"], what + " mel"))
                    assert (mel[out["clamped"]].to(F64) - log_clamp).abs().max() <= V.LOGF_ULPS * R.U32 * abs(log_clamp)
                    worst_e = max(worst_e, R.check(energy, *out["energy"], what=what + " energy") / out["energy"][2])
    print(f"[voc] stft_mel NF={NF} n_mel={n_mel}: mel max err/bound = {worst_m:.3f}, energy max err/bound = {worst_e:.3f}")


def test_stft_mel_epilogue_slaney_basis(dev):
    from fastspeech2_amd.audio import slaney_mel_filterbank
    NF, n_mel, frames, S, B = 513, 80, 33, 36, 2
    basis = slaney_mel_filterbank(22050, 1024, 80, 0, 8000)
    ft, melb, span = V.stft_mel_case(NF, n_mel, frames, S, 2 * NF + 2, B, seed=3, slaney=basis)
    out = V.stft_mel(ft, NF, frames, melb, span, 1e-5)
    mel, energy = _stft_mel(dev, ft, 2 * NF + 2, melb, span, B, S, frames, NF, n_mel)
    rm = V.assert_within(mel, *out["mel"], "stft_mel slaney mel")
    re = R.check(energy, *out["energy"], what="stft_mel slaney energy") / out["energy"][2]
    print(f"[voc] stft_mel slaney: mel max err/bound = {rm:.3f}, energy max err/bound = {re:.3f}")


# ------------------------------------------------------------------------------------------- framed DFT at small configurations
@pytest.mark.parametrize("flt,hop,win", [(16, 4, 16), (32, 8, 24), (64, 16, 64)])
def test_framed_dft_small_configurations_against_numpy(dev, flt, hop, win):
    from fastspeech2_amd.audio import STFT, TacotronSTFT
    stft = STFT(flt, hop, win).to(dev)
    taco = TacotronSTFT(flt, hop, win, 4, 16000, 0, 8000).to(dev)
    g = torch.Generator().manual_seed(flt)
    worst = 0.0
    for N in (flt // 2 + 1, 2 * flt - 1, 5 * hop, 5 * hop + 1):
        y = (torch.rand(2, N, generator=g) * 2 - 1) * 0.9
        ref = torch.from_numpy(V.stft_numpy(y.numpy(), flt, hop, win))
        mag, _ = stft.transform(y.to(dev))
        assert mag.shape == ref.shape == (2, flt // 2 + 1, N // hop + 1)
        G.assert_rounding_only(mag.cpu(), ref, torch.float32, f"STFT.transform {flt}/{hop}/{win} N={N}")
        worst = max(worst, G.rounding_ratio(mag.cpu(), ref, torch.float32))
        mel, energy = taco.mel_spectrogram(y.to(dev))
        assert mel.shape == (2, 4, N // hop + 1) and energy.shape == (2, N // hop + 1)
        G.assert_rounding_only(energy.cpu(), ref.pow(2).sum(1).sqrt(), torch.float32, f"energy {flt}/{hop}/{win} N={N}")
    print(f"[voc] framed DFT {flt}/{hop}/{win}: max err/bound = {worst:.3f}")


def test_mel_spectrogram_ragged_on_the_length_edges(dev):
    from fastspeech2_amd.audio import TacotronSTFT
    stft = TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000).to(dev)
    lens = [513, 600, 2048, 2049]                                # N = P + 1, N % hop != 0, N % hop == 0, one past it
    g = torch.Generator().manual_seed(9)
    y = torch.full((4, max(lens)), float("nan"))
    for b, n in enumerate(lens):
        y[b, :n] = (torch.rand(n, generator=g) * 2 - 1) * 0.8
    mel, energy, frames = stft.mel_spectrogram_ragged(y.to(dev), lens)
    assert frames.tolist() == [n // 256 + 1 for n in lens]
    for b, n in enumerate(lens):
        m1, e1 = stft.mel_spectrogram(y[b:b + 1, :n].to(dev))
        f = n // 256 + 1
        assert m1.shape == (1, 80, f)
        _eq(mel[b:b + 1, :, :f], m1, f"ragged mel of utterance {b}")
        _eq(energy[b:b + 1, :f], e1, f"ragged energy of utterance {b}")


# ------------------------------------------------------------------------------------ polyphase transposed convolution
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("u,k", V.CONVT_PAIRS)
def test_polyphase_transposed_convolution_elementwise(dev, dtype, u, k):
    from fastspeech2_amd import hifigan
    _lib, ops = _mods()
    td = G.DTYPES[dtype]
    Cin, Cout, B = 64, 32, 2
    g = torch.Generator().manual_seed(u * 100 + k)
    w = torch.randn(Cin, Cout, k, generator=g) / (Cin * k / u) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    wp, bp, taps, pad = hifigan.Generator._pack_convt(V.ConvtLayer(w, bias), u, k, dev, td)
    w_r = w.to(td)                                               # the pack rounds the weights to the compute type
    worst = 0.0
    for T in (1, 2, 37):
        x = (torch.randn(B * T, Cin, generator=g) * 0.7).to(td)
        for ps in (0.0, 0.1):
            buf = torch.full((B * T + 8, u * Cout), SENTINEL).to(td).to(dev)
            y = ops.conv_gemm(x.to(dev), wp, bp, T, taps=taps, pad=pad, post_slope=ps, out=buf[:B * T])
            torch.cuda.synchronize()
            _eq(buf[B * T:], torch.full((8, u * Cout), SENTINEL).to(td), f"convT {dtype} u={u} k={k} T={T}: rows past M were written")
            ref, L = V.convt_reference(x, w_r, bias, u, k, B, T, post_slope=ps)
            assert L == u * T and y.shape == (B * T, u * Cout)
            got = y.cpu().view(B * T * u, Cout)
            G.assert_rounding_only(got, ref, td, f"convT {dtype} u={u} k={k} T={T} post_slope={ps}")
            worst = max(worst, G.rounding_ratio(got, ref, td))
    print(f"[voc] polyphase convT {dtype} u={u} k={k}: max err/bound = {worst:.3f}")


# -------------------------------------------------------------------------------------------------- fused residual block
def _on_dev(dev, xb, xsb, blocks):
    """x as it is; the output buffer with 8 sentinel rows past M (its padding columns hold NaN like x's)"""
    tail = torch.full((8, xsb.shape[1]), SENTINEL).to(torch.bfloat16)
    return xb.to(dev), torch.cat([xsb, tail]).to(dev), [(w1.to(dev), w2.to(dev), b1.to(dev), b2.to(dev), k) for w1, w2, b1, b2, k in blocks]


def _untouched(out, init, M, C, what):
    """padding columns and the rows past M hold the bits they held before the launch"""
    _eq(out[:, C:].contiguous(), init[:, C:].contiguous(), what + ": padding columns were written")
    _eq(out[M:].contiguous(), init[M:].contiguous(), what + ": rows past M were written")


@pytest.mark.parametrize("kind", V.RB_KINDS)
@pytest.mark.parametrize("C,k,dil", V.RB_CONFIGS)
def test_resblock_fused_elementwise(dev, C, k, dil, kind):
    """fs2_resblock_fwd against the fp64 block with the carried per-element bound, the utterance length on every tile seam
    (fs2_resblock.hip: RbCfg<C>::E rows per tile, rb_halo(), R = E - 2 H in resblocks_impl), first and accumulating form, with and
    without the output leaky-ReLU, x and xs column slices of wider buffers whose padding holds NaN, sentinel rows past M.  Both
    operand families of vocoder_ref.resblock_case: "coherent" is the one at which a whole tap of either convolution of any pair
    lands outside the bound."""
    _lib, ops = _mods()
    B = 2
    assert _lib.load().fs2_resblock_supported(C, k, *dil, ops.BF16) == 1 and V.rb_supported(C, k, dil)
    assert _lib.load().fs2_resblock_supported(C, k, *dil, ops.F32) == 0
    H, Rr = V.rb_rows(C, [k], dil)
    worst = 0.0
    for S in V.rb_lengths(H, Rr):
        M = B * S
        xb, xsb, blocks = V.resblock_case(C, [k], S, seed=C * 1000 + k * 10 + S, kind=kind)
        xd, xsd, bd = _on_dev(dev, xb, xsb, blocks)
        w1, w2, b1, b2, _ = bd[0]
        for acc, ps in V.RB_FORMS:
            ref, lim = V.resblock_reference(xb[:, :C], blocks, B, S, dil, xs0=xsb[:, :C] if acc else None, post_slope=ps)
            out = xsd.clone()
            _lib.call("fs2_resblock_fwd", xd.data_ptr(), xd.stride(0), w1.data_ptr(), w2.data_ptr(), b1.data_ptr(), b2.data_ptr(),
                      out.data_ptr(), out.stride(0), int(acc), 1.0 / 3, 0.1, ps, B, S, C, k, *dil, ops.BF16, ops._stream())
            torch.cuda.synchronize()
            out = out.cpu()
            what = f"resblock {kind} C={C} k={k} dil={dil} S={S} accumulate={acc} post_slope={ps}"
            _untouched(out, xsd.cpu(), M, C, what)
            worst = max(worst, V.assert_within(out[:M, :C], ref, lim, what))
    print(f"[voc] resblock {kind} C={C} k={k} dil={dil}: max err/bound = {worst:.3f}")


@pytest.mark.parametrize("kind", V.RB_KINDS)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("dil", [(1, 3, 5), (1, 1, 1)])
def test_resstage_fused_elementwise(dev, C, dil, kind):
    """fs2_resstage_fwd (k = 3, 7, 11 in one launch) at ITS tile geometry - the widest halo, that of k = 11 - and equal to three block
    launches bit for bit at every one of those lengths."""
    _lib, ops = _mods()
    B, ks = 2, [3, 7, 11]
    H, Rr = V.rb_rows(C, ks, dil)
    assert (H, Rr) == V.rb_rows(C, [11], dil)
    worst = 0.0
    for S in V.rb_lengths(H, Rr):
        M = B * S
        xb, xsb, blocks = V.resblock_case(C, ks, S, seed=C * 77 + S + sum(dil), kind=kind)
        xd, xsd, bd = _on_dev(dev, xb, xsb, blocks)
        for ps in (0.0, 0.1):
            ref, lim = V.resblock_reference(xb[:, :C], blocks, B, S, dil, post_slope=ps)
            out = xsd.clone()
            args = []
            for w1, w2, b1, b2, k in bd:
                args += [w1.data_ptr(), w2.data_ptr(), b1.data_ptr(), b2.data_ptr(), k]
            _lib.call("fs2_resstage_fwd", xd.data_ptr(), xd.stride(0), *args, out.data_ptr(), out.stride(0), 1.0 / 3, 0.1, ps, B, S, C,
                      *dil, ops.BF16, ops._stream())
            xc = xd[:, :C].contiguous()
            xs = None
            for j, (w1, w2, b1, b2, k) in enumerate(bd):
                xs = ops.resblock_fwd(xc, w1, w2, b1, b2, B, S, k, dil, xs=xs, out_scale=1.0 / 3, post_slope=ps if j == 2 else 0.0)
            torch.cuda.synchronize()
            what = f"resstage {kind} C={C} dil={dil} S={S} post_slope={ps}"
            _untouched(out.cpu(), xsd.cpu(), M, C, what)
            worst = max(worst, V.assert_within(out[:M, :C].cpu(), ref, lim, what))
            _eq(out[:M, :C].contiguous(), xs, what + ": three block launches")
    print(f"[voc] resstage {kind} C={C} dil={dil}: max err/bound = {worst:.3f}")
