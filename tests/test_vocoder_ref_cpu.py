"""tests/vocoder_ref.py on the CPU: its references agree with torch / numpy, each bound accepts a faithful CPU emulation of the
kernel's arithmetic (fp32 chains, bf16 operands) and rejects a deliberately wrong one, the polyphase pack of the transposed
convolutions equals F.conv_transpose1d, and _pack_convt refuses the (stride, kernel) pairs it cannot represent."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import elem_ref as R
from tests import gemm_ref as G
from tests import vocoder_ref as V

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------- bit-exact kernels
def test_chan_to_rows_reference_and_specials():
    x = torch.randn(2, 5, 7)
    x.view(-1)[:6] = V.special_values()
    r32, r16 = V.chan_to_rows(x, torch.float32), V.chan_to_rows(x, torch.bfloat16)
    for b in range(2):
        for t in range(7):
            assert torch.equal(R.bits(r32[b * 7 + t]), R.bits(x[b, :, t]))
    assert torch.equal(R.bits(r16), R.bits(R.rne_bf16(r32)))
    got = R.bits(R.rne_bf16(V.special_values())).tolist()
    assert [v & 0xffff for v in got] == [0x8000, 0x0000, 0x3F80, 0x3F82, 0x7F7F, 0x3F80]


def test_reflect_pad_reference():
    y = torch.arange(1.0, 10.0).view(1, 9)                     # N = P + 1
    out = V.reflect_pad(y, 8, 30)
    assert out[0].tolist() == [9, 8, 7, 6, 5, 4, 3, 2, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0, 0, 0]
    assert V.reflect_pad(y, 8, 20)[0].tolist() == out[0, :20].tolist()
    yy = torch.full((3, 40), float("nan"))
    lens = [40, 9, 8]
    for b, n in enumerate(lens):
        yy[b, :n] = torch.randn(n)
    yy[2] = float("nan")                                        # lens <= P: nothing is read
    rg = V.reflect_pad_ragged(yy, lens, 8, 64)
    assert not rg.isnan().any() and (rg[2] == 0).all()
    assert torch.equal(rg[1], V.reflect_pad(yy[1:2, :9], 8, 64)[0])
    with pytest.raises(AssertionError):
        V.reflect_pad(y[:, :8], 8, 30)


# -------------------------------------------------------------------------------------------------------------- conv_post
def _emulate_conv_post(x, w, bias, in_slope, S, taps, pad, drop_tap=None, cross=False):
    """conv_post_kernel on the CPU: lrelu as an fp32 product, taps * C fmafs onto one fp32 accumulator (fp64 sum of the exact product,
    rounded to fp32), tanh correctly rounded.  drop_tap: that tap is skipped; cross: taps read across utterance boundaries."""
    M, C = x.shape
    x32 = x.float()
    a = torch.where(x32 > 0, x32, x32 * torch.tensor(in_slope, dtype=torch.float32))
    acc = torch.full((M,), float(bias[0]) if bias is not None else 0.0, dtype=torch.float32)
    m = torch.arange(M)
    for j in range(taps):
        if j == drop_tap:
            continue
        ts = m % S + j - pad
        src = m + j - pad
        ok = (src >= 0) & (src < M) if cross else (ts >= 0) & (ts < S)
        rows = a[src.clamp(0, M - 1)]
        for c in range(C):
            new = (acc.to(F64) + rows[:, c].to(F64) * w[j, c].to(F64)).float()
            acc = torch.where(ok, new, acc)
    return torch.tanh(acc.to(F64)).float()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S", V.POST_LENGTHS)
def test_conv_post_bound_passes_emulation_and_rejects_wrong_taps(dtype, B, S):
    for C, taps, slope, has_bias in ((4, 7, 0.01, True), (32, 7, 1.0, False), (32, 1, 0.01, True)):
        pad = (taps - 1) // 2
        x, w, bias = V.conv_post_case(dtype, C, taps, slope, has_bias, C + 8, B, S, seed=B * 1000 + S + C)
        assert x[:, C:].isnan().all()
        pre, mag, c = V.conv_post(x[:, :C], w, bias, slope, S, taps, pad)
        assert c == taps * C + 1 and float(torch.tanh(pre).abs().max()) <= 0.98
        # the reference is F.conv1d of the leaky-ReLU'd rows, utterance by utterance
        a64 = F.leaky_relu(x[:, :C].to(F64), G.f32(slope)).view(B, S, C).transpose(1, 2)
        want = F.conv1d(a64, w.to(F64).t().unsqueeze(0), bias.to(F64) if has_bias else None, padding=pad).reshape(-1)
        assert torch.allclose(pre, want, rtol=1e-12, atol=1e-13)
        lim = V.conv_post_bound(pre, mag, c)
        ref = torch.tanh(pre)
        V.assert_within(_emulate_conv_post(x[:, :C], w, bias, slope, S, taps, pad), ref, lim, "faithful emulation")
        if taps > 1:
            assert V.ratio(_emulate_conv_post(x[:, :C], w, bias, slope, S, taps, pad, cross=True), ref, lim) > 1   # read a neighbour
            if S > pad:
                assert V.ratio(_emulate_conv_post(x[:, :C], w, bias, slope, S, taps, pad, drop_tap=pad), ref, lim) > 1


def test_pcm_truncation_reference():
    wav = torch.tensor([0.0, 1e-5, -1e-5, 0.3, -0.3, 0.99, -0.99, 1.0, -1.0, 0.5 + 2.0 ** -17])
    assert np.array_equal(V.pcm_trunc(wav), (wav.numpy() * np.float32(32768.0)).astype("int16"))
    assert V.pcm_trunc(torch.tensor([1.0]))[0] == -32768


# --------------------------------------------------------------------------------------------------------------- stft_mel
def _emulate_stft_mel(ft, NF, frames, melb, span, clamp_min, short=False):
    """stft_mel_kernel on the CPU in fp32: magnitude, per-lane / wave-tree energy, sequential fmaf chain per mel bin, log correctly
    rounded.  short: every span loses its last bin."""
    re, im = ft[:, :frames, :NF], ft[:, :frames, NF:2 * NF]
    mag = torch.sqrt(re * re + im * im)                                      # fp32, three roundings
    B = ft.shape[0]
    lanes = torch.zeros(B, frames, 64, dtype=torch.float32)
    for k0 in range(0, NF, 64):
        v = mag[:, :, k0:k0 + 64]
        lanes[:, :, :v.shape[2]] = (lanes[:, :, :v.shape[2]].to(F64) + v.to(F64) * v.to(F64)).float()
    s = lanes
    while s.shape[2] > 1:
        s = s[:, :, :s.shape[2] // 2] + s[:, :, s.shape[2] // 2:]
    energy = torch.sqrt(s[:, :, 0])
    n_mel = melb.shape[0]
    mel = torch.empty(B, n_mel, frames, dtype=torch.float32)
    for k in range(n_mel):
        lo, hi = int(span[k, 0]), int(span[k, 1]) - (1 if short else 0)
        acc = torch.zeros(B, frames, dtype=torch.float32)
        for q in range(lo, hi):
            acc = (acc.to(F64) + melb[k, q].to(F64) * mag[:, :, q].to(F64)).float()
        mel[:, k] = torch.log(torch.clamp(acc, min=clamp_min).to(F64)).float()
    return mel, energy


@pytest.mark.parametrize("NF,n_mel", [(5, 3), (64, 3), (65, 80), (513, 3)])
def test_stft_mel_bound_passes_emulation_and_rejects_a_short_span(NF, n_mel):
    frames, S, B = 17, 20, 2
    ft, melb, span = V.stft_mel_case(NF, n_mel, frames, S, 2 * NF + 4, B, seed=NF + n_mel)
    assert ft[:, frames:].isnan().all() and ft[:, :, 2 * NF:].isnan().all()
    out = V.stft_mel(ft, NF, frames, melb, span, 1e-5)
    ref, lim = out["mel"]
    assert not ref.isnan().any() and out["clamped"][:, 0].all() and out["clamped"][:, 1, 0].all() and not out["clamped"][:, 2].any()
    assert torch.equal(ref[out["clamped"]], torch.full_like(ref[out["clamped"]], math.log(float(torch.tensor(1e-5)))))
    # pinned to torch: |DFT| -> basis matmul -> log(clamp), torch.norm for the energy
    m64 = torch.sqrt(ft[:, :frames, :NF].to(F64) ** 2 + ft[:, :frames, NF:2 * NF].to(F64) ** 2).transpose(1, 2)     # (B, NF, frames)
    w = torch.nan_to_num(melb.to(F64), nan=0.0)
    want = torch.log(torch.clamp(torch.matmul(w, m64), min=float(torch.tensor(1e-5))))
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(out["energy"][0], torch.norm(m64, dim=1), rtol=1e-13)
    mel, energy = _emulate_stft_mel(ft, NF, frames, melb, span, 1e-5)
    V.assert_within(mel, ref, lim, "mel: faithful emulation")
    R.check(energy, *out["energy"], what="energy: faithful emulation")
    mel_short, _ = _emulate_stft_mel(ft, NF, frames, melb, span, 1e-5, short=True)
    assert V.ratio(mel_short[:, 2:], ref[:, 2:], lim[:, 2:]) > 1
    assert not R.within(energy * (1 + 2.0 ** -18), *out["energy"])


def test_stft_mel_reference_refuses_sums_next_to_the_clamp():
    ft, melb, span = V.stft_mel_case(5, 3, 2, 2, 10, 1, seed=1)
    ft[:, :, :] = 1e-5
    with pytest.raises(AssertionError):
        V.stft_mel(ft, 5, 2, melb, span, 1e-5)


def test_spans_of_equals_the_module_table():
    from fastspeech2_amd import audio
    stft = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    assert torch.equal(V.spans_of(stft.mel_basis), stft.mel_span)
    assert int((stft.mel_span[:, 1] - stft.mel_span[:, 0]).min()) >= 1


@pytest.mark.parametrize("flt,hop,win", [(16, 4, 16), (32, 8, 24), (64, 16, 64)])
def test_stft_numpy_equals_the_strided_convolution(flt, hop, win):
    """the numpy restatement against audio/stft.py's own formulation: conv1d of the reflect-padded signal with the windowed basis"""
    from fastspeech2_amd import audio
    N = 5 * hop + 1
    y = torch.randn(2, N, dtype=F64)
    basis = torch.from_numpy(audio._fourier_basis(flt) * audio._window("hann", win, flt)[None, :])
    xp = F.pad(y.unsqueeze(1), (flt // 2, flt // 2), mode="reflect")
    ft = F.conv1d(xp, basis.unsqueeze(1), stride=hop)
    cut = flt // 2 + 1
    mag = torch.sqrt(ft[:, :cut] ** 2 + ft[:, cut:] ** 2)
    got = V.stft_numpy(y.numpy(), flt, hop, win)
    assert got.shape == (2, cut, N // hop + 1)
    assert np.allclose(got, mag.numpy(), rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------------------------ polyphase transposed convolution
def _pack(w, bias, u, k, cdt=torch.float32):
    from fastspeech2_amd import hifigan
    return hifigan.Generator._pack_convt(V.ConvtLayer(w, bias), u, k, torch.device("cpu"), cdt)


@pytest.mark.parametrize("u,k", V.CONVT_PAIRS)
def test_polyphase_pack_equals_transposed_convolution(u, k):
    g = torch.Generator().manual_seed(u * 100 + k)
    Cin, Cout, B = 8, 4, 2
    w, bias = torch.randn(Cin, Cout, k, generator=g), torch.randn(Cout, generator=g)
    wp, bp, taps, pad = _pack(w, bias, u, k)
    assert wp.shape == (u * Cout, taps, Cin) and bp.shape == (u * Cout,)
    for T in (1, 2, 5):
        x = torch.randn(B * T, Cin, generator=g)
        want, L = V.convt_reference(x, w, bias, u, k, B, T)
        assert L == u * T
        got = V.convt_polyphase(x, wp, bp, taps, pad, u, T)
        # the pack holds the fp32 weights themselves: only fp64 summation order separates the two
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), float((got - want).abs().max())
        G.assert_rounding_only(got, want, torch.float32, f"u={u} k={k} T={T}")
        shifted = V.convt_polyphase(x, wp.roll(1, 0), bp.roll(1, 0), taps, pad, u, T)          # a phase off by one output channel
        with pytest.raises(AssertionError):
            G.assert_rounding_only(shifted, want, torch.float32, "rolled phases")


@pytest.mark.parametrize("u,k", [(3, 4), (2, 5), (8, 15), (4, 2), (3, 1)])
def test_polyphase_pack_refuses_odd_or_negative_padding(u, k):
    """k - u odd (or negative): ConvTranspose1d(padding = (k - u) // 2) yields u T + 1 (or fewer than u T) samples, which no
    u-phase image holds"""
    w, bias = torch.randn(8, 4, k), torch.randn(4)
    if k >= u:
        assert F.conv_transpose1d(torch.randn(1, 8, 5), w, bias, stride=u, padding=(k - u) // 2).shape[2] == 5 * u + 1
    with pytest.raises(ValueError):
        _pack(w, bias, u, k)


# -------------------------------------------------------------------------------------------------- fused residual block
def test_resblock_geometry_restated():
    assert all(V.rb_supported(C, k, d) for C, k, d in V.RB_CONFIGS)
    assert V.rb_rows(32, [3], (1, 3, 5)) == (12, 1000) and V.rb_rows(64, [11], (1, 3, 5)) == (60, 392)
    assert V.rb_rows(64, [3, 7, 11], (1, 3, 5)) == (60, 392) and V.rb_rows(32, [7], (1, 1, 1)) == (18, 988)
    assert not V.rb_supported(64, 11, (1, 3, 6)) and not V.rb_supported(128, 3, (1, 3, 5)) and not V.rb_supported(32, 4, (1, 1, 1))


def _bf(t):
    return t.to(torch.bfloat16).float()


def _lrelu32(t, slope):
    return torch.where(t > 0, t, t * torch.tensor(slope, dtype=torch.float32))


def _emulate_resblock(x, blocks, B, S, dil, xs0, out_scale, slope, post_slope, mutant=None, row=0, conv=2, pair=1):
    """resblock_fused_kernel in plain torch: bf16 operands, fp32 accumulation, y kept in fp32, xs rounded to bf16 after every block.
    Mutants, in convolution `conv` (1: the dilated one, 2) of pair `pair` of the first block: "tap" drops tap 0 on utterance row `row`
    of utterance 0; "neighbour" lets the convolution read the neighbouring utterance's rows where it must read zeros; "bias" adds the
    bias of another convolution."""
    C = x.shape[1]
    x32 = x.float().view(B, S, C).transpose(1, 2)
    rows = lambda t: t.transpose(1, 2).reshape(B * S, C)                      # noqa: E731
    xs = xs0.float() if xs0 is not None else torch.zeros(B * S, C)
    osc = torch.tensor(out_scale, dtype=torch.float32)

    def run(inp, w, bias, d, p, mut):
        wt = w.float().permute(0, 2, 1)
        if mut == "neighbour":
            flat = inp.transpose(0, 1).reshape(1, C, B * S)
            out = F.conv1d(flat, wt, bias, dilation=d, padding=p * d).view(C, B, S).transpose(0, 1).clone()
        else:
            out = F.conv1d(inp, wt, bias, dilation=d, padding=p * d)
        if mut == "tap" and row - p * d >= 0:
            out[0, :, row] -= w[:, 0, :].float() @ inp[0, :, row - p * d]
        return out

    for j, (w1, w2, b1, b2, k) in enumerate(blocks):
        y = x32
        p = (k - 1) // 2
        for m in range(3):
            hit1 = mutant if (j == 0 and m == pair and conv == 1) else None
            hit2 = mutant if (j == 0 and m == pair and conv == 2) else None
            a = _bf(_lrelu32(y, slope))
            t = run(a, w1[m], b2[(m + 1) % 3] if hit1 == "bias" else b1[m], dil[m], p, hit1)
            tt = _bf(_lrelu32(t, slope))
            y = run(tt, w2[m], b1[(m + 1) % 3] if hit2 == "bias" else b2[m], 1, p, hit2) + y
        xs = _bf(xs + osc * rows(y))
    if post_slope > 0:
        xs = _bf(_lrelu32(xs, post_slope))
    return xs.to(torch.bfloat16)


@pytest.mark.parametrize("kind", V.RB_KINDS)
@pytest.mark.parametrize("C,k,dil", V.RB_CONFIGS)
def test_resblock_bound_passes_the_emulation_at_every_case_shape(C, k, dil, kind):
    H, Rr = V.rb_rows(C, [k], dil)
    worst = 0.0
    for S in V.rb_lengths(H, Rr):
        xb, xsb, blocks = V.resblock_case(C, [k], S, seed=C * 1000 + k * 10 + S, kind=kind)
        x = xb[:, :C]
        for acc, ps in V.RB_FORMS:
            xs0 = xsb[:, :C] if acc else None
            ref, lim = V.resblock_reference(x, blocks, 2, S, dil, xs0=xs0, post_slope=ps)
            got = _emulate_resblock(x, blocks, 2, S, dil, xs0, 1.0 / 3, 0.1, ps)
            worst = max(worst, V.assert_within(got, ref, lim, f"{kind} C={C} k={k} dil={dil} S={S} acc={acc} post_slope={ps}"))
    print(f"[voc] resblock emulation {kind} C={C} k={k} dil={dil}: max err/bound = {worst:.3f}")


@pytest.mark.parametrize("C,k,dil", V.RB_CONFIGS)
def test_resblock_bound_rejects_three_mutants(C, k, dil):
    H, Rr = V.rb_rows(C, [k], dil)
    S = Rr + 1                                              # row R of utterance 0: the first row of the second tile
    xb, xsb, blocks = V.resblock_case(C, [k], S, seed=C + k + sum(dil))
    x = xb[:, :C]
    ref, lim = V.resblock_reference(x, blocks, 2, S, dil)
    V.assert_within(_emulate_resblock(x, blocks, 2, S, dil, None, 1.0 / 3, 0.1, 0.0), ref, lim, "unmutated")
    for mutant in ("tap", "neighbour", "bias"):
        got = _emulate_resblock(x, blocks, 2, S, dil, None, 1.0 / 3, 0.1, 0.0, mutant=mutant, row=Rr)
        r = V.ratio(got, ref, lim)
        assert r > 1, (mutant, r)
        if mutant == "tap":                                 # a single row moved, and the bound sees it there
            bad = ((got.to(F64) - ref).abs() > lim).view(2, S, C).any(-1)
            assert bad[0, Rr] and not bad[1].any()


@pytest.mark.parametrize("C,k,dil", V.RB_CONFIGS)
def test_resblock_bound_rejects_mutants_in_either_convolution_of_every_pair(C, k, dil):
    """the "coherent" operands: a dropped tap on the first row of the second tile and a neighbour's row read for a zero, in the
    dilated conv1 and in conv2 of each of the three pairs, and a foreign bias, all land outside the bound"""
    H, Rr = V.rb_rows(C, [k], dil)
    S = Rr + 1
    xb, xsb, blocks = V.resblock_case(C, [k], S, seed=C + k + sum(dil), kind="coherent")
    x = xb[:, :C]
    ref, lim = V.resblock_reference(x, blocks, 2, S, dil)
    V.assert_within(_emulate_resblock(x, blocks, 2, S, dil, None, 1.0 / 3, 0.1, 0.0), ref, lim, "unmutated")
    lowest = math.inf
    for conv in (1, 2):
        for pair in range(3):
            for mutant in ("tap", "neighbour", "bias"):
                got = _emulate_resblock(x, blocks, 2, S, dil, None, 1.0 / 3, 0.1, 0.0, mutant=mutant, row=Rr, conv=conv, pair=pair)
                r = V.ratio(got, ref, lim)
                lowest = min(lowest, r)
                assert r > 1, (mutant, conv, pair, r)
    print(f"[voc] resblock mutants C={C} k={k} dil={dil}: smallest err/bound = {lowest:.2f}")


def test_resblock_reference_equals_the_convolution_chain():
    """the reference against hifigan/models.py's ResBlock1 in torch (fp64), first and accumulating form, with post_slope"""
    C, k, dil, B, S = 32, 7, (1, 3, 5), 2, 50
    xb, xsb, blocks = V.resblock_case(C, [k], S, seed=4)
    w1, w2, b1, b2, _ = blocks[0]
    y = xb[:, :C].to(F64).view(B, S, C).transpose(1, 2)
    for m, d in enumerate(dil):
        t = F.conv1d(F.leaky_relu(y, 0.1), w1[m].to(F64).permute(0, 2, 1), b1[m].to(F64), dilation=d, padding=(k - 1) // 2 * d)
        y = F.conv1d(F.leaky_relu(t, 0.1), w2[m].to(F64).permute(0, 2, 1), b2[m].to(F64), padding=(k - 1) // 2) + y
    want = y.transpose(1, 2).reshape(B * S, C) / 3
    ref, lim = V.resblock_reference(xb[:, :C], blocks, B, S, dil)
    assert torch.allclose(ref, want, rtol=1e-6, atol=1e-7)            # (slope and 1 / 3 as their fp32 values)
    assert (lim > 0).all() and float((lim / (ref.abs() + 1e-3)).max()) < 0.5
    ref2, _ = V.resblock_reference(xb[:, :C], blocks, B, S, dil, xs0=xsb[:, :C], post_slope=0.1)
    assert torch.allclose(ref2, F.leaky_relu(want + xsb[:, :C].to(F64), 0.1), rtol=1e-6, atol=1e-7)
