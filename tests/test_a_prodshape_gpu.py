"""Parity at PRODUCTION shapes (BASELINE configs[1]: B=48, L=128, T~925, 4+4 layers) - collected first on purpose.

What the bench times is the bf16 path (persistent / ring contraction kernels, bf16 weight-gradient kernels with ragged
`lens` and split-K atomics, bf16 attention backward) at M = 44 400 rows; the small goldens never reach those dispatch
branches.  Here:
  * every contraction shape of the train step, forward and data gradient, bf16 AND fp32, with ragged lengths + tile map, is
    compared ELEMENTWISE with an exact-product reference (same bf16-rounded operands, fp32/fp64 accumulation): a bf16 result
    may differ from it by final rounding only (1 ulp = 2^-8 relative) - a wrong tap at one sequence boundary is O(1);
  * the weight-gradient kernels at M = 44 400 with ragged lens (the 5- and 8-split grids) and bf16 attention backward at
    S = 925, per-tensor;
  * the WHOLE train step (forward + loss + backward, dropout off) at full size against the fp64 oracle in fp32: every gradient
    tensor elementwise (<= 2e-3 of its max) (reference model/fastspeech2.py:43-110, model/loss.py:19-92).  The bf16 whole-step
    budget - a statistical bar, not an elementwise one - is tests/test_z_bf16_budget_gpu.py, collected last.
"""
import math

import pytest
import torch

from oracle.weights import seeded_state_dict, synthetic_batch
from tests.golden import configs
from tests.gemm_ref import assert_rounding_only, conv_reference
from tests.helpers import make_model

pytestmark = pytest.mark.gpu
B, L = 48, 128
BF16_ULP = 2.0 ** -8


def _ops():
    from fastspeech2_amd import ops
    return ops


def ragged_lens(S, seed=5):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(int(0.55 * S), S + 1, (B,), generator=g)
    lens[0] = S
    return torch.sort(lens, descending=True)[0].to(torch.int32)


def conv_ref_gpu(x, w_tap_major, bias, S, pad, lens=None):
    """exact-product reference on the device (tests/gemm_ref.py): y[m] = sum_j x[m + j - pad] @ W[:, j, :].T (+bias), taps outside the
    row's own sequence contribute 0; fp32 operands (bf16 values are exact in fp32), fp32 matmuls, summed over taps in fp64."""
    return conv_reference(x, w_tap_major, bias, S, pad=pad, lens=lens)


# (name, Cin, Cout, k, S): every contraction of the 4+4 train step that runs at M = B*S rows
SHAPES = [("ffn w_1 k9", 256, 1024, 9, 925), ("ffn w_2 k1", 1024, 256, 1, 925), ("qkv", 256, 768, 1, 925), ("fc", 256, 256, 1, 925),
          ("postnet k5", 512, 512, 5, 925), ("postnet in", 80, 512, 5, 925), ("postnet out", 512, 80, 5, 925), ("mel", 256, 80, 1, 925),
          ("enc w_1 k9", 256, 1024, 9, 128), ("predictor k3", 256, 256, 3, 128)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name,Cin,Cout,k,S", SHAPES)
def test_contraction_forward_and_dgrad_production_shapes(dev, dtype, name, Cin, Cout, k, S):
    ops = _ops()
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    M = B * S
    pad = (k - 1) // 2
    lens = ragged_lens(S)
    x = torch.randn(M, Cin, generator=g).to(dev).to(dtype)
    w = (torch.randn(Cout, k, Cin, generator=g) / math.sqrt(Cin * k)).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev)
    wf, wd = ops.pack_weight(w, dtype)
    lens_d = lens.to(dev)
    tmap = ops.tile_map(lens_d, B, S)
    n_real = int(tmap[0].item())
    ntm = (M + 255) // 256
    assert 0 < n_real <= ntm and sorted(tmap[1:].tolist()) == list(range(ntm))       # a permutation: real first, padded last
    # forward: bias + ReLU, with and without lens / tile map (the persistent kernel needs the map; without it the ring / 128^2 run)
    ref = torch.relu(conv_ref_gpu(x, wf, bias, S, pad))
    ref_l = ref.clone()
    ref_l[(torch.arange(S, device=dev).unsqueeze(0) >= lens_d.unsqueeze(1)).reshape(-1)] = 0
    # ... and with the tail-split scratch (the persistent kernel K-splits its last partial round of tiles; slabs poisoned with NaN)
    tws = ops.tail_workspace(dev).fill_(float("nan"))
    for use_lens, use_map, tail in ((False, False, None), (True, False, None), (True, True, None), (False, False, tws), (True, True, tws)):
        y = ops.conv_gemm(x, wf, bias, S, taps=k, pad=pad, act=ops.ACT_RELU, lens=lens_d if use_lens else None,
                          tmap=tmap if use_map else None, tail_ws=tail)
        assert_rounding_only(y, ref_l if use_lens else ref, dtype, (name, "fwd", use_lens, use_map, tail is not None))
    # data gradient (tap-flipped pack, pad' = k-1-pad) with the fused residual add and with the ReLU gate
    dy = torch.randn(M, Cout, generator=g).to(dev).to(dtype)
    res = torch.randn(M, Cin, generator=g).to(dev).to(dtype)
    dref = conv_ref_gpu(dy, wd, None, S, (k - 1) - pad, lens=lens_d)
    valid = (torch.arange(S, device=dev).unsqueeze(0) < lens_d.unsqueeze(1)).reshape(-1, 1)
    for tail in (None, tws):
        dx = ops.conv_gemm(dy, wd, None, S, taps=k, pad=(k - 1) - pad, res=res, lens=lens_d, tmap=tmap, tail_ws=tail)
        assert_rounding_only(dx, (dref + res.double()) * valid, dtype, (name, "dgrad+res", tail is not None))
        dx = ops.conv_gemm(dy, wd, None, S, taps=k, pad=(k - 1) - pad, act=ops.ACT_GATE, res=res, lens=lens_d, tmap=tmap, tail_ws=tail)
        assert_rounding_only(dx, torch.where(res.double() > 0, dref, torch.zeros_like(dref)) * valid, dtype, (name, "dgrad gate", tail is not None))
    if dtype == torch.bfloat16 and Cin % 64 == 0:
        # every real-tile count from 1 to the full batch: whole rounds, 2- / 4- / 8-way tails and the all-tail launches
        for nb in (1, 3, 7, 12, 20, 29, 37, 45):
            Mq = nb * S
            lq = lens_d[:nb].contiguous()
            tq = ops.tile_map(lq, nb, S)
            yq = ops.conv_gemm(x[:Mq], wf, bias, S, taps=k, pad=pad, act=ops.ACT_RELU, lens=lq, tmap=tq, tail_ws=tws)
            assert_rounding_only(yq, ref_l[:Mq], dtype, (name, "fwd tail sweep", nb))


@pytest.mark.parametrize("name,N,S,Bq", [("qkv", 768, 925, 48), ("fc", 256, 925, 48), ("w_2 dgrad", 1024, 925, 48), ("N512 short", 512, 333, 40),
                                         ("fc 30 seqs", 256, 925, 30), ("qkv ragged tail", 768, 131, 77)])
def test_streaming_k256_kernel_epilogues_and_edges(dev, name, N, S, Bq):
    """conv_gemm_s_kernel (fs2_gemm_s.hip: weights in registers, X streamed through a ring of 64-row tiles behind two loader waves)
    takes every bf16 one-tap launch with K = 256, N % 256 == 0 and at least one (tile, column group) pair per CU.  Every epilogue
    form the engine uses through it - bias, bias + ReLU, lens (padded rows zero: the lengths are staged in LDS), residual add,
    ReLU gate, accumulate with scale - and the edges of its schedule: row counts that are not a multiple of 64 (a last tile with
    rows beyond M), stripes with unequal tile counts, 1 / 2 / 3 / 4 column groups (the XCD-aware 1-D grid), sequences shorter
    than a tile.  Elementwise against the exact-product reference, rounding only; and the dispatcher really picks variant 9."""
    ops = _ops()
    from fastspeech2_amd import _lib
    dtype, K = torch.bfloat16, 256
    M = Bq * S
    g = torch.Generator().manual_seed(sum(ord(c) for c in name) + 7)
    assert _lib.load().fs2_conv_gemm_variant(K, N, 0, 0, 0, M, N, K, S, 1, 1, 0, 0.0, 1) == 9, "not on the streaming kernel"
    x = torch.randn(M, K, generator=g).to(dev).to(dtype)
    w = (torch.randn(N, 1, K, generator=g) / math.sqrt(K)).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    wf, _ = ops.pack_weight(w, dtype)
    lens = torch.randint(max(1, S // 2), S + 1, (Bq,), generator=g).to(torch.int32)
    lens[0], lens[-1] = S, max(1, S // 3)
    lens_d = lens.to(dev)
    ref = conv_ref_gpu(x, wf, bias, S, 0)
    ref_nb = conv_ref_gpu(x, wf, None, S, 0)
    assert_rounding_only(ops.conv_gemm(x, wf, bias, S), ref, dtype, (name, "bias"))
    assert_rounding_only(ops.conv_gemm(x, wf, bias, S, act=ops.ACT_RELU), torch.relu(ref), dtype, (name, "bias + relu"))
    y = ops.conv_gemm(x, wf, bias, S, lens=lens_d)
    assert_rounding_only(y, conv_ref_gpu(x, wf, bias, S, 0, lens=lens), dtype, (name, "lens"))
    pad_rows = (torch.arange(S).unsqueeze(0) >= lens.unsqueeze(1)).reshape(-1).to(dev)
    assert (y[pad_rows] == 0).all()
    res = torch.randn(M, N, generator=g).to(dev).to(dtype)
    assert_rounding_only(ops.conv_gemm(x, wf, None, S, res=res), ref_nb + res.double(), dtype, (name, "residual"))
    assert_rounding_only(ops.conv_gemm(x, wf, None, S, act=ops.ACT_GATE, res=res, lens=lens_d),
                         torch.where((res.double() > 0) & ~pad_rows.unsqueeze(1), ref_nb, torch.zeros_like(ref_nb)), dtype, (name, "gate + lens"))
    acc0 = torch.randn(M, N, generator=g).to(dev).to(dtype)
    out = acc0.clone()
    ops.conv_gemm(x, wf, bias, S, out=out, accumulate=True, out_scale=0.5)
    assert_rounding_only(out, acc0.double() + 0.5 * ref, dtype, (name, "accumulate"))
    # a strided operand (the fused QKV buffer's K slice is read with ldx = 768) and a strided result
    xs = torch.randn(M, 3 * K, generator=g).to(dev).to(dtype)
    ys = torch.full((M, 2 * N), 7.0, device=dev, dtype=dtype)
    ops.conv_gemm(xs[:, K:2 * K], wf, bias, S, out=ys[:, N:], ldx=3 * K, ldy=2 * N, Cin=K, N=N, M=M)
    assert_rounding_only(ys[:, N:], conv_ref_gpu(xs[:, K:2 * K].contiguous(), wf, bias, S, 0), dtype, (name, "strided"))
    assert (ys[:, :N] == 7.0).all()


@pytest.mark.parametrize("name,C,N,k,dil,S,Bq", [("rb C256 k7 d3", 256, 256, 7, 3, 7200, 8), ("rb C128 k11 d5", 128, 128, 11, 5, 57600, 4),
                                                 ("rb C128 k3 d1", 128, 128, 3, 1, 57600, 4), ("rb C256 k11 d1", 256, 256, 11, 1, 7200, 8),
                                                 ("up0 as 3-tap", 512, 2048, 3, 1, 900, 8)])
def test_vocoder_convs_with_leaky_relu_prologue(dev, name, C, N, k, dil, S, Bq):
    """HiFi-GAN's pre-activation convolutions at batch-synthesis size (hifigan/models.py:96-103): leaky-ReLU prologue on the
    input fragments, dilation halos of up to 50 rows (the persistent kernel's wide-halo configuration), leaky-ReLU epilogue and
    the fused residual - elementwise against the exact-product reference."""
    ops = _ops()
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    M = Bq * S
    pad = (k * dil - dil) // 2
    x = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(N, k, C, generator=g) / math.sqrt(C * k)).to(dev).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(dev)
    xa = torch.where(x.float() > 0, x.float(), (x.float() * 0.1)).to(torch.bfloat16)       # the prologue rounds lrelu(x) to bf16
    xs = xa.float().view(Bq, S, C)
    ref = torch.zeros(Bq, S, N, device=dev, dtype=torch.float64)
    for j in range(k):
        sh = j * dil - pad
        lo, hi = max(0, -sh), min(S, S - sh)
        ref[:, lo:hi] += (xs[:, lo + sh:hi + sh] @ w[:, j, :].float().t()).double()
    ref = (ref + bias.double()).view(M, N)
    y = ops.conv_gemm(x, w, bias, S, taps=k, dil=dil, pad=pad, in_act=ops.ACT_LRELU, in_slope=0.1, act=ops.ACT_LRELU, slope=0.1)
    assert_rounding_only(y, torch.where(ref > 0, ref, ref * 0.1), torch.bfloat16, (name, "lrelu-conv-lrelu"))
    if N == C:
        res = torch.randn(M, N, generator=g).to(dev).to(torch.bfloat16)
        y = ops.conv_gemm(x, w, bias, S, taps=k, dil=dil, pad=pad, in_act=ops.ACT_LRELU, in_slope=0.1, res=res, out_scale=1.0 / 3)
        assert_rounding_only(y, (ref + res.double()) / 3, torch.bfloat16, (name, "lrelu-conv+res/3"))


# ---------------------------------------------------------------------------------------------------------------------------
# Config 5 (batch synthesis, bf16 vocoder): the kernels the RTF is quoted on, pinned at synthesis size
# ---------------------------------------------------------------------------------------------------------------------------
def dilated_conv_ref(xa, w, bias, Bq, S, k, dil, pad):
    """exact-product reference of a dilated Conv1d on rows (tests/gemm_ref.py): xa (M, C) f32 holding bf16 values (activation already
    applied and rounded as the kernel's prologue does), w (N, k, C) bf16.  fp32 matmuls per tap, summed over taps in fp64."""
    assert xa.shape[0] == Bq * S and w.shape[1] == k
    return conv_reference(xa, w, bias, S, dil=dil, pad=pad)


def _variant(ops, x, y, res, M, N, C, S, k, dil, in_act, in_slope):
    from fastspeech2_amd import _lib
    return _lib.load().fs2_conv_gemm_variant(x.stride(0), y.stride(0), res.stride(0) if res is not None else 0, 0, 0, M, N, C, S, k, dil,
                                             in_act, in_slope, ops.dt(x))


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C,S", [(64, 115200), (32, 230400)])
def test_vocoder_skinny_convs_synthesis_size(dev, C, S, k):
    """conv_skinny_kernel<64> / <32> (fs2_gemm.hip; HiFi-GAN's last two stages, hifigan/models.py:96-103) at batch-synthesis size
    - 8 utterances x 900 frames: M = 921 600 rows of 64 channels / 1 843 200 rows of 32 - in every form hifigan.py launches it:
    conv1 = leaky-ReLU prologue, dilation 1 / 3 / 5, leaky-ReLU epilogue; conv2 = residual add; a branch's last conv2 = residual,
    out_scale 1/3, fresh and ACCUMULATED onto an existing bf16 tensor.  Elementwise against the exact-product reference: a bf16
    result may differ by its final rounding only."""
    ops = _ops()
    Bq = 8
    M = Bq * S
    g = torch.Generator().manual_seed(1000 * C + k)
    x = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    w1 = (torch.randn(C, k, C, generator=g) / math.sqrt(C * k)).to(dev).to(torch.bfloat16)
    w2 = (torch.randn(C, k, C, generator=g) / math.sqrt(C * k)).to(dev).to(torch.bfloat16)
    b1 = torch.randn(C, generator=g).to(dev)
    b2 = torch.randn(C, generator=g).to(dev)
    res = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    xa = torch.where(x.float() > 0, x.float(), x.float() * 0.1).to(torch.bfloat16).float()   # the prologue rounds lrelu(x) to bf16
    for dil in (1, 3, 5):
        pad = (k * dil - dil) // 2
        y = ops.conv_gemm(x, w1, b1, S, taps=k, dil=dil, pad=pad, in_act=ops.ACT_LRELU, in_slope=0.1, act=ops.ACT_LRELU, slope=0.1)
        assert _variant(ops, x, y, None, M, C, C, S, k, dil, ops.ACT_LRELU, 0.1) == 4, "not the skinny kernel"
        ref = dilated_conv_ref(xa, w1, b1, Bq, S, k, dil, pad)
        assert_rounding_only(y, torch.where(ref > 0, ref, ref * 0.1), torch.bfloat16, ("skinny conv1", C, k, dil))
        del y, ref
    pad = (k - 1) // 2
    ref = dilated_conv_ref(x.float(), w2, b2, Bq, S, k, 1, pad)
    y = ops.conv_gemm(x, w2, b2, S, taps=k, pad=pad, res=res)
    assert _variant(ops, x, y, res, M, C, C, S, k, 1, ops.ACT_NONE, 0.0) == 4, "not the skinny kernel"
    assert_rounding_only(y, ref + res.double(), torch.bfloat16, ("skinny conv2+res", C, k))
    y = ops.conv_gemm(x, w2, b2, S, taps=k, pad=pad, res=res, out_scale=1.0 / 3)
    assert_rounding_only(y, (ref + res.double()) / 3, torch.bfloat16, ("skinny conv2+res /3", C, k))
    yold = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    want = yold.double() + (ref + res.double()) / 3
    y = ops.conv_gemm(x, w2, b2, S, taps=k, pad=pad, res=res, out=yold, accumulate=True, out_scale=1.0 / 3)
    assert y.data_ptr() == yold.data_ptr()
    assert_rounding_only(y, want, torch.bfloat16, ("skinny conv2+res /3 accumulate", C, k))


class _ConvTStub:
    """what hifigan.Generator._pack_convt reads from a layer"""

    def __init__(self, w, b):
        self.w, self.bias = w, b

    def effective_weight(self):
        return self.w


@pytest.mark.parametrize("cin,cout,k,u,T", [(512, 256, 16, 8, 900), (256, 128, 16, 8, 7200), (128, 64, 4, 2, 57600), (64, 32, 4, 2, 115200)])
def test_vocoder_polyphase_upsamplers_bf16(dev, cin, cout, k, u, T):
    """HiFi-GAN's four ConvTranspose1d layers (hifigan/models.py:124-131,152-153) as the product runs them - polyphase 3-tap
    contraction with N = u x Cout columns, leaky-ReLU prologue, bf16 - at batch-synthesis size (8 utterances x 900 frames),
    against the DEFINITION of the transposed convolution: y[q u + j - p] += x[q] W[:, :, j] (fp32 products, fp64 sums)."""
    ops = _ops()
    from fastspeech2_amd import hifigan
    Bq = 8
    g = torch.Generator().manual_seed(cin + k)
    w = (torch.randn(cin, cout, k, generator=g) * math.sqrt(u / (cin * k))).to(torch.bfloat16).float()
    b = torch.randn(cout, generator=g)
    wu, bu, taps, pad = hifigan.Generator._pack_convt(_ConvTStub(w, b), u, k, dev, torch.bfloat16)
    x = torch.randn(Bq * T, cin, generator=g).to(dev).to(torch.bfloat16)
    y = ops.conv_gemm(x, wu, bu, T, taps=taps, pad=pad, in_act=ops.ACT_LRELU, in_slope=0.1).view(Bq * T * u, cout)
    xa = torch.where(x.float() > 0, x.float(), x.float() * 0.1).to(torch.bfloat16).float().view(Bq, T, cin)
    p = (k - u) // 2
    ref = torch.zeros(Bq, T * u, cout, device=dev, dtype=torch.float64)
    wd = w.to(dev)
    q = torch.arange(T, device=dev)
    for j in range(k):
        tpos = q * u + j - p
        ok = (tpos >= 0) & (tpos < T * u)
        ref[:, tpos[ok]] += (xa[:, ok] @ wd[:, :, j]).double()             # (positions are distinct for distinct q)
    ref = (ref + b.to(dev).double()).view(Bq * T * u, cout)
    assert_rounding_only(y, ref, torch.bfloat16, ("polyphase convT", cin, cout, k, u))


def test_vocoder_conv_post_pcm_bf16_synthesis_size(dev):
    """fs2_conv_post_pcm on bf16 rows at batch-synthesis size (M = 8 x 230 400, C = 32, k = 7): leaky-ReLU with the DEFAULT slope
    0.01, conv_post, tanh (hifigan/models.py:161-163) against fp64; int16 PCM = numpy astype of the kernel's own float wave
    (utils/model.py:82-85), and within one LSB of the fp64 wave's."""
    import numpy as np
    from fastspeech2_amd import _lib
    ops = _ops()
    Bq, S, C, k = 8, 230400, 32, 7
    M = Bq * S
    g = torch.Generator().manual_seed(77)
    x = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(k, C, generator=g) * (1.2 / math.sqrt(C * k))).to(dev)
    bias = torch.tensor([0.05], device=dev)
    wav = torch.empty(M, device=dev)
    pcm = torch.empty(M, device=dev, dtype=torch.int16)
    _lib.call("fs2_conv_post_pcm", x.data_ptr(), x.stride(0), w.data_ptr(), bias.data_ptr(), 0.01, wav.data_ptr(), pcm.data_ptr(), 32768.0, M, S,
              C, k, 3, ops.dt(x), ops._stream())
    xa = torch.where(x.double() > 0, x.double(), x.double() * 0.01).view(Bq, S, C)
    acc = torch.zeros(Bq, S, device=dev, dtype=torch.float64)
    for j in range(k):
        sh = j - 3
        lo, hi = max(0, -sh), min(S, S - sh)
        acc[:, lo:hi] += xa[:, lo + sh:hi + sh] @ w[j].double()
    ref = torch.tanh(acc + bias.double()).view(M)
    assert ref.abs().max().item() < 0.9999                                 # (no int16 wrap in this case: tested bit-exactly elsewhere)
    err = (wav.double() - ref).abs().max().item()
    assert err < 5e-6, err
    got = pcm.cpu().numpy()
    assert np.array_equal(got, (wav.cpu().numpy() * 32768.0).astype("int16"))
    want = (ref.cpu().numpy() * 32768.0).astype("int16")
    assert np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1


def test_hifigan_bf16_per_stage_budget(dev):
    """The bf16 generator against bars DERIVED from bf16 itself (replaces round 2's 8 % whole-wave bar): every stage of the
    product (conv_pre, the four up-sampling stages with their residual blocks, conv_post) is fed into the fp64 oracle as that
    stage's INPUT, so a stage is judged on its own arithmetic.  For each stage three results of the same input exist - exact
    (fp64 activations, the bf16-rounded weights the product holds), EMULATED (the same with bf16 rounding at the product's storage
    points, oracle.hifigan_forward_stored) and the product's - and the bars are: product-to-exact <= 2 x emulated-to-exact (the
    price of bf16 storage, measured here, not chosen), product-to-emulated <= emulated-to-exact (they differ by accumulation
    order only).  The whole wave the same way."""
    from oracle import fs2_oracle as O
    from tests.test_oracle_golden import hifigan_shapes, hifigan_weights
    from tests.test_vocoder_stft_gpu import _generator

    keys = sorted(hifigan_shapes().keys())
    sd = hifigan_weights(9, keys)
    gen = _generator(sd, dev, dtype="bf16")
    Bq, T = 2, 64
    mel = torch.clamp(torch.randn(Bq, 80, T, generator=torch.Generator().manual_seed(1)) * 2 - 5, -11.5, 2.0)
    gen.stage_probe = []
    with torch.no_grad():
        wav = gen(mel.to(dev)).cpu().double()
    probes, gen.stage_probe = gen.stage_probe, None
    assert len(probes) == 5
    prod = [r.float().cpu().double().view(Bq, S, -1).transpose(1, 2).contiguous() for r, S in probes]     # (B, C, S) like the oracle
    sd64 = {k: v.double() for k, v in O.remove_weight_norm_sd(sd).items()}
    h = configs.HIFIGAN
    rel = lambda a, b: float((a - b).norm() / b.norm())
    with torch.no_grad():
        exact, emu = [], []
        inputs = [None] + prod                                               # stage i's input = the product's output of stage i-1
        wav_exact = O.hifigan_forward_stored(sd64, h, mel.double(), stages=exact, stage_inputs=inputs, weight_store=O.bf16_store)
        wav_emu = O.hifigan_forward_stored(sd64, h, mel.double(), store=O.bf16_store, stages=emu, stage_inputs=inputs,
                                           weight_store=O.bf16_store)
        full_exact = O.hifigan_forward_stored(sd64, h, mel.double(), weight_store=O.bf16_store)
        full_emu = O.hifigan_forward_stored(sd64, h, mel.double(), store=O.bf16_store, weight_store=O.bf16_store)
    for i in range(5):
        e = rel(emu[i], exact[i])
        pe, pm = rel(prod[i], exact[i]), rel(prod[i], emu[i])
        print(f"stage {i}: emulated-to-exact {e:.2e}  product-to-exact {pe:.2e}  product-to-emulated {pm:.2e}")
        assert 1e-4 < e < 2e-2, (i, e)                                       # bf16-sized
        assert pe <= 2 * e, (i, pe, e)
        assert pm <= e, (i, pm, e)
    # conv_post on the product's own last stage: fp32 arithmetic on bf16 rows
    assert (wav - wav_exact).abs().max().item() < 1e-5
    ew = rel(full_emu, full_exact)
    pw = rel(wav, full_exact)
    print(f"whole wave: emulated-to-exact {ew:.2e}  product-to-exact {pw:.2e}")
    assert pw <= 2 * ew, (pw, ew)


@pytest.mark.parametrize("name,K,S", [("fc", 256, 925), ("w_2", 1024, 925), ("fc enc", 256, 128)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_gemm_res_ln_matches_contraction_plus_layernorm(dev, name, K, S, p):
    """fs2_gemm_res_ln_fwd (the wide one-tap kernel with the LayerNorm epilogue) at the FFT blocks' production shapes, ragged lens +
    tile map, dropout on and off: the saved pre-norm sum z against an exact-product reference with the SAME dropout mask (read off
    fs2_ln_fwd's own stream: final bf16 rounding only), the statistics and the normalised output against fp64 LayerNorm of the
    product's stored z, padded rows exactly zero."""
    ops = _ops()
    g = torch.Generator().manual_seed(sum(ord(c) for c in name) + int(p * 10))
    M, N = B * S, 256
    lens = ragged_lens(S, seed=21).to(dev)
    tmap = ops.tile_map(lens, B, S)
    x = torch.randn(M, K, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(N, 1, K, generator=g) / math.sqrt(K)).to(dev).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev).to(torch.bfloat16)
    gamma = (torch.rand(N, generator=g) + 0.5).to(dev)
    beta = (torch.randn(N, generator=g) * 0.1).to(dev)
    seed = 0x1234567 + 77
    r = ops.gemm_res_ln(x, w, bias, res, gamma, beta, lens, tmap, B, S, p_pre=p, seed_pre=seed)
    assert r is not None, "shape not taken by the fused kernel"
    z, out, mean, rstd = r
    # the dropout mask of this (seed, element) stream: fs2_ln_fwd on ones
    ones = torch.ones(M, N, device=dev, dtype=torch.bfloat16)
    ops.ln_fwd(ones, None, gamma, beta, None, B, S, p_pre=p, seed_pre=seed)            # ones <- drop(ones) (z written back in place)
    mask = ones.double() if p > 0 else torch.ones(M, N, device=dev, dtype=torch.float64)
    if p > 0:
        keep = (mask != 0).double().mean().item()
        assert abs(keep - (1 - p)) < 5e-3 and torch.allclose(mask[mask != 0], torch.tensor(1.25, dtype=torch.float64, device=dev))
    y = conv_ref_gpu(x, w, bias, S, 0)
    pad = (torch.arange(S, device=dev).unsqueeze(0) >= lens.unsqueeze(1)).reshape(-1)
    # (z at padded rows is unspecified - zero in fully padded tiles - and never used: LayerNorm's backward zeroes those rows)
    assert_rounding_only(z[~pad], (y * mask + res.double())[~pad], torch.bfloat16, (name, p, "z"))
    assert torch.isfinite(z.float()).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    zd = z.double()
    mu = zd.mean(1, keepdim=True)
    var = ((zd - mu) ** 2).mean(1, keepdim=True)
    rs = (var + 1e-5).rsqrt()
    assert torch.allclose(mean.double()[~pad], mu.squeeze(1)[~pad], rtol=0, atol=2e-5) and torch.allclose(rstd.double()[~pad], rs.squeeze(1)[~pad], rtol=2e-5, atol=0)
    ref = (zd - mu) * rs * gamma.double() + beta.double()
    ref[pad] = 0
    assert_rounding_only(out, ref, torch.bfloat16, (name, p, "out"))
    assert (out[pad] == 0).all()
    # and against the two-launch path on the same inputs: identical statistics up to the one rounding the fused form saves
    y2 = ops.conv_gemm(x, w, bias, S, lens=lens, tmap=tmap)
    out2, mean2, rstd2 = ops.ln_fwd(y2, res, gamma, beta, lens, B, S, p_pre=p, seed_pre=seed)
    valid = ~pad
    assert ((out.float() - out2.float())[valid].abs().max().item()) <= 0.1 and ((out.float() - out2.float())[valid].norm() / out2.float()[valid].norm()).item() < 6e-3


@pytest.mark.parametrize("ks", [2, 4])
def test_splitk_contraction_matches_unsplit_reference(dev, ks):
    """the encoder's k=9 data gradient shape (M = 48 x 128, N = 256, K = 9 x 1024) through the K-split path: partial tiles stored
    into per-split f32 slabs (scratch: poisoned with NaN here), finalize launch (slab sum, residual, gate, padded rows)."""
    ops = _ops()
    S, Cin, Cout, k = 128, 1024, 256, 9
    M, pad = B * S, 4
    g = torch.Generator().manual_seed(77 + ks)
    lens = ragged_lens(S, seed=3).to(dev)
    tmap = ops.tile_map(lens, B, S)
    x = torch.randn(M, Cin, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(Cout, k, Cin, generator=g) / math.sqrt(Cin * k)).to(dev).to(torch.bfloat16)
    res = torch.randn(M, Cout, generator=g).to(dev).to(torch.bfloat16)
    ws = torch.full((ks, M, Cout), float("nan"), device=dev)
    ref = conv_ref_gpu(x, w, None, S, pad, lens=lens)
    valid = (torch.arange(S, device=dev).unsqueeze(0) < lens.unsqueeze(1)).reshape(-1, 1)
    for _ in range(2):                                                    # twice: the second call starts from the first one's slabs
        y = ops.conv_gemm(x, w, None, S, taps=k, pad=pad, res=res, lens=lens, tmap=tmap, ksplit=ks, ws=ws)
        assert_rounding_only(y, (ref + res.double()) * valid, torch.bfloat16, ("splitk res", ks))
    y = ops.conv_gemm(x, w, None, S, taps=k, pad=pad, act=ops.ACT_GATE, res=res, lens=lens, tmap=tmap, ksplit=ks, ws=ws)
    assert_rounding_only(y, torch.where(res.double() > 0, ref, torch.zeros_like(ref)) * valid, torch.bfloat16, ("splitk gate", ks))
    bias = torch.randn(Cout, generator=g).to(dev)
    y = ops.conv_gemm(x, w, bias, S, taps=k, pad=pad, act=ops.ACT_RELU, ksplit=ks, ws=ws)            # no lens, bias + ReLU
    assert_rounding_only(y, torch.relu(conv_ref_gpu(x, w, bias, S, pad)), torch.bfloat16, ("splitk relu", ks))


@pytest.mark.parametrize("Cin,Cout,k", [(256, 1024, 9), (1024, 256, 1), (512, 512, 5), (256, 768, 1), (80, 512, 5)])
def test_weight_gradient_production_shapes_bf16(dev, Cin, Cout, k):
    """conv_wgrad_bf16_kernel<3,0,8> / <3,2,8> / <1,0,4> at M = 44 400 with ragged lens: the split-K grids the bench runs."""
    ops = _ops()
    S, pad = 925, (k - 1) // 2
    M = B * S
    g = torch.Generator().manual_seed(Cin + k)
    lens = ragged_lens(S, seed=9).to(dev)
    valid = (torch.arange(S, device=dev).unsqueeze(0) < lens.unsqueeze(1)).reshape(-1, 1)
    x = torch.randn(M, Cin, generator=g).to(dev).to(torch.bfloat16)
    dy = (torch.randn(M, Cout, generator=g).to(dev) * valid).to(torch.bfloat16)       # contract: gradient rows >= lens are zero
    dw = torch.zeros(Cout, k, Cin, device=dev)
    db = torch.zeros(Cout, device=dev)
    ops.conv_wgrad(dy, x, dw, S, taps=k, pad=pad, lens=lens, dbias=db)
    xs, dys = x.float().view(B, S, Cin), dy.float().view(B, S, Cout)
    ref = torch.zeros(Cout, k, Cin, device=dev, dtype=torch.float64)
    for j in range(k):
        sh = j - pad
        lo, hi = max(0, -sh), min(S, S - sh)
        ref[:, j, :] = torch.einsum("bsn,bsc->nc", dys[:, lo:hi].double(), xs[:, lo + sh:hi + sh].double())
    scale = ref.abs().max().item()
    err = (dw.double() - ref).abs().max().item()
    assert err <= 1e-4 * scale, (err, scale)                       # exact bf16 products, fp32 accumulate + atomics
    fro = ((dw.double() - ref).norm() / ref.norm()).item()
    assert fro <= 2e-5, fro
    bref = dys.double().sum((0, 1))
    assert (db.double() - bref).abs().max().item() <= 1e-4 * bref.abs().max().item()


def test_attention_backward_bf16_at_full_length(dev):
    from tests.test_ops_gpu import attn_ref
    ops = _ops()
    S, H = 925, 2
    g = torch.Generator().manual_seed(3)
    lens = ragged_lens(S, seed=11)
    valid = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).reshape(-1)
    Bq = 8                                                                 # the reference needs B*H*S*S fp64 scores on the host
    qkv = torch.randn(Bq * S, 3 * H * 128, generator=g)
    dctx = torch.randn(Bq * S, H * 128, generator=g)
    dctx[~valid[:Bq * S]] = 0
    qd, dd = qkv.to(dev).to(torch.bfloat16), dctx.to(dev).to(torch.bfloat16)
    qr = qd.float().cpu().double().requires_grad_(True)
    ref = attn_ref(qr, lens[:Bq], Bq, S, H)
    ref.backward(dd.float().cpu().double())
    ctx, lse = ops.attn_fwd(qd, lens[:Bq].to(dev), Bq, S, H)
    dq = ops.attn_bwd(qd, ctx, dd, lse, lens[:Bq].to(dev), Bq, S, H).float().cpu().double()
    v = valid[:Bq * S]
    fro_c = ((ctx.float().cpu().double()[v] - ref.detach()[v]).norm() / ref.detach()[v].norm()).item()
    print(f"attention S=925 bf16: ctx rel-Frobenius {fro_c:.2e}")
    assert fro_c <= 6e-3, fro_c                                            # one bf16 rounding of P and of the output
    gref = qr.grad
    for name, sl in (("dq", slice(0, 256)), ("dk", slice(256, 512)), ("dv", slice(512, 768))):
        fro = ((dq[v][:, sl] - gref[v][:, sl]).norm() / gref[v][:, sl].norm()).item()
        print(f"attention S=925 bf16: {name} rel-Frobenius {fro:.2e}")
        assert fro <= 1.2e-2, (name, fro)                                  # bf16 P, dS and ctx feed the five products
    assert not dq[~v].any()


# ------------------------------------------------------------------------------------------------ normalisation kernels
@pytest.mark.parametrize("form", ["residual", "predictor"])
def test_layernorm_production_shape_bf16(dev, form):
    """ln_fwd_c256_bf16_kernel / ln_bwd_c256_bf16_kernel (half a wave per row, 16-byte lanes, DPP row sums) at 48 x 925 rows,
    C = 256, against an fp64 restatement on the device: outputs within bf16 rounding, affine gradients to fp32 accumulation.
    "residual": dropout-free add + LayerNorm + pad mask with an upstream gradient added into d1 (the FFT block form);
    "predictor": ReLU'd input, no residual, no lens, ReLU backward fused into d2 (the variance predictor form)."""
    ops = _ops()
    S, C = 925, 256
    M = B * S
    g = torch.Generator().manual_seed(31)
    resid = form == "residual"
    lens = ragged_lens(S, seed=9).to(dev) if resid else None
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(dev).to(torch.bfloat16)
    if not resid:
        y = torch.relu(y)
    res = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16) if resid else None
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    dout = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    d1a = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16) if resid else None
    z = y.double() + (res.double() if resid else 0)
    zr = z.to(torch.bfloat16).double()                                     # the kernel normalises z as stored
    valid = (torch.arange(S, device=dev).unsqueeze(0) < lens.unsqueeze(1)).reshape(-1, 1).double() if resid else torch.ones(M, 1, device=dev, dtype=torch.float64)
    mu = zr.mean(1, keepdim=True)
    rstd = (((zr - mu) ** 2).mean(1, keepdim=True) + 1e-5).rsqrt()
    xh = (zr - mu) * rstd
    o_ref = (xh * gamma.double() + beta.double()) * valid
    gdo = dout.double() * valid
    gg = gdo * gamma.double()
    dz = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    o, mean, rs = ops.ln_fwd(y, res, gamma, beta, lens, B, S)
    assert torch.equal(y.double(), zr)                                     # z written back (bf16) for backward
    assert_rounding_only(o, o_ref, torch.bfloat16, (form, "out"))
    assert torch.allclose(mean.double(), mu.squeeze(1), rtol=0, atol=1e-5) and torch.allclose(rs.double(), rstd.squeeze(1), rtol=1e-5, atol=0)
    dg = torch.zeros(C, device=dev); db = torch.zeros(C, device=dev)
    d1, d2 = ops.ln_bwd(y, dout, gamma, lens, mean, rs, dg, db, B, S, want_d1=resid, want_d2=True, d1_add=d1a, relu_bwd=not resid)
    if resid:
        assert_rounding_only(d1, dz + d1a.double(), torch.bfloat16, (form, "d1"))
        assert_rounding_only(d2, dz, torch.bfloat16, (form, "d2"))
    else:
        assert_rounding_only(d2, dz * (zr > 0), torch.bfloat16, (form, "d2 relu"))
    for got, ref, nm in ((dg, (gdo * xh).sum(0), "dgamma"), (db, gdo.sum(0), "dbeta")):
        assert ((got.double() - ref).norm() / ref.norm()).item() < 1e-5, (form, nm)
    # the upstream gradient as a PAIR (fs2_ln_bwd_sum: dout + dout2 added while the rows are read - round 6: the FFT blocks'
    # residual-branch gradient no longer goes through a contraction epilogue): every output against fp64 of the summed gradient
    dout2 = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    gdo2 = (dout.double() + dout2.double()) * valid
    gg2 = gdo2 * gamma.double()
    dzs = rstd * (gg2 - gg2.mean(1, keepdim=True) - xh * (gg2 * xh).mean(1, keepdim=True))
    dg2 = torch.zeros(C, device=dev); db2 = torch.zeros(C, device=dev)
    e1, e2 = ops.ln_bwd(y, dout, gamma, lens, mean, rs, dg2, db2, B, S, want_d1=resid, want_d2=True, d1_add=d1a, relu_bwd=not resid, dout2=dout2)
    if resid:
        assert_rounding_only(e1, dzs + d1a.double(), torch.bfloat16, (form, "d1, pair"))
        assert_rounding_only(e2, dzs, torch.bfloat16, (form, "d2, pair"))
    else:
        assert_rounding_only(e2, dzs * (zr > 0), torch.bfloat16, (form, "d2 relu, pair"))
    for got, ref, nm in ((dg2, (gdo2 * xh).sum(0), "dgamma"), (db2, gdo2.sum(0), "dbeta")):
        assert ((got.double() - ref).norm() / ref.norm()).item() < 1e-5, (form, nm, "pair")
    # dropout forms: the backward regenerates the forward's masks (d2 is zero exactly where the pre-LN dropout dropped y)
    y2 = (torch.randn(M, C, generator=g) + 2.0).to(dev).to(torch.bfloat16)          # away from 0: a zero in z - res marks a dropped element
    y2[y2 == 0] = 1.0                                                                # (11 M samples: one does land on 0)
    r2 = torch.zeros(M, C, device=dev, dtype=torch.bfloat16)
    o2, m2, s2 = ops.ln_fwd(y2, r2, gamma, beta, lens, B, S, p_pre=0.2, seed_pre=4321)
    dropped = y2 == 0
    assert abs(dropped.float().mean().item() - 0.2) < 5e-3
    dg.zero_(); db.zero_()
    _, dd2 = ops.ln_bwd(y2, dout, gamma, lens, m2, s2, dg, db, B, S, want_d1=True, want_d2=True, p_pre=0.2, seed_pre=4321)
    assert not dd2[dropped].any()
    live_rows = valid.squeeze(1) > 0
    assert (dd2[live_rows][~dropped[live_rows]] != 0).float().mean().item() > 0.99


@pytest.mark.parametrize("C", [512, 80])
def test_batchnorm_production_shape_bf16(dev, C):
    """bn_rows_kernel<.., V = 8> (16-byte lanes) at M = 44 400 rows, the PostNet's two widths: statistics, apply + tanh, both
    backward passes against fp64 on the device."""
    ops = _ops()
    M = B * 925
    g = torch.Generator().manual_seed(41 + C)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dev).to(torch.bfloat16)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.1).to(dev)
    dout = torch.randn(M, C, generator=g).to(dev).to(torch.bfloat16)
    xd = x.double()
    mu = xd.mean(0, keepdim=True)
    var = ((xd - mu) ** 2).mean(0, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    xh = (xd - mu) * rstd
    t = torch.tanh(xh * gamma.double() + beta.double())
    rm = torch.zeros(C, device=dev); rv = torch.ones(C, device=dev)
    out, mean_rstd = ops.bn_train_fwd(x, gamma, beta, rm, rv, ops.ACT_TANH, 0.0, 0)
    assert torch.allclose(mean_rstd[:C].double(), mu.squeeze(0), rtol=0, atol=2e-5) and torch.allclose(mean_rstd[C:].double(), rstd.squeeze(0), rtol=2e-5, atol=0)
    assert torch.allclose(rm.double(), 0.1 * mu.squeeze(0), rtol=1e-4, atol=1e-6)
    assert torch.allclose(rv.double(), 0.9 + 0.1 * var.squeeze(0) * M / (M - 1), rtol=1e-4, atol=0)
    assert_rounding_only(out, t, torch.bfloat16, (C, "tanh(bn(x))"))
    gq = dout.double() * (1 - t * t)
    dgam, dbet = (gq * xh).sum(0), gq.sum(0)
    dx_ref = gamma.double() * rstd * (gq - dbet / M - xh * dgam / M)
    dx, dgamma, dbeta = ops.bn_bwd(x, dout, mean_rstd, gamma, beta, ops.ACT_TANH, 0.0, 0)
    assert_rounding_only(dx, dx_ref, torch.bfloat16, (C, "dx"))
    assert ((dgamma.double() - dgam).norm() / dgam.norm()).item() < 1e-4 and ((dbeta.double() - dbet).norm() / dbet.norm()).item() < 1e-4


# ------------------------------------------------------------------------------------------------ whole train step
# the full-size case (fp64 oracle of the whole step) lives in tests/conftest.py: the bf16 budget test, collected LAST
# (tests/test_z_bf16_budget_gpu.py), shares it
from tests.conftest import train_step_grads as _train_step  # noqa: E402


def test_full_size_train_step_fp32_matches_fp64_oracle_elementwise(dev, full_case):
    pcfg, mcfg, sd, b, oout, olosses, ograds = full_case
    out, losses, grads = _train_step(dev, pcfg, mcfg, sd, b, "fp32")
    assert torch.equal(out[9].cpu(), oout[9]) and torch.equal(out[7].cpu(), oout[7])
    for i in (0, 1):
        l1 = (out[i].detach().float().cpu().double() - oout[i].detach()).abs().mean().item()
        assert l1 < 1e-4, (i, l1)                                           # north_star bar
    for a, o in zip(losses, olosses):
        assert abs(a.item() - o.item()) <= 1e-5 * max(1.0, abs(o.item()))
    assert sorted(grads) == sorted(ograds)
    gmax = max(g.abs().max().item() for g in ograds.values())
    for n, og in ograds.items():
        scale = og.abs().max().item()
        err = (grads[n] - og).abs().max().item()
        if scale < 1e-9 * gmax:
            # TRUE gradient zero (w_ks.bias: softmax is shift-invariant; conv biases in front of BatchNorm: the batch mean absorbs
            # them; fp64 leaves ~1e-15): only rounding noise can be there
            assert err <= 1e-6 * gmax, (n, err, gmax)
            continue
        assert err <= 2e-3 * scale, (n, err, scale)
        fro = ((grads[n] - og).norm() / og.norm()).item()
        assert fro <= 1e-3, (n, fro)
