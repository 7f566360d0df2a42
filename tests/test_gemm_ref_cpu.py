"""CPU: the checker of the contraction tests is itself checked (tests/gemm_ref.py, used by tests/test_gemm_dispatch_gpu.py).

  * the exact-product reference equals fp64 F.conv1d (+ a plainly written epilogue) to 1e-12 - dilation, asymmetric left pad,
    ragged lens and every epilogue form the kernels have;
  * the rounding-only bound accepts the reference rounded once to bf16 / fp32;
  * it rejects six injected faults of the kind a contraction kernel makes at ONE place (a tap dropped on a sequence's first row,
    a tap read across a sequence boundary, a padded row left non-zero, bias missing in the last N % 8 columns, the residual added
    after out_scale, an accumulate that overwrites), each by at least 10 x the bound - and a NaN;
  * the case table is well formed (K <= 9216, legal channel counts, unique ids, both sides of every pair present).
"""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G

DT = [torch.bfloat16, torch.float32]


def _inputs(Bq, S, Cin, N, taps, seed, dtype=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Bq * S, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(N, taps, Cin, generator=g, dtype=torch.float64) / (Cin * taps) ** 0.5
    sign = lambda *s: torch.where(torch.rand(*s, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    bias = sign(N) * (1 + torch.rand(N, generator=g, dtype=torch.float64))          # |.| in [1, 2): a missing term is never small
    res = sign(Bq * S, N) * (1 + torch.rand(Bq * S, N, generator=g, dtype=torch.float64))
    old = sign(Bq * S, N) * (1 + torch.rand(Bq * S, N, generator=g, dtype=torch.float64))
    if dtype is not None:                                                             # the values a kernel of that type would read
        x, w, res, old = (t.to(dtype).double() for t in (x, w, res, old))
        bias = bias.float().double()
    return x, w, bias, res, old


def _conv1d(x, w, S, dil, pad):
    """fp64 F.conv1d on rows: x [Bq*S][Cin], w [N][taps][Cin], left pad `pad`, output length S"""
    Bq = x.shape[0] // S
    taps = w.shape[1]
    xx = F.pad(x.view(Bq, S, -1).transpose(1, 2), (pad, (taps - 1) * dil - pad))
    return F.conv1d(xx, w.permute(0, 2, 1).contiguous(), None, dilation=dil).transpose(1, 2).reshape(Bq * S, -1)


EPILOGUES = ["none", "bias", "bias_relu", "bias_lrelu", "bias_tanh", "res", "gate", "res_scale", "accumulate", "lrelu_io", "in_act"]


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("taps,dil,pad", [(1, 1, 0), (3, 1, 1), (5, 1, 0), (5, 1, 4), (4, 1, 0), (7, 3, 9), (7, 3, 4), (11, 5, 50), (9, 1, 4), (2, 17, 8)])
@pytest.mark.parametrize("with_lens", [False, True])
def test_reference_equals_fp64_conv1d(epi, taps, dil, pad, with_lens):
    Bq, S, Cin, N = 4, 23, 12, 11
    x, w, bias, res, old = _inputs(Bq, S, Cin, N, taps, seed=taps * 100 + dil * 10 + pad)
    lens = torch.tensor([S, 0, 1, 9]) if with_lens else None
    s = G.f32(1.0 / 3)
    xin = torch.where(x > 0, x, x * G.f32(0.1)) if epi == "in_act" else x
    acc = _conv1d(xin, w, S, dil, pad)
    kw = {}
    if epi == "none":
        want = acc
    elif epi in ("bias", "in_act"):
        want, kw = acc + bias, dict(bias=bias)
        if epi == "in_act":
            kw.update(in_act=G.ACT_LRELU, in_slope=0.1)
    elif epi == "bias_relu":
        want, kw = (acc + bias).clamp_min(0), dict(bias=bias, act=G.ACT_RELU)
    elif epi == "bias_lrelu":
        v = acc + bias
        want, kw = torch.where(v > 0, v, v * G.f32(0.1)), dict(bias=bias, act=G.ACT_LRELU, slope=0.1)
    elif epi == "bias_tanh":
        want, kw = torch.tanh(acc + bias), dict(bias=bias, act=G.ACT_TANH)
    elif epi == "res":
        want, kw = acc + bias + res, dict(bias=bias, res=res)
    elif epi == "gate":
        want, kw = acc * (res > 0), dict(act=G.ACT_GATE, res=res)
    elif epi == "res_scale":
        want, kw = (torch.relu(acc + bias) + res) * s, dict(bias=bias, act=G.ACT_RELU, res=res, out_scale=1.0 / 3)
    elif epi == "accumulate":
        want, kw = (acc + bias) * s, dict(bias=bias, out_scale=1.0 / 3, old=old)
    elif epi == "lrelu_io":
        r = torch.where(res > 0, res, res * G.f32(10.0))
        want, kw = (acc + bias + r) * s, dict(bias=bias, res=res, out_scale=1.0 / 3, res_unlrelu=10.0, post_slope=0.1, old=old)
    if with_lens:
        want = want.clone()
        want[G.pad_rows(lens, Bq, S)] = 0
    if "old" in kw:
        want = want + old
    if epi == "lrelu_io":
        want = torch.where(want > 0, want, want * G.f32(0.1))
    got = G.conv_reference(x, w, kw.pop("bias", None), S, dil=dil, pad=pad, lens=lens, **kw)
    assert got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    if with_lens and "old" not in kw:
        assert (got[G.pad_rows(lens, Bq, S)] == 0).all()                 # exact zeros


def test_prologue_is_rounded_to_the_storage_type():
    x, w, *_ = _inputs(2, 9, 8, 5, 3, seed=1, dtype=torch.bfloat16)
    xa = torch.where(x.float() > 0, x.float(), x.float() * 0.1).to(torch.bfloat16)
    want = _conv1d(xa.double(), w, 9, 1, 1)
    got = G.conv_acc(x.to(torch.bfloat16), w.to(torch.bfloat16), 9, 1, 1, G.ACT_LRELU, 0.1)
    assert (got - want).abs().max().item() <= 1e-5                       # (fp32 matmul of exact products)
    assert (G.conv_acc(x, w, 9, 1, 1, G.ACT_LRELU, 0.1, store=torch.bfloat16) - want).abs().max().item() <= 1e-12


def test_dgrad_weight_is_the_transposed_flip():
    """conv with dgrad_weight(w) and pad' = (k-1) dil - pad is the autograd gradient of the forward conv"""
    Bq, S, Cin, N, taps, dil, pad = 2, 17, 8, 6, 5, 2, 3
    x, w, *_ = _inputs(Bq, S, Cin, N, taps, seed=5)
    dy = torch.randn(Bq * S, N, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    xr = x.clone().requires_grad_(True)
    _conv1d(xr, w, S, dil, pad).backward(dy)
    got = G.conv_reference(dy, G.dgrad_weight(w), None, S, dil=dil, pad=(taps - 1) * dil - pad)
    assert (got - xr.grad).abs().max().item() <= 1e-12


@pytest.mark.parametrize("dtype", DT)
def test_bound_accepts_one_rounding(dtype):
    x, w, bias, res, old = _inputs(3, 40, 64, 83, 5, seed=11, dtype=dtype)
    for kw in (dict(), dict(act=G.ACT_RELU), dict(res=res, out_scale=1.0 / 3), dict(old=old), dict(act=G.ACT_TANH)):
        ref = G.conv_reference(x, w, bias, 40, pad=2, lens=torch.tensor([40, 0, 1]), **kw)
        y = ref.to(dtype)
        G.assert_rounding_only(y, ref, dtype, "rounded once")
        assert G.rounding_ratio(y, ref, dtype) <= (1.0 if dtype == torch.bfloat16 else 1.0 / 16)    # half a spacing: 2^-8 |ref| at most in bf16, 2^-24 in fp32
    assert G.rounding_ratio(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.float64), dtype) == 0.0


FAULTS = ["tap dropped on a first row", "tap read across a sequence boundary", "padded row left non-zero", "bias missing in the last N % 8 columns",
          "residual added after out_scale", "accumulate overwrites", "one NaN"]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("fault", FAULTS)
def test_bound_rejects_single_place_faults(fault, dtype):
    Bq, S, Cin, N, taps, pad = 3, 40, 64, 83, 5, 2
    x, w, bias, res, old = _inputs(Bq, S, Cin, N, taps, seed=23, dtype=dtype)
    lens = torch.tensor([S, 17, 1])
    where = None
    if fault == "tap dropped on a first row":
        ref = G.conv_reference(x, w, bias, S, pad=pad)
        y = ref.clone()
        y[S] -= x[S + (3 - pad)] @ w[:, 3].t()                              # tap 3 of sequence 1's row 0 reads its row 1
        where = (slice(S, S + 1), slice(None))
    elif fault == "tap read across a sequence boundary":
        ref = G.conv_reference(x, w, bias, S, pad=pad)
        y = ref.clone()
        y[S] += x[S - pad] @ w[:, 0].t()                                    # tap 0 of sequence 1's row 0: row S - 2 of sequence 0
        where = (slice(S, S + 1), slice(None))
    elif fault == "padded row left non-zero":
        ref = G.conv_reference(x, w, bias, S, pad=pad, lens=lens)
        y = ref.clone()
        y[S + 17] = G.conv_reference(x, w, bias, S, pad=pad)[S + 17]        # the first padded row of sequence 1
        where = (slice(S + 17, S + 18), slice(None))
    elif fault == "bias missing in the last N % 8 columns":
        ref = G.conv_reference(x, w, bias, S, pad=pad)
        y = ref.clone()
        y[:, N - N % 8:] -= bias[N - N % 8:]
        where = (slice(None), slice(N - N % 8, N))
    elif fault == "residual added after out_scale":
        ref = G.conv_reference(x, w, bias, S, pad=pad, res=res, out_scale=1.0 / 3)
        y = G.conv_reference(x, w, bias, S, pad=pad, out_scale=1.0 / 3) + res
    elif fault == "accumulate overwrites":
        ref = G.conv_reference(x, w, bias, S, pad=pad, out_scale=1.0 / 3, old=old)
        y = G.conv_reference(x, w, bias, S, pad=pad, out_scale=1.0 / 3)
    else:
        ref = G.conv_reference(x, w, bias, S, pad=pad)
        y = ref.clone()
        y[7, 5] = float("nan")
    y = y.to(dtype)                                                          # the faulty kernel still rounds its result
    with pytest.raises(AssertionError):
        G.assert_rounding_only(y, ref, dtype, fault)
    err = (y.double() - ref).abs()
    ratio = (err / G.rounding_bound(ref, dtype)).nan_to_num(nan=float("inf"))
    if fault in ("residual added after out_scale", "accumulate overwrites", "bias missing in the last N % 8 columns"):
        sel = ratio[where] if where is not None else ratio
        assert sel.min().item() >= 10, (fault, sel.min().item())            # EVERY affected element is far outside
    elif where is not None:
        assert ratio[where].max().item() >= 10, (fault, ratio[where].max().item())
        rest = ratio.clone()
        rest[where] = 0
        assert rest.max().item() <= 1.0                                      # and nothing else is flagged
    assert G.rounding_ratio(y, ref, dtype) >= 10


def test_case_table_is_well_formed():
    for cus in (256, 304, 64):
        table = G.case_table(cus)
        ids = [(c.dtype, c.shape, c.pair, c.side) for c in table]
        assert len(set(ids)) == len(ids)
        fam = {c.family for c in table}
        assert fam == {"single", "stft", "edge", "pair", "ops13"}, fam
        pairs = {}
        for c in table:
            assert c.taps * c.Cin <= G.K_MAX and c.Cin % c.epc == 0 and 0 <= c.pad <= (c.taps - 1) * c.dil and c.Bq >= 1 and c.S >= 1
            assert c.ldy >= c.N + c.epc - (c.epc - 1) and (c.ldy % c.epc == 0) == (not c.ldy_odd)
            if c.pair:
                pairs.setdefault(c.pair, set()).add(c.side)
        assert len(pairs) >= 40 and all(s == {"a", "b"} for s in pairs.values()), {k: v for k, v in pairs.items() if v != {"a", "b"}}
    t = G.case_table(256)
    # the families the issue names: the model's shapes at every single-utterance length, both dtypes
    assert sum(c.family == "single" for c in t) == 2 * len(G.MODEL_SHAPES) * 9
    assert {c.S for c in t if c.family == "single" and c.Bq == 1} == {1, 7, 50, 127, 128, 129, 257, 800}
    assert sum(c.family == "ops13" for c in t) == 2 * len(set(G.OPS_FWD_SHAPES + G.OPS_GRAD_SHAPES)) == 2 * 12    # (13 listed, one shared by both tests)
    edge = [c for c in t if c.family == "edge"]
    assert {c.M for c in edge} >= {127, 128, 129, 255, 256, 257}
    assert {c.N for c in edge} >= {1, 3, 8, 80, 127, 128, 129, 136, 1026}
    assert {c.Cin for c in edge if c.dtype == "bf16"} >= {8, 24, 72, 80, 136} and {c.Cin for c in edge if c.dtype == "fp32"} >= {4, 12}
    assert {c.taps for c in edge} >= {1, 2, 3, 4, 9, 17, 32, 33}
    assert any(c.S < c.taps for c in edge) and any(c.S < c.pad for c in edge) and any(c.S == 1 for c in edge)
    assert any(c.family == "stft" and (c.dtype, c.Cin, c.taps, c.pad, c.N) == ("fp32", 256, 4, 0, 1026) for c in t)
