"""CPU self-test of tests/attn_ref.py: the fp64 reference is the op, and its elementwise bound accepts a computation that
rounds where the bf16 kernels round but rejects the two faults the bound exists for (a padded key that leaks into the
softmax; a running maximum that is not raised)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attn_ref as A

LOG2E = 1.4426950408889634


def _qkv_split(qkv, B, S, H):
    q, k, v = qkv.view(B, S, 3, H, A.DK).unbind(2)
    return [t.permute(0, 2, 1, 3) for t in (q, k, v)]                    # [B][H][S][128]


def test_reference_matches_sdpa_forward_and_autograd():
    B, S, H = 3, 70, 2
    lens = torch.tensor([70, 33, 1], dtype=torch.int32)
    qkv, dctx = A.make_inputs(B, S, H, lens, torch.float64, "cpu", seed=1, pad="leak")
    ref = A.reference(qkv, lens, B, S, H, dctx, dtype=torch.float32)
    x = qkv.clone().requires_grad_(True)
    q, k, v = _qkv_split(x, B, S, H)
    keep = (torch.arange(S).view(1, 1, 1, S) < lens.view(B, 1, 1, 1))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=keep)
    o = o.permute(0, 2, 1, 3).reshape(B * S, H * A.DK)
    v_rows = ref["valid"]
    torch.testing.assert_close(ref["ctx"][v_rows], o.detach()[v_rows], rtol=1e-12, atol=1e-12)
    s = (q @ k.transpose(-1, -2)) * A.SCALE
    lse = torch.logsumexp(s.masked_fill(~keep, -math.inf), -1).detach()
    vl = keep.squeeze(2).expand(B, H, S)
    torch.testing.assert_close(ref["lse"][vl], lse[vl], rtol=1e-12, atol=1e-12)
    assert not ref["lse"][~vl].any() and not ref["ctx"][~v_rows].any()
    o.backward(dctx)
    torch.testing.assert_close(ref["dqkv"], x.grad, rtol=1e-10, atol=1e-12)
    assert not ref["dqkv"][~v_rows].any()


def _emulate_bf16(qkv, lens, B, S, H, dctx, stale_max=False):
    """The bf16 kernels' arithmetic on the CPU: fp32 scores of the bf16 operands; forward over 64-key tiles with the lazy
    running maximum (raised, accumulators rescaled, only when some query of a 32-query wave gained > 8 log2 units - or, with
    stale_max, only on the first tile), P rounded to bf16 before P V, ctx rounded to bf16, natural-log lse; backward from the
    rounded ctx and the fp32 lse with P and dS rounded to bf16 before their products, outputs rounded to bf16."""
    bf = torch.bfloat16
    L = A._lens_list(lens, B, S)
    x = qkv.float().view(B, S, 3, H, A.DK)
    g = dctx.float().view(B, S, H, A.DK)
    ctx = torch.zeros(B, S, H, A.DK, dtype=bf)
    lse_o = torch.zeros(B, H, S)
    dqkv = torch.zeros(B, S, 3, H, A.DK, dtype=bf)
    sc2 = torch.tensor(A.SCALE * LOG2E, dtype=torch.float32)
    for b, n in enumerate(L):
        if n == 0:
            continue
        q, k, v = (x[b, :n, i].transpose(0, 1) for i in range(3))
        s = q @ k.transpose(1, 2)
        m = torch.full((H, n), -math.inf)
        l = torch.zeros(H, n)
        o = torch.zeros(H, n, A.DK)
        nw = (n + 31) // 32
        for k0 in range(0, n, 64):
            st = s[:, :, k0:k0 + 64]
            mx = st.max(-1).values * sc2
            need = F.pad(mx > m + 8.0, (0, 32 * nw - n)).view(H, nw, 32).any(-1)          # the wave's ballot
            need = need.repeat_interleave(32, 1)[:, :n]
            if stale_max:
                need &= torch.isinf(m)
            mn = torch.where(need, torch.maximum(m, mx), m)
            alpha = torch.where(need, torch.exp2(m - mn), torch.ones_like(m))
            l, o, m = l * alpha, o * alpha.unsqueeze(-1), mn
            p = torch.exp2(st * sc2 - m.unsqueeze(-1))
            l = l + p.sum(-1)
            o = o + p.to(bf).float() @ v[:, k0:k0 + 64]
        ob = (o / l.unsqueeze(-1)).to(bf)
        ctx[b, :n] = ob.transpose(0, 1)
        ls = m * math.log(2.0) + torch.log(l)
        lse_o[b, :, :n] = ls
        do = g[b, :n].transpose(0, 1)
        delta = (do * ob.float()).sum(-1, keepdim=True)
        p = torch.exp2(s * sc2 - (ls * LOG2E).unsqueeze(-1))
        ds = (p * (do @ v.transpose(1, 2) - delta)).to(bf).float()
        pb = p.to(bf).float()
        dqkv[b, :n, 0] = (A.SCALE * (ds @ k)).transpose(0, 1).to(bf)
        dqkv[b, :n, 1] = (A.SCALE * (ds.transpose(1, 2) @ q)).transpose(0, 1).to(bf)
        dqkv[b, :n, 2] = (pb.transpose(1, 2) @ do).transpose(0, 1).to(bf)
    return ctx.view(B * S, H * A.DK), lse_o, dqkv.view(B * S, 3 * H * A.DK)


CASES = [  # (B, S, H, lens, regime, pad)
    (3, 150, 2, [150, 97, 1], "randn", "leak"),
    (2, 130, 1, [130, 65], "peaked", "randn"),
    (2, 130, 1, [130, 64], "flat", "randn"),
    (3, 257, 2, [257, 200, 64], "rising", "randn"),
]


@pytest.mark.parametrize("B,S,H,lens,regime,pad", CASES)
def test_bound_accepts_bf16_rounding(B, S, H, lens, regime, pad):
    lens = torch.tensor(lens, dtype=torch.int32)
    qkv, dctx = A.make_inputs(B, S, H, lens, torch.bfloat16, "cpu", seed=7, regime=regime, pad=pad)
    ref = A.reference(qkv, lens, B, S, H, dctx)
    ctx, lse, dqkv = _emulate_bf16(qkv, lens, B, S, H, dctx)
    r = A.check_all(ref, ctx, lse, dqkv, torch.bfloat16, H, what=f"emulated bf16 {regime}/{pad}")
    print(f"emulated bf16 {regime}/{pad}: max err/(u mag) " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r[k] for k in ("ctx", "dq", "dk", "dv")) > 0.05                   # the rounding is visible: not a vacuous pass


def test_bound_rejects_one_leaked_padded_key():
    B, S, H = 2, 150, 2
    lens = torch.tensor([150, 97], dtype=torch.int32)
    qkv, dctx = A.make_inputs(B, S, H, lens, torch.bfloat16, "cpu", seed=9, pad="leak")
    ref = A.reference(qkv, lens, B, S, H, dctx)
    leaked = A.reference(qkv, torch.tensor([150, 98], dtype=torch.int32), B, S, H, dctx)     # key 97 of sequence 1 unmasked
    v = ref["valid"]
    with pytest.raises(AssertionError, match="ctx"):
        A.bound_ratio(leaked["ctx"][v].to(torch.bfloat16), ref["ctx"][v], ref["ctx_mag"][v], torch.bfloat16, what="ctx")
    with pytest.raises(AssertionError, match="lse"):
        A.check_lse(leaked["lse"].float(), ref, what="lse")
    d = leaked["dqkv"].clone()
    d[~v] = 0
    with pytest.raises(AssertionError, match="dq"):
        A.check_all(ref, ref["ctx"], ref["lse"], d.to(torch.bfloat16), torch.bfloat16, H)


def test_bound_rejects_a_stale_running_maximum():
    B, S, H = 2, 257, 2
    lens = torch.tensor([257, 200], dtype=torch.int32)
    qkv, dctx = A.make_inputs(B, S, H, lens, torch.bfloat16, "cpu", seed=11, regime="rising")
    ref = A.reference(qkv, lens, B, S, H, dctx)
    ctx, lse, _ = _emulate_bf16(qkv, lens, B, S, H, dctx, stale_max=True)
    v = ref["valid"]
    with pytest.raises(AssertionError, match="ctx"):
        A.bound_ratio(ctx[v], ref["ctx"][v], ref["ctx_mag"][v], torch.bfloat16, what="ctx")


def test_inputs_reach_the_edges_they_are_for():
    """the score regimes and paddings of make_inputs do what the GPU tests rely on"""
    B, S, H = 2, 257, 1
    lens = torch.tensor([257, 150], dtype=torch.int32)
    qkv, _ = A.make_inputs(B, S, H, lens, torch.float64, "cpu", seed=3, regime="rising")
    q, k, _ = _qkv_split(qkv, B, S, H)
    s = (q[0, 0] @ k[0, 0].T) * A.SCALE * LOG2E                                       # log2 units, sequence 0
    first = s[:, :64].max(-1).values
    gain = s.max(-1).values - first
    assert (gain > 128).any() and (gain < 8).any()                     # rescale past fp32 range for some, none for others
    per_tile = torch.stack([s[:, k0:k0 + 64].max(-1).values for k0 in range(0, 256, 64)], 1).diff(dim=1)
    assert (per_tile > 8).all(-1).any()                                # a new maximum > 8 log2 units up in every full tile
    assert (torch.exp2((s - s.max(-1, keepdim=True).values).float()) == 0).any()   # p of far keys underflows fp32
    for pad, lo, hi in (("leak", 10, 20), ("overflow", 88.8, 130)):
        qkv, _ = A.make_inputs(B, S, H, lens, torch.bfloat16, "cpu", seed=3, pad=pad)
        q, k, v = (t.double() for t in _qkv_split(qkv, B, S, H))
        s = (q[1, 0, :150] @ k[1, 0].T) * A.SCALE
        margin = s[:, 150:].min(-1).values - s[:, :150].max(-1).values   # padded key over every valid key
        lse = torch.logsumexp(s[:, :150], -1)
        assert margin.min() > (lo if pad == "leak" else 0) and margin.max() < hi
        if pad == "overflow":
            assert ((s[:, 150:] - lse.unsqueeze(-1)) * LOG2E).min() > 128
        assert (v[1, 0, 150:] > 90).all()
