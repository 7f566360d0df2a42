"""fp64 reference of the fused attention (fs2_attn_fwd / fs2_attn_bwd) and a per-element running-error bound for it.

The op (transformer/Modules.py:14-25 with the key-padding mask of SubLayers.py): per (sequence, head)
    ctx = softmax(q k^T / sqrt(128), keys j >= len masked) @ v,   lse = logsumexp of the scaled scores (natural log),
and its gradients dq, dk, dv for an upstream dctx whose rows >= len are zero (the engine's contract: ln_bwd zeroes them).

The bound is elementwise and NOT normalised by a maximum or a norm:
    |kernel - ref| <= c * u * mag + FLOOR
with u = 2^-8 (bf16) or 2^-20 (fp32) and `mag` the same contraction taken over absolute values:
    ctx: sum_j w_ij |v_j|          dV: sum_i w_ij |dO_i|
    dQ:  scale sum_j m_ij |k_j|    dK: scale sum_i m_ij |q_i|      m_ij = w_ij (|dO_i|.|v_j| + sum_d |dO_id o_id|)
w_ij is the probability p_ij widened by the error of its exponent: the kernels evaluate exp(s_ij - lse_i) from fp32 scores,
and the absolute error of that argument grows with the absolute-value score scale * |q_i|.|k_j| and with |lse_i|.  A score is
a 128-term fp32 sum accumulated over 64 MFMA steps (fp32 kernels), so its rounding error grows like sqrt(64) half-ulps of the
partial sums: EPS_ARG = 4 * 2^-24 per unit of (|q_i|.|k_j| scale + |lse_i|).  Relative to u that is 2^-14 in bf16
(invisible) and 1/4 in fp32, where scores of +-60 (the 'rising' inputs) would otherwise exceed any fixed multiple of u.
FLOOR only absorbs probabilities below the fp32 range (p < 2^-126 are flushed to 0 by the kernels).
"""
import math

import torch

DK = 128
SCALE = DK ** -0.5
EPS_ARG = 4 * 2.0 ** -24
U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -20}
# c per dtype, calibrated on the MI355X (tests/test_attention_gpu.py prints the observed maxima of err / (u mag)):
# bf16 1.77 (ctx, peaked scores; 1.5 for the CPU emulation of its roundings in tests/test_attn_bound_cpu.py), fp32 1.6 (ctx,
# rising scores)
C = {torch.bfloat16: 3.0, torch.float32: 3.0}
FLOOR = 1e-30
LSE_TOL = 2e-6                          # |lse - ref| <= LSE_TOL * (1 + |ref|) on valid rows (observed: 7.4e-7 fp32, 2.5e-7 bf16)


def _lens_list(lens, B, S):
    if lens is None:
        return [S] * B
    return [min(max(int(x), 0), S) for x in lens.tolist()]


def reference(qkv, lens, B, S, H, dctx=None, dtype=None):
    """fp64 reference on qkv's device, one sequence at a time (production sizes fit).  qkv: [B*S][3*H*128] (the same
    bf16 / fp32 values the kernel reads); dctx: [B*S][H*128] or None.  Returns a dict of tensors in the kernels' layouts:
    ctx, ctx_mag [B*S][H*128]; lse [B][H][S]; dqkv, dqkv_mag [B*S][3*H*128] (if dctx); rows >= len are 0 everywhere;
    valid [B*S] bool (row < len)."""
    dtype = dtype or qkv.dtype
    u = U[dtype]
    dev = qkv.device
    f64 = torch.float64
    x = qkv.to(f64).view(B, S, 3, H, DK)
    g = dctx.to(f64).view(B, S, H, DK) if dctx is not None else None
    L = _lens_list(lens, B, S)
    ctx = torch.zeros(B, S, H, DK, dtype=f64, device=dev)
    ctx_mag = torch.zeros_like(ctx)
    lse = torch.zeros(B, H, S, dtype=f64, device=dev)
    if g is not None:
        dqkv = torch.zeros(B, S, 3, H, DK, dtype=f64, device=dev)
        dqkv_mag = torch.zeros_like(dqkv)
    for b, n in enumerate(L):
        if n == 0:
            continue
        q, k, v = (x[b, :n, i].transpose(0, 1) for i in range(3))              # [H][n][128]
        s = (q @ k.transpose(1, 2)) * SCALE
        ls = torch.logsumexp(s, -1)
        p = torch.exp(s - ls.unsqueeze(-1))
        sabs = (q.abs() @ k.abs().transpose(1, 2)) * SCALE
        w = p * (1.0 + (sabs + ls.abs().unsqueeze(-1)) * (EPS_ARG / u))
        o = p @ v
        ctx[b, :n] = o.transpose(0, 1)
        ctx_mag[b, :n] = (w @ v.abs()).transpose(0, 1)
        lse[b, :, :n] = ls
        if g is None:
            continue
        do = g[b, :n].transpose(0, 1)
        dp = do @ v.transpose(1, 2)
        delta = (do * o).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        dqkv[b, :n, 0] = (SCALE * (ds @ k)).transpose(0, 1)
        dqkv[b, :n, 1] = (SCALE * (ds.transpose(1, 2) @ q)).transpose(0, 1)
        dqkv[b, :n, 2] = (p.transpose(1, 2) @ do).transpose(0, 1)
        m = w * (do.abs() @ v.abs().transpose(1, 2) + (do * o).abs().sum(-1, keepdim=True))
        dqkv_mag[b, :n, 0] = (SCALE * (m @ k.abs())).transpose(0, 1)
        dqkv_mag[b, :n, 1] = (SCALE * (m.transpose(1, 2) @ q.abs())).transpose(0, 1)
        dqkv_mag[b, :n, 2] = (w.transpose(1, 2) @ do.abs()).transpose(0, 1)
    valid = (torch.arange(S, device=dev).unsqueeze(0) < torch.tensor(L, device=dev).unsqueeze(1)).reshape(-1)
    out = dict(ctx=ctx.view(B * S, H * DK), ctx_mag=ctx_mag.view(B * S, H * DK), lse=lse, valid=valid, lens=L)
    if g is not None:
        out["dqkv"] = dqkv.view(B * S, 3 * H * DK)
        out["dqkv_mag"] = dqkv_mag.view(B * S, 3 * H * DK)
    return out


def bound_ratio(got, ref, mag, dtype, c=None, what=""):
    """Assert |got - ref| <= c u mag + FLOOR elementwise (NaN fails); return max err / (u mag) over elements above FLOOR."""
    u = U[dtype]
    c = C[dtype] if c is None else c
    err = (got.to(torch.float64) - ref).abs()
    bad = ~(err <= c * u * mag + FLOOR)
    ratio = torch.where(err <= FLOOR, torch.zeros_like(err), err / (u * mag))
    worst = ratio.nan_to_num(nan=math.inf).max().item() if ratio.numel() else 0.0
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside |err| <= {c} u mag + {FLOOR:g} "
                             f"(max err/(u mag) {worst:.3g}; first at flat index {i}: got {got.reshape(-1)[i].item():.6g}, "
                             f"ref {ref.reshape(-1)[i].item():.6g}, mag {mag.reshape(-1)[i].item():.3g})")
    return worst


def check_lse(lse, ref, what=""):
    """lse finite everywhere; on valid rows |lse - ref| <= LSE_TOL (1 + |ref|).  Returns max |lse - ref| / (1 + |ref|)."""
    assert torch.isfinite(lse).all(), f"{what}: non-finite lse"
    B, H, S = lse.shape
    v = (torch.arange(S, device=lse.device).unsqueeze(0) < torch.tensor(ref["lens"], device=lse.device).unsqueeze(1))
    v = v.unsqueeze(1).expand(B, H, S)
    r = ref["lse"][v]
    rel = (lse.to(torch.float64)[v] - r).abs() / (1.0 + r.abs())
    worst = rel.max().item() if rel.numel() else 0.0
    assert worst <= LSE_TOL, f"{what}: lse off by {worst:.3g} (1 + |lse|) > {LSE_TOL}"
    return worst


def check_all(ref, ctx, lse, dqkv, dtype, H, what=""):
    """Every bound of one forward + backward; returns {quantity: max err / (u mag)} (lse: max |dlse| / (1 + |lse|))."""
    v = ref["valid"]
    r = {"ctx": bound_ratio(ctx[v], ref["ctx"][v], ref["ctx_mag"][v], dtype, what=f"{what} ctx"),
         "lse": check_lse(lse, ref, what)}
    if dqkv is not None:
        assert torch.isfinite(dqkv.float()).all(), f"{what}: non-finite dqkv"
        assert not dqkv[~v].any(), f"{what}: dqkv rows >= len are not exactly 0"
        for i, name in enumerate(("dq", "dk", "dv")):
            sl = slice(i * H * DK, (i + 1) * H * DK)
            r[name] = bound_ratio(dqkv[v][:, sl], ref["dqkv"][v][:, sl], ref["dqkv_mag"][v][:, sl], dtype, what=f"{what} {name}")
    return r


# ---------------------------------------------------------------------------------------------------------------- inputs
PAD_LEAK_SCORE = 17.0        # a padded key's score: ~10-20 above every valid key (valid scores are ~N(0, 1.1))
PAD_OVERFLOW_SCORE = 120.0   # > 128 log2 units (88.7) above any valid query's lse: exp overflows fp32
_A_PAD = 4.0                 # every query's component along the padding direction (d = 1 of each head)
_A_RISE = 8.0                # |query component| along the rising direction (d = 0 of each head)
RISE_RANGE = 130.0           # score span (natural log) over a sequence's keys for a query with t = +-1


def make_inputs(B, S, H, lens, dtype, device, seed, regime="randn", pad="randn"):
    """(qkv, dctx) as the kernels read them.  regime: 'randn' | 'flat' (q x 0.05) | 'peaked' (q x 4) | 'rising' (keys carry
    a component that grows linearly with the key index, queries a mixed-sign multiple of it: scores span RISE_RANGE, so
    rising queries find a new maximum > 8 log2 units up in every 64-key tile and outgrow their first tile's maximum by more
    than 128 log2 units, falling queries underflow to exact zeros).  pad: 'randn' | 'leak' | 'overflow' - what rows
    [len, S) of K and V hold: plain randn, or K aligned with every query (score PAD_LEAK_SCORE / PAD_OVERFLOW_SCORE) and
    V ~ 1e2.  dctx rows >= len are 0."""
    gen = torch.Generator().manual_seed(seed)
    L = _lens_list(lens, B, S)
    x = torch.randn(B, S, 3, H, DK, generator=gen, dtype=torch.float64)
    if regime == "flat":
        x[:, :, 0] *= 0.05
    elif regime == "peaked":
        x[:, :, 0] *= 4.0
    elif regime == "rising":
        t = (torch.rand(B, S, H, generator=gen, dtype=torch.float64) * 2.4 - 1.2).clamp(-1.0, 1.0)
        x[:, :, 0, :, 0] = _A_RISE * t
        for b, n in enumerate(L):
            if n:
                slope = RISE_RANGE / (_A_RISE * SCALE * max(n - 1, 1))
                x[b, :n, 1, :, 0] = (slope * (torch.arange(n, dtype=torch.float64) - (n - 1) / 2)).unsqueeze(1)
    elif regime != "randn":
        raise ValueError(regime)
    if pad != "randn":
        beta = (PAD_LEAK_SCORE if pad == "leak" else PAD_OVERFLOW_SCORE) / (_A_PAD * SCALE)
        x[:, :, 0, :, 1] = _A_PAD
        for b, n in enumerate(L):
            if n < S:
                x[b, n:, 1] *= 0.1
                x[b, n:, 1, :, 1] = beta
                x[b, n:, 2] += 100.0
    dctx = torch.randn(B, S, H * DK, generator=gen, dtype=torch.float64)
    for b, n in enumerate(L):
        dctx[b, n:] = 0
    return (x.view(B * S, 3 * H * DK).to(dtype).to(device), dctx.view(B * S, H * DK).to(dtype).to(device))
