"""The dropout generator restated in integers, and fp64 references with per-element bounds for LayerNorm forward / backward
(fs2_norm.hip, fs2_common.h).  Conventions of tests/elem_ref.py: a result that is ONE rounded fp32 operation is bit-exact, a
reduction is held to c * u * mag with c counted from the kernel's chain of dependent roundings, never fitted.

The mask.  keep(seed, idx, p) = (u >= p), u = (h >> 8) 2^-24, h = hash32(hash32(idx ^ lo(seed)) + hi(seed) + 0x9e3779b9), all in
int64 tensors masked to 32 bits; u is exact in fp32 and p is the fp32 value the kernel receives.  idx = (row C + c) mod 2^32,
seed = (seed + seed_dev offset) mod 2^64.  hash32 is a bijection, so `seed_with_tie` builds a seed for which a chosen element
draws u == 0.5 exactly: with p = 0.5 that element tells `>=` from `>`.

LayerNorm forward (chain = additions onto one row sum: 4 NV + 6 shuffle stages in ln_fwd_kernel<T, NV>, 8 + 5 in the bf16
C = 256 kernel):
  z     one multiply (dropout) or one add (residual) alone is bit-exact; both together c = 2 (they may fuse), + the bf16 store
  mean  of the STORED z: c = chain + 1 (the division) on mean_c |z|
  rstd  about the kernel's own saved mean (what a two-pass variance is): each (z - mean)^2 carries 3 u, the sum chain + 1, and the
        eps addition 1 u of var + eps:  |rstd - ref| <= ref (0.5 ((chain + 4) var / (var + eps) + 1) u + 4 u), 4 u for the
        hardware reciprocal square root (as test_batchnorm_persistent_workspace)
  out   from the kernel's own saved mean and rstd (each held to its bound above, so the composed bound is the sum of the two):
        subtraction, two products, the add of beta, the dropout product: c = 5 on (|xhat gamma| + |beta|) / (1 - p_post)
LayerNorm backward, from the saved mean / rstd, n_g = roundings in g (dout + dout2: 1, dropout: 1):
  dz    s2 = mean_c(g gamma xhat): the products n_g + 4, the sum chain + 1, times xhat 3 more; two subtractions and the product
        with rstd: c = n_g + chain + 11 on rstd (|g gamma| + mean_c |g gamma| + |xhat| mean_c |g gamma xhat|)
  d1    + 1 for d1_add (its magnitude added);  d2  + 1 for the dropout product;  both + the bf16 store
  dgamma / dbeta   any association of `rows` terms onto the initial contents, plus the rounded factors:
        c = rows + n_g + 3 / rows + n_g  (as test_layernorm_deferred_reduce)

Observed maxima of err / (u mag) on the MI355X (tests/test_norm_gpu.py prints them; nothing above is fitted to them):
fp32 / bf16 (bf16: beyond its own output rounding; rstd: err / limit).
  forward   z (dropout and residual, c = 2) 1.84 / 0.40, one operation alone bit-exact; mean 1.54 / 1.05 (c = 11 .. 39 / 14);
            rstd 0.20 / 0.20; out 3.11 / 0 (c = 5); the misaligned bf16 fallback: mean 0.34, rstd 0.11
  backward  3 x 7 rows, eleven forms: d1 2.81 / 0.08, d2 2.69 / 0.08 (c = 21 .. 52), dgamma 3.04 / 2.99, dbeta 2.47 / 1.98 (c = 21 .. 26)
            row loops (8200 .. 32769 rows): d1 2.49 / 0.63, d2 2.39 / 0.13, dgamma 0.17 / 0.12, dbeta 0.14 / 0.06
  masks     every site equals the restated mask in every element; gemm_res_ln z 0 beyond the bf16 rounding (c = 2);
            BatchNorm backward with the restated mask: dgamma 1.30 / 1.19, dbeta 0.75 / 0.62, dx 2.41 / 0
  BatchNorm at 1, 2, 5 rows (fp32): mean 1.31, out 1.95, running_var 0.75, dgamma 1.59, dbeta 1.02, dx 1.25
"""
import types

import torch

from tests import elem_ref as R
from tests.elem_ref import F64, U32, allowed, bits, check, store  # noqa: F401  (re-exported for the tests)

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B9
MUL1, MUL2 = 0x7FEB352D, 0x846CA68B


def f32(v):
    """the fp32 value a C float argument receives"""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ the mask
def hash32(x):
    """fs2_hash32 on an int64 tensor holding 32-bit values (the int64 products wrap; their low 32 bits are the uint32 product)"""
    x = x ^ (x >> 16)
    x = (x * MUL1) & M32
    x = x ^ (x >> 15)
    x = (x * MUL2) & M32
    return x ^ (x >> 16)


def uniform24(seed, idx):
    """u 2^24 = h >> 8 of fs2_uniform, for a 64-bit seed (Python int) and an int64 tensor of 32-bit element indices"""
    seed &= M64
    h = hash32((idx & M32) ^ (seed & M32))
    h = hash32((h + (seed >> 32) + GOLDEN) & M32)
    return h >> 8


def keep(seed, idx, p, strict=False):
    """the keep decision u >= p of fs2_drop_scale (strict=True: the wrong `>`, for the tests of the tests)"""
    u = uniform24(seed, idx).to(F64) * 2.0 ** -24
    return u > f32(p) if strict else u >= f32(p)


def drop_scale(p):
    """the fp32 value 1.f / (1.f - p) the kernels multiply kept elements by (1 when p <= 0)"""
    if p <= 0:
        return 1.0
    one = torch.tensor(1.0, dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


def keep_rows(seed, rows, C, p, offset=0, index_C=None, shift=0, strict=False):
    """the [rows, C] keep tensor of a site: seed + offset is a 64-bit add (a carry goes into the high half), the element index is
    (row C + c) mod 2^32.  index_C / shift / strict restate the faults the CPU tests must see rejected."""
    if p <= 0:
        return torch.ones(rows, C, dtype=torch.bool)
    r = torch.arange(rows, dtype=torch.int64).unsqueeze(1)
    c = torch.arange(C, dtype=torch.int64).unsqueeze(0)
    idx = (r * (index_C or C) + c + shift) & M32
    return keep((seed + offset) & M64, idx, p, strict)


def _unhash32(h):
    h ^= h >> 16
    h = (h * pow(MUL2, -1, 1 << 32)) & M32
    h ^= (h >> 15) ^ (h >> 30)
    h = (h * pow(MUL1, -1, 1 << 32)) & M32
    return h ^ (h >> 16)


def seed_with_tie(hi, idx, offset=0, u24=1 << 23):
    """the seed s for which s + offset has high half `hi` and element `idx` draws exactly u = u24 2^-24 (default 0.5)"""
    h1 = (_unhash32((u24 << 8) & M32) - hi - GOLDEN) & M32
    lo = _unhash32(h1) ^ (idx & M32)
    return (((hi & M32) << 32 | lo) - offset) & M64


def carrying_offset(seed_eff):
    """an offset k < 2^63 such that (seed_eff - k) + k carries out of the low half (whatever seed_eff's low half below 2^32 - 1)"""
    assert seed_eff & M32 != M32
    return (3 << 32) | M32


def site_seed(p, hi, tie_idx, offset=0):
    """the seed a test hands a site: at p = 0.5 one whose element tie_idx sits exactly on u == p"""
    if p == 0.5:
        return seed_with_tie(hi, tie_idx, offset)
    return (((hi & M32) << 32 | ((0xFFFFFF00 ^ tie_idx) & M32)) - offset) & M64


# ----------------------------------------------------------------------------------------------------------------- the cases
def ln_chain(dtype, C, aligned=True):
    """additions onto one row sum: ln_*_c256_bf16_kernel 8 per lane + 5 stages; ln_*_kernel<T, NV> 4 NV per lane + 6 stages"""
    if dtype == torch.bfloat16 and C == 256 and aligned:
        return 8 + 5
    nv = 1 if C <= 256 else (2 if C <= 512 else (4 if C <= 1024 else 8))
    return 4 * nv + 6


def lens_for(B, S):
    """lengths that contain S and 0 (from B = 2 on), then a boundary inside the sequence"""
    pat = [S, 0, (S + 1) // 2, max(S - 1, 0)]
    return torch.tensor([pat[b % 4] for b in range(B)], dtype=torch.int32)


FAMILIES = ("randn", "const", "bigmean", "tiny", "huge", "outlier")


def family_rows(family, rows, C, g):
    x = torch.randn(rows, C, generator=g)
    if family == "randn":
        return x * 1.5 + 0.3
    if family == "const":                                   # every row one value
        return (1.5 + 0.25 * torch.arange(rows, dtype=torch.float32)).unsqueeze(1).expand(rows, C).contiguous()
    if family == "bigmean":                                 # the mean far above the spread: a one-pass variance cancels
        return 1000.0 + 0.01 * x
    if family == "tiny":                                    # variance far below eps
        return 1e-6 * x
    if family == "huge":
        return 1e15 * x
    if family == "outlier":
        x[rows // 2, C // 3] = 1e4
        return x
    raise ValueError(family)


def fwd_case(dtype, B, S, C, family="randn", res=True, lens=True, p_pre=0.0, p_post=0.0, offset=0, aligned=True, gamma_one=False,
             beta_fill=None):
    g = torch.Generator().manual_seed(1000 * C + 10 * B * S + S + FAMILIES.index(family))
    rows = B * S
    y = family_rows(family, rows, C, g).to(dtype)
    y = torch.where(y == 0, torch.ones_like(y), y)          # nowhere zero: a dropped element is recognisable
    k = types.SimpleNamespace(dtype=dtype, B=B, S=S, C=C, rows=rows, eps=1e-5, p_pre=p_pre, p_post=p_post, offset=offset,
                              aligned=aligned, family=family, y=y)
    k.res = (torch.randn(rows, C, generator=g) * 0.7).to(dtype) if res else None
    k.gamma = torch.ones(C) if gamma_one else torch.rand(C, generator=g) + 0.5
    k.beta = torch.full((C,), float(beta_fill)) if beta_fill is not None else torch.randn(C, generator=g) * 0.3
    k.lens = lens_for(B, S) if lens else None
    k.tie_pre, k.tie_post = (rows * C) // 3, C // 2 + 1    # (the post site's tie sits in row 0, never padded)
    k.seed_pre = site_seed(p_pre, 0x9E3779B1, k.tie_pre, offset)
    k.seed_post = site_seed(p_post, 0x85EBCA6B, k.tie_post, offset)
    return k


def pad_rows(k):
    return R.padding(k.lens, k.B, k.S).reshape(-1)


# ---------------------------------------------------------------------------------------------------------- LayerNorm forward
def ln_fwd_z(k, **fault):
    """z = keep_pre y / (1 - p_pre) + res in fp64 -> (z, mag, c, fp32 image when z is one rounded operation else None, keep)"""
    kp = keep_rows(k.seed_pre, k.rows, k.C, k.p_pre, k.offset, **fault)
    sc = kp.to(torch.float32) * torch.tensor(drop_scale(k.p_pre), dtype=torch.float32)
    z = k.y.to(F64) * sc.to(F64)
    mag, c = z.abs(), int(k.p_pre > 0)
    one = k.y.float() * sc if k.p_pre > 0 else k.y.float()
    if k.res is not None:
        z, mag, c = z + k.res.to(F64), mag + k.res.to(F64).abs(), c + 1
        one = one + k.res.float()
    return z, mag, c, (store(one, k.dtype) if c <= 1 else None), kp


def ln_stats(k, z, mean_k):
    """fp64 statistics of the stored z -> (mean, mean magnitude, c), (rstd about the kernel's saved mean, its absolute limit)"""
    z64 = z.to(F64)
    chain = getattr(k, "chain", None) or ln_chain(k.dtype, k.C, k.aligned)
    d = z64 - mean_k.to(F64).unsqueeze(1)
    var, eps = (d * d).mean(1), f32(k.eps)
    rs = (var + eps).rsqrt()
    lim = rs * (0.5 * ((chain + 4) * var / (var + eps) + 1) * U32 + 4 * U32)
    return (z64.mean(1), z64.abs().mean(1), chain + 1), (rs, lim)


def ln_out(k, z, mean_k, rstd_k, **fault):
    """out = (xhat gamma + beta) keep_post / (1 - p_post), 0 on padded rows, from the saved statistics -> (out, mag, c, keep)"""
    xh = (z.to(F64) - mean_k.to(F64).unsqueeze(1)) * rstd_k.to(F64).unsqueeze(1)
    t = xh * k.gamma.to(F64)
    kq = keep_rows(k.seed_post, k.rows, k.C, k.p_post, k.offset, **fault)
    sc = kq.to(F64) * drop_scale(k.p_post)
    o, mag = (t + k.beta.to(F64)) * sc, (t.abs() + k.beta.to(F64).abs()) * sc
    pad = pad_rows(k).unsqueeze(1)
    zero = torch.zeros((), dtype=F64)
    return torch.where(pad, zero, o), torch.where(pad, zero, mag), 4 + int(k.p_post > 0), kq


def verify_fwd(k, z, mean, rstd, out):
    """every check of the forward on CPU tensors as the kernel left them; AssertionError names the first element out of bound.
    Returns the largest err / (u mag) per output (rstd: err / limit)."""
    z, mean, rstd, out = z.cpu(), mean.cpu(), rstd.cpu(), out.cpu()
    rep = {}
    zr, zm, zc, zone, _ = ln_fwd_z(k)
    if zone is not None:
        n = int((bits(z) != bits(zone)).sum())
        assert n == 0, f"z: {n} of {z.numel()} elements are not the one rounded operation"
        rep["z"] = 0.0
    else:
        rep["z"] = check(z, zr, zm, zc, k.dtype, what="z")
    assert bool(torch.isfinite(mean).all() and torch.isfinite(rstd).all()), "mean / rstd not written on every row"
    (mr, mm, mc), (rs, rs_lim) = ln_stats(k, z, mean)
    rep["mean"] = check(mean, mr, mm, mc, what="mean")
    err = (rstd.to(F64) - rs).abs()
    bad = ~(err <= rs_lim)
    assert not bool(bad.any()), (f"rstd: {int(bad.sum())} rows out of bound; first #{int(bad.nonzero()[0])}: got "
                                 f"{float(rstd[bad][0]):.9g} ref {float(rs[bad][0]):.9g} lim {float(rs_lim[bad][0]):.3g}")
    rep["rstd"] = float((err / rs_lim).max())
    orf, om, oc, _ = ln_out(k, z, mean, rstd)
    rep["out"] = check(out, orf, om, oc, k.dtype, what="out")
    pad = pad_rows(k)
    assert int((bits(out)[pad] != 0).sum()) == 0, "padded rows of out are not exactly zero"
    return rep


# --------------------------------------------------------------------------------------------------------- LayerNorm backward
FORMS = ("plain", "d1_add", "d1_only", "d2_only", "d1_add_no_d1", "dout2", "relu_bwd", "p_pre", "p_post", "all", "deferred")


def bwd_case(dtype, B, S, C, form="plain", lens=True, aligned=True):
    """inputs of fs2_ln_bwd_sum for one option form.  z, mean and rstd are what a forward could have written: finite on every row
    (the contract); dout and dout2 hold NaN on padded rows, which must reach no output."""
    assert form in FORMS
    g = torch.Generator().manual_seed(77 * C + 10 * B * S + S + FORMS.index(form))
    rows = B * S
    every = form in ("all", "deferred")
    k = types.SimpleNamespace(dtype=dtype, B=B, S=S, C=C, rows=rows, eps=1e-5, aligned=aligned, form=form)
    k.want_d1 = form not in ("d2_only", "d1_add_no_d1")
    k.want_d2 = form != "d1_only"
    k.relu_bwd = every or form == "relu_bwd"
    k.p_pre = 0.5 if every or form == "p_pre" else 0.0
    k.p_post = 0.5 if form == "p_post" else (0.1 if every else 0.0)
    k.defer = form == "deferred"
    k.offset = carrying_offset(0x1234ABCD) if every else 0
    z = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    k.lens = lens_for(B, S) if lens else None
    k.tie_pre = k.tie_post = C // 2 + 1                     # row 0, never padded
    z = z.to(dtype)
    if rows * C >= 64:
        z.view(-1)[7::61] = 0.0                             # exact +0 and -0: neither passes the ReLU gate
        z.view(-1)[11::67] = -0.0
    z.view(-1)[k.tie_pre] = 0.75                            # (positive: the ReLU gate must not hide the tie)
    k.z = z
    zf = z.float()
    k.mean = zf.mean(1)
    k.rstd = ((zf - k.mean.unsqueeze(1)) ** 2).mean(1).add(1e-5).rsqrt()
    pad = pad_rows(k).unsqueeze(1)
    nan = torch.full((), float("nan"))
    k.dout = torch.where(pad, nan, torch.randn(rows, C, generator=g)).to(dtype)
    k.dout2 = torch.where(pad, nan, torch.randn(rows, C, generator=g)).to(dtype) if every or form == "dout2" else None
    k.d1_add = torch.randn(rows, C, generator=g).to(dtype) if every or form in ("d1_add", "d1_add_no_d1") else None
    k.gamma = torch.rand(C, generator=g) + 0.5
    k.dgamma0 = torch.randn(C, generator=g) if every else torch.zeros(C)
    k.dbeta0 = torch.randn(C, generator=g) if every else torch.zeros(C)
    k.seed_pre = site_seed(k.p_pre, 0x9E3779B1, k.tie_pre, k.offset)
    k.seed_post = site_seed(k.p_post, 0x85EBCA6B, k.tie_post, k.offset)
    return k


def ln_bwd_ref(k, pre_fault=None, post_fault=None):
    """fp64 backward from the saved mean / rstd -> {name: (ref, mag, c)} for d1, d2, dgamma, dbeta"""
    zero = torch.zeros((), dtype=F64)
    chain = getattr(k, "chain", None) or ln_chain(k.dtype, k.C, k.aligned)
    pad = pad_rows(k).unsqueeze(1)
    kq = keep_rows(k.seed_post, k.rows, k.C, k.p_post, k.offset, **(post_fault or {}))
    kp = keep_rows(k.seed_pre, k.rows, k.C, k.p_pre, k.offset, **(pre_fault or {}))
    g = k.dout.to(F64) + (k.dout2.to(F64) if k.dout2 is not None else 0.0)
    g = torch.where(pad, zero, g * (kq.to(F64) * drop_scale(k.p_post)))         # (select: padded rows may hold NaN)
    n_g = int(k.dout2 is not None) + int(k.p_post > 0)
    z64, rs = k.z.to(F64), k.rstd.to(F64).unsqueeze(1)
    xh = (z64 - k.mean.to(F64).unsqueeze(1)) * rs
    gg = g * k.gamma.to(F64)
    s1, s1m = gg.mean(1, keepdim=True), gg.abs().mean(1, keepdim=True)
    s2, s2m = (gg * xh).mean(1, keepdim=True), (gg * xh).abs().mean(1, keepdim=True)
    dz = rs * (gg - s1 - xh * s2)
    dz_m = rs * (gg.abs() + s1m + xh.abs() * s2m)
    c_dz = n_g + chain + 11
    out = {}
    add = k.d1_add.to(F64) if k.d1_add is not None else None
    out["d1"] = (dz + add, dz_m + add.abs(), c_dz + 1) if add is not None else (dz, dz_m, c_dz)
    sc = kp.to(F64) * drop_scale(k.p_pre)
    if k.relu_bwd:
        sc = torch.where(z64 > 0, sc, zero)
    out["d2"] = (dz * sc, dz_m * sc, c_dz + int(k.p_pre > 0))
    dg0, db0 = k.dgamma0.to(F64), k.dbeta0.to(F64)
    out["dgamma"] = (dg0 + (g * xh).sum(0), dg0.abs() + (g * xh).abs().sum(0), k.rows + n_g + 3)
    out["dbeta"] = (db0 + g.sum(0), db0.abs() + g.abs().sum(0), k.rows + n_g)
    return out


def verify_bwd(k, d1, d2, dgamma, dbeta):
    """every check of the backward; d1 / d2 are None where the form does not ask for them"""
    ref = ln_bwd_ref(k)
    pad = pad_rows(k)
    rep = {}
    for name, got, dt_ in (("d1", d1, k.dtype), ("d2", d2, k.dtype), ("dgamma", dgamma, torch.float32), ("dbeta", dbeta, torch.float32)):
        if got is None:
            continue
        got = got.cpu()
        assert not bool(torch.isnan(got.float()).any()), f"{name}: NaN reached the output"
        r, m, c = ref[name]
        rep[name] = check(got, r, m, c, dt_, what=name)
    if d1 is not None:
        want = k.d1_add if k.d1_add is not None else torch.zeros_like(k.z)
        n = int((bits(d1.cpu())[pad] != bits(want)[pad]).sum())
        assert n == 0, f"d1: {n} elements of padded rows differ from d1_add"
    if d2 is not None:
        assert bool((d2.cpu()[pad] == 0).all()), "d2 is not zero on padded rows"
    return rep
