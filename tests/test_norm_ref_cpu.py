"""tests/norm_ref.py checked without a GPU: the restated dropout generator reproduces known answers of the C functions, the fp64
LayerNorm references agree with torch, every bound accepts fp32 emulations of the kernels in two other associations, and every
check rejects a list of single-place faults at the inputs tests/test_norm_gpu.py uses."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as N
from tests.norm_ref import F64

BF16, F32 = torch.bfloat16, torch.float32

# (seed, idx, u 2^24) printed by fs2_hash32 / fs2_uniform of fs2_common.h compiled as host C++.  Seeds with a non-zero high half,
# idx 0 and 2^32 - 1, and 0x1fffffff0 + 0x20 (the low half carries) are among them.
KNOWN = [
    (0x0000000000000000, 0x00000000, 130277),
    (0x0000000000000000, 0x00000001, 11672718),
    (0x0000000000000000, 0x000000ff, 481225),
    (0x0000000000000000, 0x00000100, 7277467),
    (0x0000000000000000, 0x00010001, 6483847),
    (0x0000000000000000, 0x80000000, 7924594),
    (0x0000000000000000, 0xffffffff, 10357028),
    (0x0000000000000001, 0x00000000, 11672718),
    (0x0000000000000001, 0x00000001, 130277),
    (0x0000000000000001, 0x000000ff, 11067399),
    (0x0000000000000001, 0x00000100, 12051725),
    (0x0000000000000001, 0x00010001, 7717735),
    (0x0000000000000001, 0x80000000, 8940709),
    (0x0000000000000001, 0xffffffff, 12698665),
    (0x0000000001234567, 0x00000000, 2785425),
    (0x0000000001234567, 0x00000001, 12420334),
    (0x0000000001234567, 0x000000ff, 14899205),
    (0x0000000001234567, 0x00000100, 11915120),
    (0x0000000001234567, 0x00010001, 1748851),
    (0x0000000001234567, 0x80000000, 14545840),
    (0x0000000001234567, 0xffffffff, 5763157),
    (0x00000000ffffffff, 0x00000000, 10357028),
    (0x00000000ffffffff, 0x00000001, 12698665),
    (0x00000000ffffffff, 0x000000ff, 13871690),
    (0x00000000ffffffff, 0x00000100, 14748411),
    (0x00000000ffffffff, 0x00010001, 2911015),
    (0x00000000ffffffff, 0x80000000, 14950632),
    (0x00000000ffffffff, 0xffffffff, 130277),
    (0x0000000100000000, 0x00000000, 10440790),
    (0x0000000100000000, 0x00000001, 3031039),
    (0x0000000100000000, 0x000000ff, 11722141),
    (0x0000000100000000, 0x00000100, 12105996),
    (0x0000000100000000, 0x00010001, 11597435),
    (0x0000000100000000, 0x80000000, 10675194),
    (0x0000000100000000, 0xffffffff, 13804882),
    (0xdeadbeef00000000, 0x00000000, 4136681),
    (0xdeadbeef00000000, 0x00000001, 8797636),
    (0xdeadbeef00000000, 0x000000ff, 16468420),
    (0xdeadbeef00000000, 0x00000100, 4800176),
    (0xdeadbeef00000000, 0x00010001, 12813945),
    (0xdeadbeef00000000, 0x80000000, 9383989),
    (0xdeadbeef00000000, 0xffffffff, 6529853),
    (0x9e3779b97f4a7c15, 0x00000000, 3898698),
    (0x9e3779b97f4a7c15, 0x00000001, 2650486),
    (0x9e3779b97f4a7c15, 0x000000ff, 2788525),
    (0x9e3779b97f4a7c15, 0x00000100, 12605246),
    (0x9e3779b97f4a7c15, 0x00010001, 15935391),
    (0x9e3779b97f4a7c15, 0x80000000, 12331559),
    (0x9e3779b97f4a7c15, 0xffffffff, 3753599),
    (0xffffffffffffffff, 0x00000000, 1588930),
    (0xffffffffffffffff, 0x00000001, 962042),
    (0xffffffffffffffff, 0x000000ff, 13629484),
    (0xffffffffffffffff, 0x00000100, 13923241),
    (0xffffffffffffffff, 0x00010001, 4959576),
    (0xffffffffffffffff, 0x80000000, 2643411),
    (0xffffffffffffffff, 0xffffffff, 10811273),
    (0x0000000200000010, 0x00000000, 11681172),
    (0x0000000200000010, 0x00000001, 4789261),
    (0x0000000200000010, 0x000000ff, 4983643),
    (0x0000000200000010, 0x00000100, 11365930),
    (0x0000000200000010, 0x00010001, 1305776),
    (0x0000000200000010, 0x80000000, 7386156),
    (0x0000000200000010, 0xffffffff, 12291800),
    (0x8000000000000004, 0x00000000, 8899074),
    (0x8000000000000004, 0x00000001, 12322568),
    (0x8000000000000004, 0x000000ff, 10951906),
    (0x8000000000000004, 0x00000100, 10018822),
    (0x8000000000000004, 0x00010001, 6155054),
    (0x8000000000000004, 0x80000000, 8512313),
    (0x8000000000000004, 0xffffffff, 5225367),
]


# ------------------------------------------------------------------------------------------------------------------ the mask
def test_generator_known_answers():
    assert len(KNOWN) >= 64
    for seed, idx, u24 in KNOWN:
        assert int(N.uniform24(seed, torch.tensor([idx]))[0]) == u24, (hex(seed), hex(idx))
    idx = torch.tensor([r[1] for r in KNOWN[:7]])
    assert N.uniform24(KNOWN[0][0], idx).tolist() == [r[2] for r in KNOWN[:7]]          # vectorised == one by one
    # the offset is a 64-bit add: 0x1fffffff0 + 0x20 = 0x200000010 (a carry into the high half), then mod 2^64
    k = N.keep_rows(0x1FFFFFFF0, 2, 8, 0.5, offset=0x20)
    assert torch.equal(k, N.keep_rows(0x200000010, 2, 8, 0.5))
    assert torch.equal(N.keep_rows(N.M64, 2, 8, 0.5, offset=1), N.keep_rows(0, 2, 8, 0.5))
    # the element index is (row C + c) mod 2^32
    assert bool(N.keep(5, torch.tensor([(1 << 32) + 3]), 0.5) == N.keep(5, torch.tensor([3]), 0.5))


def test_keep_sits_on_the_right_side_of_a_tie():
    for hi, idx, off in ((0, 0, 0), (0xDEADBEEF, 12345, 0), (7, N.M32, 99), (0x9E3779B1, 1793, N.carrying_offset(0x55))):
        s = N.seed_with_tie(hi, idx, off)
        eff = (s + off) & N.M64
        assert eff >> 32 == hi and int(N.uniform24(eff, torch.tensor([idx]))[0]) == 1 << 23          # u == 0.5 exactly
        assert bool(N.keep(eff, torch.tensor([idx]), 0.5)) and not bool(N.keep(eff, torch.tensor([idx]), 0.5, strict=True))
    s = N.seed_with_tie(3, 40, u24=1)                                                                # u = 2^-24 > 0: kept at p -> 0+
    assert bool(N.keep(s, torch.tensor([40]), 2.0 ** -24)) and not bool(N.keep(s, torch.tensor([40]), 2.0 ** -23))
    off = N.carrying_offset(0x1234ABCD)
    assert ((0x1234ABCD - off) & N.M32) + (off & N.M32) > N.M32 and off < 1 << 63


def test_streams_differ():
    a = N.keep_rows(0x1234567800000011, 16, 256, 0.5)
    assert 0.4 < a.float().mean() < 0.6
    for other in (0x1234567800000012, 0x1234567900000011, 0x0000001100000000 | 0x12345678, 0x11):
        b = N.keep_rows(other, 16, 256, 0.5)
        assert 0.4 < (a ^ b).float().mean() < 0.6, hex(other)          # independent streams, not a shifted or equal one
    assert 0.05 < (~N.keep_rows(9 << 32, 64, 256, 0.1)).float().mean() < 0.15
    assert abs(N.drop_scale(0.1) - 1 / 0.9) < 1e-7 and N.drop_scale(0.5) == 2.0 and N.drop_scale(0.0) == 1.0


# ------------------------------------------------------------------------------------------------------ agreement with torch
@pytest.mark.parametrize("C", [4, 260, 1024])
def test_forward_reference_agrees_with_torch(C):
    k = N.fwd_case(F32, 3, 7, C, p_pre=0.5, p_post=0.1)
    z, _, c, _, kp = N.ln_fwd_z(k)
    assert c == 2
    zt = k.y.double() * kp.double() * 2.0 + k.res.double()
    assert torch.equal(z, zt)
    mean = z.mean(1)
    (mr, _, _), (rs, _) = N.ln_stats(k, z, mean)
    rstd = (z.var(1, unbiased=False) + N.f32(1e-5)).rsqrt()
    assert torch.allclose(rs, rstd, rtol=1e-12, atol=0) and torch.equal(mr, mean)
    out, _, _, kq = N.ln_out(k, z, mean, rstd)
    ref = F.layer_norm(z, (C,), k.gamma.double(), k.beta.double(), N.f32(1e-5)) * kq.double() * N.drop_scale(0.1)
    ref = ref * (~N.pad_rows(k)).double().unsqueeze(1)
    assert torch.allclose(out, ref, rtol=1e-11, atol=1e-12)
    assert bool((out[N.pad_rows(k)] == 0).all()) and int(N.pad_rows(k).sum()) == 7 + 3


@pytest.mark.parametrize("form", ["all", "relu_bwd", "plain"])
@pytest.mark.parametrize("C", [4, 260, 1024])
def test_backward_reference_agrees_with_autograd(C, form):
    k = N.bwd_case(F32, 3, 7, C, form)
    g = torch.Generator().manual_seed(C)
    kp = N.keep_rows(k.seed_pre, k.rows, C, k.p_pre, k.offset).double() * N.drop_scale(k.p_pre)
    kq = N.keep_rows(k.seed_post, k.rows, C, k.p_post, k.offset).double() * N.drop_scale(k.p_post)
    h = torch.randn(k.rows, C, generator=g, dtype=F64).requires_grad_(True)
    res = torch.randn(k.rows, C, generator=g, dtype=F64).requires_grad_(True)
    gamma, beta = k.gamma.double().requires_grad_(True), torch.zeros(C, dtype=F64, requires_grad=True)
    if form == "relu_bwd":
        z = torch.relu(h)                                   # the variance predictor: z IS the ReLU output, gated on z > 0
    else:
        k.relu_bwd = False
        z = h * kp + res
    out = F.layer_norm(z, (C,), gamma, beta, 1e-5) * kq
    live = ~N.pad_rows(k).unsqueeze(1)
    up = k.dout.double() + (k.dout2.double() if k.dout2 is not None else 0.0)
    up = torch.where(live, up, torch.zeros((), dtype=F64))
    (out * up).sum().backward()
    k.z = z.detach()
    k.mean = k.z.mean(1)
    k.rstd = (k.z.var(1, unbiased=False) + 1e-5).rsqrt()
    ref = N.ln_bwd_ref(k)
    add = k.d1_add.double() if k.d1_add is not None else 0.0
    tol = dict(rtol=1e-9, atol=1e-10)
    assert torch.allclose(ref["d2"][0], h.grad, **tol)
    if form != "relu_bwd":
        assert torch.allclose(ref["d1"][0], res.grad + add, **tol)
    assert torch.allclose(ref["dgamma"][0], gamma.grad + k.dgamma0.double(), **tol)
    assert torch.allclose(ref["dbeta"][0], beta.grad + k.dbeta0.double(), **tol)


# ---------------------------------------------------------------------------------------------------------- fp32 emulations
def _fsum(x, assoc):
    """row sums of an fp32 [rows, n] tensor: one sequential chain, or a pairwise tree (neither is the kernels' association)"""
    if assoc == "seq":
        acc = torch.zeros(x.shape[0], dtype=F32)
        for c in range(x.shape[1]):
            acc = acc + x[:, c]
        return acc
    n = 1
    while n < x.shape[1]:
        n *= 2
    x = torch.cat([x, torch.zeros(x.shape[0], n - x.shape[1], dtype=F32)], 1)
    while x.shape[1] > 1:
        x = x[:, : x.shape[1] // 2] + x[:, x.shape[1] // 2:]
    return x[:, 0]


def _mask_fault(mut, site):
    return {f"index256_{site}": dict(index_C=256), f"shift_{site}": dict(shift=1), f"strict_{site}": dict(strict=True)}.get(mut, {})


def _pad(k, mut):
    if k.lens is None:
        return torch.zeros(k.rows, dtype=torch.bool)
    t = torch.arange(k.S).unsqueeze(0)
    ln = k.lens.long().view(k.B, 1)
    return (t > ln if mut == "pad_gt" else t >= ln).reshape(-1)


def emu_fwd(k, assoc, mut=None):
    """ln_fwd in fp32 on the CPU with one fault (mut) or none -> z, mean, rstd, out as the kernel would leave them"""
    C = k.C
    z = k.y.float()
    if k.p_pre > 0:
        z = z * (N.keep_rows(k.seed_pre, k.rows, C, k.p_pre, k.offset, **_mask_fault(mut, "pre")).float() * N.drop_scale(k.p_pre))
    if k.res is not None:
        z = z + k.res.float()
    zs = N.store(z, k.dtype)
    x = z if mut == "unrounded" else zs.float()
    nm, nv = (C - 4 if mut == "mean4" else C), (C - 4 if mut == "var4" else C)
    div = float(C - 1) if mut == "c_minus_1" else None
    mean = _fsum(x[:, :nm], assoc) / (div or float(nm))
    if mut == "one_pass":
        var = _fsum(x * x, assoc) / float(C) - mean * mean
    else:
        d = x[:, :nv] - mean.unsqueeze(1)
        var = _fsum(d * d, assoc) / (div or float(nv))
    rstd = torch.rsqrt(var + (0.0 if mut == "no_eps" else torch.tensor(k.eps, dtype=F32)))
    o = (x - mean.unsqueeze(1)) * rstd.unsqueeze(1) * k.gamma + k.beta
    if k.p_post > 0:
        o = o * (N.keep_rows(k.seed_post, k.rows, C, k.p_post, k.offset, **_mask_fault(mut, "post")).float() * N.drop_scale(k.p_post))
    o = torch.where(_pad(k, mut).unsqueeze(1), torch.zeros(()), o)
    return zs, mean, rstd, N.store(o, k.dtype)


def emu_bwd(k, assoc, mut=None):
    C = k.C
    g = k.dout.float() + (k.dout2.float() if k.dout2 is not None else 0.0)
    if k.p_post > 0:
        g = g * (N.keep_rows(k.seed_post, k.rows, C, k.p_post, k.offset, **_mask_fault(mut, "post")).float() * N.drop_scale(k.p_post))
    g = torch.where(_pad(k, mut).unsqueeze(1), torch.zeros(()), g)
    zf, rs = k.z.float(), k.rstd.unsqueeze(1)
    x = (zf - k.mean.unsqueeze(1)) * rs
    gg = g * k.gamma
    s1 = (_fsum(gg, assoc) / float(C)).unsqueeze(1)
    s2 = (_fsum(gg * x, assoc) / float(C)).unsqueeze(1)
    dz = rs * (gg - s1 - x * s2)
    d1 = N.store(dz + k.d1_add.float() if k.d1_add is not None else dz, k.dtype) if k.want_d1 else None
    d2 = None
    if k.want_d2:
        o = dz
        if k.p_pre > 0:
            o = o * (N.keep_rows(k.seed_pre, k.rows, C, k.p_pre, k.offset, **_mask_fault(mut, "pre")).float() * N.drop_scale(k.p_pre))
        if k.relu_bwd:
            o = torch.where((zf >= 0) if mut == "relu_zero" else (zf > 0), o, torch.zeros(()))
        d2 = N.store(o, k.dtype)
    dgamma = k.dgamma0 + _fsum((g * x).t().contiguous(), assoc)
    dbeta = k.dbeta0 + _fsum(g.t().contiguous(), assoc)
    return d1, d2, dgamma, dbeta


def _rejected(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


# the forward inputs of tests/test_norm_gpu.py, thinned to one of each kind (the GPU file runs all of them)
def _fwd_cases():
    out = []
    for dtype in (F32, BF16):
        for C in (4, 260, 512, 2048):
            out.append(N.fwd_case(dtype, 3, 7, C, p_pre=0.5, p_post=0.1))
        out.append(N.fwd_case(dtype, 3, 5, 256, p_pre=0.1, p_post=0.5))
        out.append(N.fwd_case(dtype, 3, 7, 256, res=False, lens=False))
        for fam in N.FAMILIES[1:]:
            if not (fam == "bigmean" and dtype == BF16):
                out.append(N.fwd_case(dtype, 3, 7, 256, family=fam, res=False))
    out.append(N.fwd_case(F32, 3, 7, 516, family="bigmean", res=False))
    return out


def _name(k):
    return f"{k.dtype} C={k.C} {k.B}x{k.S} {getattr(k, 'family', getattr(k, 'form', ''))}"


@pytest.mark.parametrize("assoc", ["seq", "pair"])
def test_forward_bounds_accept_other_associations(assoc):
    for k in _fwd_cases():
        if assoc == "seq" and k.family == "bigmean":
            # one chain of C - 1 additions whose running sum is 10^5 spreads: every rounding has the same sign and nothing averages
            # out, so this association is held to the bound of ITS chain length (k.chain overrides the kernel's)
            k.chain = k.C - 1
        rep = N.verify_fwd(k, *emu_fwd(k, assoc))
        assert all(v == v for v in rep.values()), _name(k)


def test_forward_checks_reject_faults():
    seen = set()
    for k in _fwd_cases():
        muts = ["mean4", "var4", "c_minus_1"] if k.family not in ("const", "tiny") else []   # (a constant row has no spread to mis-state)
        if k.family == "tiny":
            muts = ["no_eps"]
        if k.family == "bigmean":
            muts.append("one_pass")
            muts.remove("mean4")          # (4 of 256 channels move this mean by less than the roundings of 1000; the other families see it)
        if k.dtype == BF16 and k.res is not None:
            muts.append("unrounded")
        if k.lens is not None and k.family == "randn":
            muts.append("pad_gt")
        for site, p in (("pre", k.p_pre), ("post", k.p_post)):
            if p > 0:
                muts.append(f"shift_{site}")
                if k.C != 256:
                    muts.append(f"index256_{site}")
                if p == 0.5:
                    muts.append(f"strict_{site}")
        for mut in muts:
            assert _rejected(N.verify_fwd, k, *emu_fwd(k, "pair", mut)), f"{mut} passes at {_name(k)}"
            seen.add(mut.split("_p")[0] if mut.endswith(("_pre", "_post")) else mut)
    assert seen >= {"mean4", "var4", "c_minus_1", "no_eps", "one_pass", "unrounded", "pad_gt", "shift", "index256", "strict"}


def _bwd_cases():
    out = [N.bwd_case(dtype, 3, 7, C, form) for dtype in (F32, BF16) for C in (256, 512) for form in N.FORMS]
    out += [N.bwd_case(F32, 3, 7, 2048, "all"), N.bwd_case(BF16, 3, 7, 1024, "all")]
    return out


@pytest.mark.parametrize("assoc", ["seq", "pair"])
def test_backward_bounds_accept_other_associations(assoc):
    for k in _bwd_cases():
        N.verify_bwd(k, *emu_bwd(k, assoc))


def test_backward_checks_reject_faults():
    seen = set()
    for k in _bwd_cases():
        muts = ["pad_gt"]
        if k.relu_bwd:
            muts.append("relu_zero")
        for site, p, used in (("pre", k.p_pre, k.want_d2), ("post", k.p_post, True)):
            if p > 0 and used:
                muts.append(f"shift_{site}")
                if k.C != 256:
                    muts.append(f"index256_{site}")
                if p == 0.5:
                    muts.append(f"strict_{site}")
        for mut in muts:
            assert _rejected(N.verify_bwd, k, *emu_bwd(k, "pair", mut)), f"{mut} passes at {_name(k)}"
            seen.add(mut)
    assert seen >= {"pad_gt", "relu_zero", "shift_pre", "shift_post", "index256_pre", "index256_post", "strict_pre", "strict_post"}
