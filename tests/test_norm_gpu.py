"""LayerNorm forward / backward and every dropout site, element by element: the masks against the integer restatement of the
generator (exact), the arithmetic against fp64 within bounds counted from the kernels (tests/norm_ref.py).
Each case prints the largest err / (u mag) it saw ("[elem] ..." lines, shown with -s)."""
import pytest
import torch

from tests import norm_ref as N
from tests.test_elem_gpu import _bn_ref_bwd, _bn_stat_bounds

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]


def _ops():
    from fastspeech2_amd import ops
    return ops


def _rep(what, rep):
    print(f"[elem] {what}: max err/(u mag) " + ", ".join(f"{n} {v:.3g}" for n, v in rep.items()))


def _d(t, dev):
    return None if t is None else t.to(dev)


def _seed_dev(offset, dev):
    return torch.tensor([offset], dtype=torch.int64, device=dev) if offset else None


def _offset(with_dev):
    return N.carrying_offset(0) if with_dev else 0


def _run_fwd(dev, k):
    """fs2_ln_fwd on the case -> z (y written back), mean, rstd, out on the CPU.  aligned=False: y starts 8 bytes into its buffer."""
    ops = _ops()
    if k.aligned:
        y = k.y.to(dev).clone()
    else:
        flat = torch.zeros(k.rows * k.C + 8, dtype=k.dtype, device=dev)
        y = flat[4:4 + k.rows * k.C].view(k.rows, k.C)
        y.copy_(k.y)
        assert y.data_ptr() % 16 == 8 and y.is_contiguous()
    out, mean, rstd = ops.ln_fwd(y, _d(k.res, dev), k.gamma.to(dev), k.beta.to(dev), _d(k.lens, dev), k.B, k.S, eps=k.eps,
                                 p_pre=k.p_pre, seed_pre=k.seed_pre, p_post=k.p_post, seed_post=k.seed_post,
                                 seed_dev=_seed_dev(k.offset, dev))
    return y.cpu(), mean.cpu(), rstd.cpu(), out.cpu()


def _same_set(dropped, keep, what):
    n = int((dropped != ~keep).sum())
    assert n == 0, f"{what}: the dropped set differs from the restated mask in {n} of {keep.numel()} elements"


def _eq(got, ref, what):
    n = int((N.bits(got) != N.bits(ref)).sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} elements differ"


# --------------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("with_dev", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("C", [256, 512, 260])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_fwd_masks_exact(dev, dtype, C, p, with_dev):
    """both LayerNorm sites against the restated generator, seeds with a non-zero high half, with and without a carrying
    seed_dev offset; at p = 0.5 one element of each site draws u == p exactly and must be kept.  The same restated mask serves both
    dtypes and all three kernels (bf16 C = 256, NV = 1, NV = 2 with a partial group at 260).
    pre: res absent, so z = store(y ik keep) bit for bit.  post: gamma = 1, beta = 8 (no output is zero); fp32 kept values are
    fl(o ik) of the p_post = 0 output o bit for bit, bf16 ones 2 o at p = 0.5 and within the bound of the elementwise check at
    p = 0.1 (o is rounded to bf16 after the product)."""
    off = _offset(with_dev)
    k = N.fwd_case(dtype, 3, 7, C, res=False, lens=False, p_pre=p, offset=off)
    assert k.seed_pre >> 32 != 0 and (not with_dev or ((k.seed_pre & N.M32) + (off & N.M32)) >> 32 == 1)
    z, mean, rstd, out = _run_fwd(dev, k)
    keep = N.keep_rows(k.seed_pre, k.rows, C, p, off)
    _same_set(z == 0, keep, "p_pre")
    assert p != 0.5 or bool(keep.view(-1)[k.tie_pre])
    N.verify_fwd(k, z, mean, rstd, out)                                    # (z bit for bit: one rounded operation)
    k = N.fwd_case(dtype, 3, 7, C, res=False, lens=False, p_post=p, offset=off, gamma_one=True, beta_fill=8.0)
    z, mean, rstd, out = _run_fwd(dev, k)
    k0 = N.fwd_case(dtype, 3, 7, C, res=False, lens=False, gamma_one=True, beta_fill=8.0)
    o0 = _run_fwd(dev, k0)[3]
    assert bool((o0 != 0).all())
    keep = N.keep_rows(k.seed_post, k.rows, C, p, off)
    _same_set(out == 0, keep, "p_post")
    assert p != 0.5 or bool(keep.view(-1)[k.tie_post])
    if dtype == F32 or p == 0.5:
        _eq(out, N.store(o0.float() * (keep.float() * N.drop_scale(p)), dtype), "p_post kept values")
    _rep(f"ln_fwd masks {dtype} C={C} p={p} seed_dev={with_dev}", N.verify_fwd(k, z, mean, rstd, out))


@pytest.mark.parametrize("with_dev", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("C", [20, 80, 512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_masks_exact(dev, dtype, C, p, with_dev):
    """BatchNorm apply (4 channels per thread; 8 for bf16 at C % 8 == 0) and backward against the restated generator.  Apply with
    identity statistics (mean 0, rstd 1, gamma 1, beta 0) stores store(x ik keep) bit for bit; bn_train_fwd drops the same set;
    the backward's dgamma, dbeta and dx are held to _bn_ref_bwd with the restated mask."""
    ops = _ops()
    from fastspeech2_amd import _lib
    g = torch.Generator().manual_seed(C + int(p * 10))
    M = 77
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    x = torch.where(x.to(dtype) == 0, torch.ones(()), x).to(dtype)
    off = _offset(with_dev)
    seed = N.site_seed(p, 0xC2B2AE35, (M * C) // 2 + 3, off)
    sd = _seed_dev(off, dev)
    keep = N.keep_rows(seed, M, C, p, off)
    ik = N.drop_scale(p)
    xd = x.to(dev)
    ident = torch.cat([torch.zeros(C), torch.ones(C)]).to(dev)
    out = torch.empty_like(xd)
    _lib.call("fs2_bn_apply", xd.data_ptr(), ident.data_ptr(), ident[C:].data_ptr(), ident[:C].data_ptr(), None, out.data_ptr(), M, C,
              ops.ACT_NONE, p, seed, None if sd is None else sd.data_ptr(), ops.dt(dtype), ops._stream())
    _same_set(out.cpu() == 0, keep, "bn_apply")
    _eq(out, N.store(x.float() * (keep.float() * ik), dtype), "bn_apply kept values")
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.full((C,), 9.0)
    o, mr = ops.bn_train_fwd(xd, gamma.to(dev), beta.to(dev), None, None, ops.ACT_NONE, p, seed, seed_dev=sd)
    _same_set(o.cpu() == 0, keep, "bn_train_fwd")
    dout = torch.randn(M, C, generator=g).to(dtype)
    dx, dgam, dbet = ops.bn_bwd(xd, dout.to(dev), mr, gamma.to(dev), beta.to(dev), ops.ACT_NONE, p, seed, seed_dev=sd)
    rdx, mdx, (rdb, mdb), (rdg, mdg) = _bn_ref_bwd(x.float(), dout.double() * (keep.double() * ik), mr.cpu(), gamma)
    c_sum = M + 5                      # any association of M terms; xhat (2), g ik (1) and g * xhat (1) rounded
    rep = dict(dbeta=N.check(dbet, rdb, mdb, c_sum, what="bn dbeta"), dgamma=N.check(dgam, rdg, mdg, c_sum, what="bn dgamma"),
               dx=N.check(dx, rdx, mdx, c_sum + 8, dtype, what="bn dx"))
    _rep(f"bn masks {dtype} C={C} p={p} seed_dev={with_dev}", rep)


@pytest.mark.parametrize("with_dev", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,K,streams", [(23, 167, 128, False), (19, 859, 256, True)])
def test_gemm_res_ln_mask_exact(dev, B, S, K, streams, p, with_dev):
    """the LayerNorm epilogues of the wide contraction kernel (its smallest supported shape: 16 tiles of 256 rows, Cin = 128) and of
    the streaming K = 256 kernel (its smallest: a 64-row tile for each of 256 compute units).  Small-integer operands make the fp32
    product exact and bias k + 1/8 keeps it off zero, so z = bf16(y ik keep + res) is known to two roundings and a dropped element
    is exactly res."""
    ops = _ops()
    from fastspeech2_amd import _lib
    Nn, M = 256, B * S
    lib = _lib.load()
    assert lib.fs2_gemm_res_ln_supported(M, Nn, K, S, ops.BF16) and bool(lib.fs2_gemm_res_ln_streams(M, Nn, K, S, ops.BF16)) == streams
    assert not (lib.fs2_gemm_res_ln_streams if streams else lib.fs2_gemm_res_ln_supported)(M - S, Nn, K, S, ops.BF16)
    g = torch.Generator().manual_seed(5 + int(p * 10) + K)
    x = torch.randint(-2, 3, (M, K), generator=g).to(BF16)
    w = torch.randint(-1, 2, (Nn, 1, K), generator=g).to(BF16)
    bias = torch.randint(-3, 4, (Nn,), generator=g).float() + 0.125
    res = (torch.randint(-8, 9, (M, Nn), generator=g).float() / 16).to(BF16)
    off = _offset(with_dev)
    seed = N.site_seed(p, 0x27D4EB2F, 5 * Nn + 77, off)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    r = ops.gemm_res_ln(x.to(dev), w.to(dev), bias.to(dev), res.to(dev), torch.ones(Nn, device=dev), torch.zeros(Nn, device=dev), lens,
                        ops.tile_map(lens, B, S), B, S, p_pre=p, seed_pre=seed, seed_dev=_seed_dev(off, dev))
    assert r is not None, "shape not taken by the fused kernel"
    z = r[0].cpu()
    y = x.double() @ w.double().view(Nn, K).t() + bias.double()            # exact in fp32 as well: integers below 2^10, eighths
    assert bool((y != 0).all())
    keep = N.keep_rows(seed, M, Nn, p, off)
    sc = keep.double() * N.drop_scale(p)
    _same_set(z == res, keep, "gemm_res_ln")                               # (|y ik| >= 1/8 moves every kept element off res)
    rep = dict(z=N.check(z, y * sc + res.double(), (y * sc).abs() + res.double().abs(), 2, BF16, what="gemm_res_ln z"))
    _rep(f"gemm_res_ln mask K={K} p={p} seed_dev={with_dev}", rep)


# ---------------------------------------------------------------------------------------------------------- LayerNorm forward
def _fwd(dev, k, what):
    _rep(f"ln_fwd {what} {k.dtype} C={k.C} {k.B}x{k.S}", N.verify_fwd(k, *_run_fwd(dev, k)))


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("C", [4, 8, 252, 256, 260, 512, 516, 1024, 1028, 2048])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_fwd_widths(dev, dtype, C, extras):
    """every NV instantiation, with whole and partial last 256-groups; extras: residual, lens [7, 0, 4], both dropouts"""
    if extras:
        _fwd(dev, N.fwd_case(dtype, 3, 7, C, p_pre=0.5, p_post=0.1, offset=_offset(C % 8 == 0)), "widths+")
    else:
        _fwd(dev, N.fwd_case(dtype, 3, 7, C, res=False, lens=False), "widths")


@pytest.mark.parametrize("B,S", [(1, 1), (3, 1), (4, 1), (1, 5), (5, 1), (3, 5), (15, 1), (16, 1), (17, 1), (3, 11), (33, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_fwd_rows(dev, dtype, B, S):
    """C = 256 around the 16 rows of a bf16 workgroup and the 4 of a generic one (clamped loads, `ok` guards), batch boundaries
    inside a wave's rows and between the two rows of a half-wave pair, lens containing 0 and S"""
    _fwd(dev, N.fwd_case(dtype, B, S, 256, p_pre=0.1, p_post=0.5), "rows+")
    _fwd(dev, N.fwd_case(dtype, B, S, 256, res=False, lens=False), "rows")


@pytest.mark.parametrize("res", [False, True])
def test_ln_fwd_misaligned_bf16(dev, res):
    """bf16 C = 256 with y 8 bytes into its buffer: the generic kernel, the same bounds (its own chain) and the identical mask"""
    k = N.fwd_case(BF16, 3, 7, 256, res=res, p_pre=0.5, p_post=0.1, aligned=False)
    zm, mean, rstd, outm = _run_fwd(dev, k)
    _rep(f"ln_fwd misaligned res={res}", N.verify_fwd(k, zm, mean, rstd, outm))
    k.aligned = True
    za, _, _, outa = _run_fwd(dev, k)
    assert torch.equal(outa == 0, outm == 0)
    if not res:
        _eq(zm, za, "z of the two kernels")
        _same_set(zm == 0, N.keep_rows(k.seed_pre, k.rows, 256, 0.5), "misaligned p_pre")


@pytest.mark.parametrize("dtype,C,family", [(d, c, f) for d, c in ((F32, 256), (BF16, 256), (F32, 516)) for f in N.FAMILIES[1:]
                                            if not (f == "bigmean" and d == BF16)])
def test_ln_fwd_variance_regimes(dev, dtype, C, family):
    """a constant row (out == beta, rstd == eps^-1/2 within the bounds), mean 1000 with spread 0.01 (fp32: bf16 cannot hold it),
    values of 1e-6 (variance far below eps), of 1e15, and a single outlier"""
    k = N.fwd_case(dtype, 3, 7, C, family=family, res=False)
    z, mean, rstd, out = _run_fwd(dev, k)
    _rep(f"ln_fwd {family} {dtype} C={C}", N.verify_fwd(k, z, mean, rstd, out))
    if family == "const":
        assert torch.allclose(rstd.double(), torch.full((k.rows,), 1e-5 ** -0.5, dtype=torch.float64), rtol=1e-4, atol=0)


# --------------------------------------------------------------------------------------------------------- LayerNorm backward
def _run_bwd(dev, k):
    ops = _ops()
    dg, db = k.dgamma0.to(dev), k.dbeta0.to(dev)
    r = ops.ln_bwd(k.z.to(dev), k.dout.to(dev), k.gamma.to(dev), _d(k.lens, dev), k.mean.to(dev), k.rstd.to(dev), dg, db, k.B, k.S,
                   want_d1=k.want_d1, want_d2=k.want_d2, d1_add=_d(k.d1_add, dev), p_pre=k.p_pre, seed_pre=k.seed_pre,
                   p_post=k.p_post, seed_post=k.seed_post, relu_bwd=k.relu_bwd, seed_dev=_seed_dev(k.offset, dev), defer=k.defer,
                   dout2=_d(k.dout2, dev))
    if k.defer:
        ops.ln_bwd_reduce(r[2], k.C, dg, db)
    return r[0], r[1], dg, db


@pytest.mark.parametrize("form", N.FORMS)
@pytest.mark.parametrize("C", [256, 512, 1024, 2048])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_bwd_forms(dev, dtype, C, form):
    """3 x 7 rows, lens [7, 0, 4]: the batch boundaries fall between the two rows of a half-wave pair.  On padded rows d1 is d1_add
    bit for bit and d2 exactly zero; dout and dout2 hold NaN there and it reaches no output.  z, mean and rstd are finite on every
    row, padded ones included: the forward writes them for every row, and the backward relies on it (0 * NaN would not be 0)."""
    k = N.bwd_case(dtype, 3, 7, C, form)
    _rep(f"ln_bwd {form} {dtype} C={C}", N.verify_bwd(k, *_run_bwd(dev, k)))


@pytest.mark.parametrize("dtype,C,rows", [(BF16, 256, 16385), (BF16, 256, 32768), (BF16, 256, 32769), (F32, 256, 8200), (F32, 512, 8200)])
def test_ln_bwd_row_loops(dev, dtype, C, rows):
    """the row loops past their first trip: the bf16 kernel's prefetched second and third sweeps (1024 workgroups x 16 rows; a
    partial and an exact last sweep), the generic kernel's grid stride (1024 x 8 rows), with p_pre and d1_add on"""
    k = N.bwd_case(dtype, 1, rows, C, "all")
    k.relu_bwd, k.dout2, k.p_post = False, None, 0.0
    k.lens = torch.tensor([rows - 3], dtype=torch.int32)
    _rep(f"ln_bwd rows={rows} {dtype} C={C}", N.verify_bwd(k, *_run_bwd(dev, k)))


# --------------------------------------------------------------------------------------------------- BatchNorm, tiny row counts
@pytest.mark.parametrize("C", [4, 80])
@pytest.mark.parametrize("M", [1, 2, 5])
def test_batchnorm_tiny_rows(dev, M, C):
    """fewer rows than row lanes; M = 1 takes the `unb = var` branch of the running variance"""
    ops = _ops()
    g = torch.Generator().manual_seed(10 * M + C)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    o, mr = ops.bn_train_fwd(x.to(dev), gamma.to(dev), beta.to(dev), rm, rv, ops.ACT_NONE, 0.0, 0)
    mean, mean_m, ssd, ssd_m = _bn_stat_bounds(x, M)
    rep = dict(mean=N.check(mr[:C], mean, mean_m, M + 4, what="bn mean"))
    var = ssd / M
    rs_ref = (var + 1e-5).rsqrt()
    rs_lim = rs_ref * (0.5 * (M + 6) * N.U32 * ssd_m / M / (var + 1e-5) + 4 * N.U32)
    assert bool(((mr[C:].cpu().double() - rs_ref).abs() <= rs_lim).all()), "bn rstd"
    unb = ssd / (M - 1) if M > 1 else var
    rep["running_mean"] = N.check(rm, 0.1 * mean, 0.1 * mean_m * (M + 8), 4, what="running_mean")
    rep["running_var"] = N.check(rv, 0.9 + 0.1 * unb, 0.9 + 0.1 * ssd_m / max(M - 1, 1) * (M + 8), 4, what="running_var")
    xh = (x.double() - mr[:C].cpu().double()) * mr[C:].cpu().double()
    ref_o = xh * gamma.double() + beta.double()
    rep["out"] = N.check(o, ref_o, (xh * gamma.double()).abs() + beta.double().abs(), 4, what="bn out")
    dout = torch.randn(M, C, generator=g)
    dx, dgam, dbet = ops.bn_bwd(x.to(dev), dout.to(dev), mr, gamma.to(dev), beta.to(dev), ops.ACT_NONE, 0.0, 0)
    rdx, mdx, (rdb, mdb), (rdg, mdg) = _bn_ref_bwd(x, dout, mr.cpu(), gamma)
    rep["dbeta"] = N.check(dbet, rdb, mdb, M + 4, what="bn dbeta")
    rep["dgamma"] = N.check(dgam, rdg, mdg, M + 4, what="bn dgamma")
    rep["dx"] = N.check(dx, rdx, mdx, M + 12, what="bn dx")
    _rep(f"bn tiny M={M} C={C}", rep)
