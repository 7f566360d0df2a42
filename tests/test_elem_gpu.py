"""The gather, cast, loss, optimiser and normalisation-side kernels of the train step, element by element against fp64 (or
exact fp32 / integer) restatements - tests/elem_ref.py holds the references and the bounds.  One-operation kernels must be
bit-exact; reductions must stay within c * u * mag of the exact sum, c read from the kernel's summation chain.
Each test prints the largest err / (u mag) it saw ("[elem] ..." lines, shown with -s)."""
import math

import pytest
import torch

from tests import elem_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from fastspeech2_amd import ops
    return ops


def _eq(got, ref, what):
    g, r = R.bits(got), R.bits(ref)
    n = int((g != r).sum())
    assert n == 0, f"{what}: {n} of {g.numel()} elements differ"
    print(f"[elem] {what}: {g.numel()} / {g.numel()} bit-exact")


def _rep(what, ratio, c):
    print(f"[elem] {what}: max err/(u mag) = {ratio:.3g} (c = {c})")


# ------------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [80, 260])
def test_embed_pe_edges(dev, dtype, C):
    ops = _ops()
    torch.manual_seed(31)
    B, L, V = 5, 37, 50
    tok = torch.randint(1, V, (B, L))
    tok[0, :3] = torch.tensor([-1, V, V + 7])                 # out of range: row 0 forward, no gradient
    tok[1] = 7                                                 # a heavily repeated id
    tok[2, 20:] = 0                                            # padding rows
    emb, pe = torch.randn(V, C), torch.randn(64, C)
    out = ops.embed_pe_fwd(tok.to(dev), emb.to(dev), pe.to(dev), dtype)
    _eq(out, R.embed_pe(tok, emb, pe, dtype), f"embed_pe_fwd {dtype} C={C}")
    dy = torch.randn(B * L, C).to(dtype)
    init = torch.randn(V, C)
    demb = init.to(dev)
    ops.embed_bwd(tok.to(dev), dy.to(dev), demb, pad_idx=0)
    ref, mag, c = R.embed_bwd(tok, dy, V, 0, init)
    _rep(f"embed_bwd {dtype} C={C}", R.check(demb, ref, mag, c, what="embed_bwd"), "rows per id")
    assert torch.equal(demb[0].cpu(), init[0]), "pad_idx row received a gradient"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1, 1000])
def test_speaker_rowvec(dev, dtype, S):
    ops = _ops()
    torch.manual_seed(32)
    B, C, V = 7, 256, 5
    idx = torch.tensor([3, 3, 1, 3, -2, 9, 1])                 # shared ids; -2 and 9 use row 0
    table = torch.randn(V, C)
    x = torch.randn(B * S, C).to(dtype)
    xd = x.to(dev)
    ops.add_rowvec(xd, table.to(dev), idx.to(dev), B, S)
    _eq(xd, R.add_rowvec(x, table, idx, B, S), f"add_rowvec {dtype} S={S}")
    dy = torch.randn(B * S, C).to(dtype)
    init = torch.randn(V, C)
    dt = init.to(dev)
    ops.rowvec_bwd(dy.to(dev), dt, idx.to(dev), B, S)
    ref, mag, c = R.rowvec_bwd(dy, idx, B, S, V, init)
    _rep(f"rowvec_bwd {dtype} S={S}", R.check(dt, ref, mag, c, what="rowvec_bwd"), "S - 1 + sharing")


# ------------------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [4, 80, 252, 256, 260, 1024])
def test_row_kernels(dev, dtype, C):
    ops = _ops()
    torch.manual_seed(33)
    B, S = 3, 67
    lens = torch.tensor([67, 0, 40], dtype=torch.int32)
    a = torch.randn(B * S, C).to(dtype)
    b = torch.randn(B * S, C).to(dtype)
    pe = torch.randn(S, C)
    _eq(ops.add(a.to(dev), b.to(dev)), R.store(a.float() + b.float(), dtype), f"add {dtype} C={C}")
    xd = a.to(dev)
    ops.add_pe(xd, pe.to(dev), B, S)
    _eq(xd, R.store((a.float().view(B, S, C) + pe).reshape(B * S, C), dtype), f"add_pe {dtype} C={C}")
    xd = a.to(dev)
    ops.mask_rows(xd, lens.to(dev), B, S)
    ref = torch.where(R.padding(lens, B, S).reshape(-1, 1), torch.zeros((), dtype=dtype), a)
    _eq(xd, ref, f"mask_rows {dtype} C={C}")
    w, bias = torch.randn(C), torch.randn(1)
    y = ops.rowdot_fwd(a.to(dev), w.to(dev), bias.to(dev), lens.to(dev), B, S)
    ref, mag, c = R.rowdot_fwd(a, w, bias, lens, B, S)
    _rep(f"rowdot_fwd {dtype} C={C}", R.check(y.view(-1), ref, mag, c, what="rowdot_fwd"), c)
    assert torch.all(y.cpu()[1] == 0) and torch.all(y.cpu()[2, 40:] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S", [(1, 300), (4, 256), (3, 700)])
def test_rowdot_bwd(dev, dtype, B, S):
    """rows below, at and above the 512-block grid (1024 is a multiple of it, 2100 is not); lengths 0 and S."""
    ops = _ops()
    torch.manual_seed(34)
    C = 256
    lens = torch.tensor([S, 0, S // 3, S][:B], dtype=torch.int32) if B > 1 else torch.tensor([S // 2], dtype=torch.int32)
    x = torch.randn(B * S, C).to(dtype)
    w, g = torch.randn(C), torch.randn(B, S)
    dw0, db0 = torch.randn(C), torch.randn(1)
    dw, db = dw0.to(dev), db0.to(dev)
    dx = ops.rowdot_bwd(x.to(dev), w.to(dev), g.to(dev), lens.to(dev), dw, db, B, S)
    rdx, (rdw, mdw), (rdb, mdb), c = R.rowdot_bwd(x, w, g, lens, B, S, dw0, db0)
    _eq(dx, rdx, f"rowdot_bwd dx {dtype} rows={B * S}")
    _rep(f"rowdot_bwd dw {dtype} rows={B * S}", R.check(dw, rdw, mdw, c, what="rowdot_bwd dw"), c)
    _rep(f"rowdot_bwd db {dtype} rows={B * S}", R.check(db, rdb.view(1), mdb.view(1), c, what="rowdot_bwd db"), c)


# ------------------------------------------------------------------------------------------------------------- bucketize
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1.7])
def test_bucket_embed_fwd_edges(dev, dtype, scale):
    ops = _ops()
    torch.manual_seed(35)
    nb, C, rows = 256, 256, 3000
    bins = torch.linspace(-2.9, 11.3, nb - 1)
    vals = torch.randn(rows) * 5
    vals[:255] = bins / scale                                  # on (or next to) every bin
    vals[255:259] = torch.tensor([float("inf"), float("-inf"), float("nan"), float("nan")])
    emb = torch.randn(nb, C)
    x = torch.randn(rows, C).to(dtype)
    out, idx = ops.bucket_embed_add_fwd(x.to(dev), vals.to(dev), scale, bins.to(dev), emb.to(dev))
    ridx = R.bucketize(vals, scale, bins)
    assert int(ridx[257]) == nb - 1 and int(ridx[258]) == nb - 1       # NaN -> the last bucket, as torch.bucketize
    n_bad = int((idx.cpu().long() != ridx).sum())
    assert n_bad == 0, f"{n_bad} bucket indices differ from torch.bucketize (NaN rows: {idx.cpu()[257:259].tolist()})"
    _eq(out, R.store(x.float() + emb[ridx], dtype), f"bucket_embed_add_fwd {dtype} scale={scale}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bucket_embed_bwd_bounds(dev, dtype):
    """3 splits of 1024 rows, one bin taking > 256 rows of one chunk, bins never hit, += into a non-zero gradient"""
    ops = _ops()
    torch.manual_seed(36)
    nb, C, rows = 256, 260, 2500
    idx = torch.randint(0, 200, (rows,), dtype=torch.int32)   # bins 200.. are never hit
    idx[:300] = 52                                             # > 256 rows of the first chunk in one bin
    idx[1500:2100] = 7
    dy = torch.randn(rows, C).to(dtype)
    init = torch.randn(nb, C)
    demb = init.to(dev)
    ops.bucket_embed_bwd(idx.to(dev), dy.to(dev), demb)
    ref, mag, c = R.bucket_embed_bwd(idx, dy, nb, init)
    _rep(f"bucket_embed_bwd {dtype}", R.check(demb, ref, mag, c, what="bucket_embed_bwd"), "per-bin chain")
    assert torch.equal(demb[200:].cpu(), init[200:])


# ------------------------------------------------------------------------------------------------------ length regulator
def _lr_plain(dur, T):
    """plain-Python LengthRegulator indices: cum (exclusive), idx per frame (-1 past the end), mel_len"""
    B, L = dur.shape
    cum = torch.zeros(B, L + 1, dtype=torch.int64)
    idx = torch.full((B, T), -1, dtype=torch.int64)
    for b in range(B):
        run = 0
        for i in range(L):
            n = max(int(dur[b, i]), 0)
            cum[b, i] = run
            for t in range(run, min(run + n, T)):
                idx[b, t] = i
            run += n
        cum[b, L] = run
    return cum, idx, cum[:, L].clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,crop", [(37, True), (1000, False), (3000, True)])
def test_length_regulator_elementwise(dev, dtype, L, crop):
    ops = _ops()
    torch.manual_seed(37)
    B, C = 3, 256
    dur = torch.randint(0, 4, (B, L)).float()
    dur[1] = 0                                                 # all-zero durations
    dur[2, :5] = torch.tensor([-2.0, 2.7, 0.4, 3.0, 1.0])      # negative and fractional: truncation toward zero
    total = int(dur.clamp_min(0).long().sum(1).max())
    T = total - 3 if crop else total + 5                       # crop lands inside a segment of row 0 (or not at all)
    cum, idx, mel_len = ops.lr_index(dur.to(dev), T)
    rc, ri, rl = _lr_plain(dur, T)
    assert torch.equal(cum.cpu().long(), rc) and torch.equal(idx.cpu().long(), ri) and torch.equal(mel_len.cpu(), rl)
    _, _, ml1 = ops.lr_index(dur.to(dev), 1)                   # the engine's mel_len-only call
    assert torch.equal(ml1.cpu(), rl)
    x = torch.randn(B * L, C).to(dtype)
    pe = torch.randn(T, C)
    for p in (None, pe):
        out = ops.lr_gather_fwd(x.to(dev), idx, None if p is None else p.to(dev), B, L, T)
        _eq(out, R.lr_gather(x, idx, p, B, L, T), f"lr_gather_fwd {dtype} L={L} pe={p is not None}")
    dy = torch.randn(B * T, C).to(dtype)
    dx = ops.lr_gather_bwd(dy.to(dev), cum, B, L, T)
    ref, mag, c = R.lr_gather_bwd(dy, cum, B, L, T)
    _rep(f"lr_gather_bwd {dtype} L={L}", R.check(dx, ref, mag, c, dtype, what="lr_gather_bwd"), "segment length")
    init = torch.randn(B * L, C).to(dtype)
    dxa = init.to(dev)
    ops.lr_gather_bwd(dy.to(dev), cum, B, L, T, dx=dxa, accumulate=True)
    ref, mag, c = R.lr_gather_bwd(dy, cum, B, L, T, init=init)
    _rep(f"lr_gather_bwd acc {dtype} L={L}", R.check(dxa, ref, mag, c, dtype, what="lr_gather_bwd accumulate"), "segment + 1")


# -------------------------------------------------------------------------------------------------------------------- cast
def test_cast_bf16_to_f32_every_pattern(dev):
    ops = _ops()
    allp = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    got = ops.cast(allp.to(dev), torch.float32)
    _eq(got, allp.float(), "cast bf16->f32, all 65536 patterns")


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_cast_f32_to_bf16_edges(dev):
    """fp32 subnormals convert exactly as on the CPU: the kernels are built with fp32 denormals preserved
    (.amdhsa_float_denorm_mode_32 3 under the project's HIPFLAGS) and v_cvt_pk_bf16_f32 rounds them to nearest even."""
    ops = _ops()
    torch.manual_seed(38)
    special = [
        0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF,        # ties to even (down, up) and just past / short of a tie
        0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,                    # largest finite that stays finite; the first that rounds to inf
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80400000, 0x00800000,   # subnormals, smallest normal
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,
    ]
    sp = _f32(special)
    n = 2048 * 256 * 4 + 2048 * 4 * 3 + 12                     # beyond one sweep of the 2048-block grid-stride loop
    x = torch.randn(n) * 10.0 ** torch.randint(-30, 30, (n,)).float()
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp
    got = ops.cast(x.to(dev), torch.bfloat16).cpu()
    ref = R.rne_bf16(x)
    nan = torch.isnan(x)
    assert torch.isnan(got[nan].float()).all()
    diff = (R.bits(got) != R.bits(ref)) & ~nan
    sub = (x.abs() < 2.0 ** -126) & (x != 0)
    assert int(diff.sum()) == 0, (f"{int(diff.sum())} of {n} casts differ ({int((diff & sub).sum())} of them subnormal inputs): "
                                  f"x {x[diff][:4].tolist()} got {got[diff][:4].float().tolist()} ref {ref[diff][:4].float().tolist()}")
    print(f"[elem] cast f32->bf16: {n - int(nan.sum())} / {n - int(nan.sum())} bit-exact, {int(nan.sum())} NaN kept")


# --------------------------------------------------------------------------------------------------------------- lens_prep
@pytest.mark.parametrize("B,S", [(1, 256), (1, 77), (48, 128), (48, 925), (5, 7)])
def test_lens_prep(dev, B, S):
    ops = _ops()
    torch.manual_seed(39)
    lens = torch.randint(0, S + 1, (B,))
    special = torch.tensor([-3, 0, S, S + 5, S - 1])
    lens[:min(B, 5)] = special[:min(B, 5)]
    cnt = torch.full((1,), float("nan"), device=dev)
    l32, mask, tmap = ops.lens_prep(lens.to(dev), B, S, cnt)
    cl = [min(max(int(v), 0), S) for v in lens]
    assert l32.cpu().tolist() == cl
    assert torch.equal(mask.cpu(), torch.tensor([[t >= int(v) for t in range(S)] for v in lens]))
    assert cnt.item() == float(sum(cl))
    ref = ops.tile_map(torch.tensor(cl, dtype=torch.int32, device=dev), B, S)
    assert torch.equal(tmap.cpu(), ref.cpu())


# -------------------------------------------------------------------------------------------------------------------- loss
def _ulp(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


@pytest.mark.parametrize("p_frame", [0, 1])
def test_loss_elementwise(dev, p_frame):
    """B=48, T=925, L=128: mel_lens > T, targets longer than the predictions (strided views), predictions equal to the targets at
    chosen positions (sign(0) = 0), NaN in every padded prediction and target position."""
    ops = _ops()
    torch.manual_seed(40)
    B, T, L, n_mel = 48, 925, 128, 80
    e_frame = 1 - p_frame
    mel_lens = torch.randint(T // 2, T + 1, (B,))
    mel_lens[:3] = torch.tensor([T, T + 50, 1])
    src_lens = torch.randint(L // 2, L + 1, (B,))
    src_lens[:3] = torch.tensor([L, 1, L + 9])
    ml, sl = mel_lens.clamp(max=T), src_lens.clamp(max=L)
    fmask = torch.arange(T).unsqueeze(0) < ml.unsqueeze(1)
    smask = torch.arange(L).unsqueeze(0) < sl.unsqueeze(1)
    nan = float("nan")
    mel, post = torch.randn(B, T, n_mel), torch.randn(B, T, n_mel)
    mel_t_full = torch.randn(B, T + 7, n_mel)
    mel[:, :5] = mel_t_full[:, :5]                            # equal to the target: d = 0 -> gradient exactly 0
    post[:, 3:9] = mel_t_full[:, 3:9]
    Pn, En = (T if p_frame else L), (T if e_frame else L)
    p_pred, e_pred = torch.randn(B, Pn), torch.randn(B, En)
    p_big, e_big = torch.randn(B, Pn + 9), torch.randn(B, En + 4)
    logd = torch.randn(B, L)
    dur_big = torch.randint(0, 9, (B, L + 3))
    pmask = fmask if p_frame else smask
    emask = fmask if e_frame else smask
    for t_, m_ in ((mel, fmask), (post, fmask)):
        t_.masked_fill_(~m_.unsqueeze(-1), nan)
    mel_t_full[:, :T].masked_fill_(~fmask.unsqueeze(-1), nan)
    p_pred.masked_fill_(~pmask, nan); e_pred.masked_fill_(~emask, nan); logd.masked_fill_(~smask, nan)
    p_big[:, 2:2 + Pn].masked_fill_(~pmask, nan); e_big[:, 1:1 + En].masked_fill_(~emask, nan)
    views = lambda pb, eb, db: (pb[:, 2:2 + Pn + 5], eb[:, 1:1 + En + 3], db[:, 3:])   # noqa: E731  (strided, longer than the predictions)
    p_t, e_t, dur = views(p_big, e_big, dur_big)
    nsv, nmv = int(sl.sum()), int(ml.sum())
    cnt = torch.tensor([float(nsv), float(nmv)])
    D = lambda t: t.to(dev)                                    # noqa: E731
    p_td, e_td, dur_d = views(D(p_big), D(e_big), D(dur_big))
    args = (D(mel), D(post), D(mel_t_full), D(mel_lens), D(src_lens), D(p_pred), p_td, D(e_pred), e_td, D(logd), dur_d, D(cnt))
    assert args[6].stride(0) == Pn + 9
    losses = ops.loss_fwd(*args, p_frame, e_frame).cpu().double()
    assert torch.isfinite(losses).all()
    terms, ns2, nm2 = R.loss_terms(mel, post, mel_t_full, mel_lens, src_lens, p_pred, p_t, e_pred, e_t, logd, dur, p_frame, e_frame)
    assert (ns2, nm2) == (nsv, nmv)
    bps = min(8, math.ceil(T * n_mel / (256 * 32)))
    den = dict(mel=nmv * n_mel, post=nmv * n_mel, pitch=nmv if p_frame else nsv, energy=nmv if e_frame else nsv, duration=nsv)
    tot, tot_lim, tot_abs, worst = 0.0, 0.0, 0.0, 0.0
    for k, name in enumerate(["mel", "post", "pitch", "energy", "duration"]):
        s, mag, per = terms[name]
        if name in ("mel", "post"):      # per-thread chain + block tree (6 + 3) + atomics over all workgroups + |d| + 2 for the mean
            c = math.ceil(T * n_mel / (bps * 256)) + 9 + B * bps + 1 + 2
        else:                            # block 0 of each sequence: per-thread chain + tree + one atomic per sequence + d^2 + mean
            c = math.ceil(per / 256) + 9 + B + 2 + 2
        extra = 0.0
        if name == "duration":           # device logf vs the CPU log of the target: <= 2 ulp, times |2 d|
            ld = torch.log(dur.float() + 1)[:, :L]
            dd = torch.where(smask, (logd.double() - ld.double()).abs() * 2 * 2 * _ulp(ld), torch.zeros((), dtype=torch.float64))
            extra = float(dd.sum()) / den[name]
        ref, m = float(s) / den[name], float(mag) / den[name]
        err = abs(float(losses[k + 1]) - ref)
        assert err <= c * R.U32 * m + extra, (name, float(losses[k + 1]), ref, c * R.U32 * m + extra)
        worst = max(worst, (err - extra) / (R.U32 * m) if m else 0.0)
        tot, tot_lim, tot_abs = tot + ref, tot_lim + c * R.U32 * m + extra, tot_abs + abs(ref) + c * R.U32 * m + extra
    assert abs(float(losses[0]) - tot) <= tot_lim + 4 * R.U32 * tot_abs          # the total: 4 more fp32 additions
    _rep(f"loss_fwd p_frame={p_frame}", worst, "per term")

    g = torch.tensor([1.0, 0.3, -0.2, 0.1, 0.7, 0.5])
    dmel, dpost, dp, de, dlogd = (t.cpu() for t in ops.loss_bwd(*args[:-1], D(cnt), D(g), p_frame, e_frame))
    f = lambda v: torch.tensor(v, dtype=torch.float32)        # noqa: E731  (the kernel's fp32 scalar arithmetic, on the CPU)
    ns, nm, nmf = f(nsv), f(nmv), f(n_mel)
    km, kq = (g[0] + g[1]) / (nm * nmf), (g[0] + g[2]) / (nm * nmf)
    kp = 2.0 * (g[0] + g[3]) / (nm if p_frame else ns)
    ke = 2.0 * (g[0] + g[4]) / (nm if e_frame else ns)
    kd = 2.0 * (g[0] + g[5]) / ns
    zero = torch.zeros(())
    mt = mel_t_full[:, :T]
    fm3 = fmask.unsqueeze(-1)
    sgn = lambda d, k: torch.where(d > 0, k, torch.where(d < 0, -k, zero))      # noqa: E731
    _eq(dmel, torch.where(fm3, sgn(mel - mt, km), zero), f"loss_bwd dmel p_frame={p_frame}")
    _eq(dpost, torch.where(fm3, sgn(post - mt, kq), zero), f"loss_bwd dpost p_frame={p_frame}")
    assert int((dmel[:, :5][fm3[:, :5].expand(-1, -1, n_mel)] != 0).sum()) == 0
    _eq(dp, torch.where(pmask, kp * (p_pred - p_t[:, :Pn]), zero), f"loss_bwd dp p_frame={p_frame}")
    _eq(de, torch.where(emask, ke * (e_pred - e_t[:, :En]), zero), f"loss_bwd de p_frame={p_frame}")
    ld = torch.log(dur.float() + 1)[:, :L]
    rdl = torch.where(smask, kd * (logd - ld), zero)
    assert torch.isfinite(dlogd).all() and torch.equal(dlogd[~smask], torch.zeros(int((~smask).sum())))
    lim = 2 * _ulp(rdl) + 2 * abs(float(kd)) * _ulp(ld)        # logf within 2 ulp of the CPU's log
    err = (dlogd.double() - rdl.double()).abs()
    assert bool((err <= lim).all()), float((err / lim.clamp_min(1e-300)).max())
    print(f"[elem] loss_bwd dlogd p_frame={p_frame}: {int((err == 0).sum())} / {err.numel()} bit-exact, max err/lim "
          f"{float((err / lim.clamp_min(1e-300)).max()):.3g}")


# --------------------------------------------------------------------------------------------------------- sumsq and Adam
def test_sumsq(dev):
    ops = _ops()
    torch.manual_seed(41)
    big = 1024 * 256 * 4 * 3 + 5                               # above 1024 blocks of work, scalar tail
    for n in list(range(1, 10)) + [1024 * 256 * 4 - 4, big]:
        x = torch.randn(n) * 3
        out0 = 1.25
        out = torch.full((1,), out0, device=dev)
        xd = x.to(dev)
        ops.sumsq(xd, out)
        ref, mag, c = R.sumsq(x, out0)
        r = R.check(out, torch.tensor([ref], dtype=R.F64), torch.tensor([mag], dtype=R.F64), c, what=f"sumsq n={n}")
        again = torch.full((1,), out0, device=dev)
        ops.sumsq(xd, again)
        assert torch.equal(out, again), "sumsq is not bit-reproducible"
        if n in (9, big):
            _rep(f"sumsq n={n}", r, c)
    buf = torch.zeros(64, device=dev)
    with pytest.raises(ValueError, match="aligned"):
        ops.sumsq(buf[1:], torch.zeros(1, device=dev))


@pytest.mark.parametrize("case", ["clip", "noclip", "off", "wd"])
def test_adam_elementwise(dev, case):
    ops = _ops()
    torch.manual_seed(42)
    n = 4096 * 256 * 4 + 4 * 37                                # above 4096 blocks of work
    p, g = torch.randn(n), torch.randn(n) * 1e-3
    m, v = torch.randn(n) * 1e-3, torch.rand(n) * 1e-6
    gsq = {"clip": 1e4, "noclip": 1e-4, "off": 1e4, "wd": 1e4}[case]
    max_norm = 0.0 if case == "off" else 1.0
    wd = 0.01 if case == "wd" else 0.0
    hyper = torch.tensor([1e-3, 1 - 0.9 ** 3, 1 - 0.98 ** 3, 0.0])
    pd, gd, md, vd = p.to(dev), g.to(dev), m.to(dev), v.to(dev)
    lp = torch.empty(n, device=dev, dtype=torch.bfloat16)
    ops.adam_step(pd, gd, md, vd, torch.tensor([gsq], device=dev), max_norm, hyper.to(dev), 0.9, 0.98, 1e-9, wd, p_lowp=lp,
                  zero_grad=True)
    ref = R.adam(p, g, m, v, gsq, max_norm, hyper, 0.9, 0.98, 1e-9, wd)
    for name, got in (("m", md), ("v", vd)):
        r, mag, c = ref[name]
        _rep(f"adam {name} {case}", R.check(got, r, mag, c, what=f"adam {name}"), c)
    r, mag, c = ref["p"]
    pg = pd.cpu().double()
    err = (pg - r).abs()
    lim = c * R.U32 * mag + R.U32 * r.abs()
    assert bool((err <= lim).all()), float(((err - R.U32 * r.abs()) / (R.U32 * mag)).max())
    _rep(f"adam p {case}", float(((err - R.U32 * r.abs()).clamp_min(0) / (R.U32 * mag.clamp_min(1e-300))).max()), c)
    _eq(lp, R.rne_bf16(pd.cpu()), f"adam bf16 shadow {case}")
    assert torch.count_nonzero(gd).item() == 0


def test_adam_misaligned_is_refused(dev):
    ops = _ops()
    buf = torch.zeros(4 * 65, device=dev)
    hyper = torch.tensor([1e-3, 0.1, 0.02, 0.0], device=dev)
    with pytest.raises(ValueError, match="aligned"):
        ops.adam_step(buf[1:65], buf[65:129], buf[129:193], buf[193:257], None, 0.0, hyper, 0.9, 0.98, 1e-9, 0.0)


# ---------------------------------------------------------------------------------------------------- normalisation forms
def _bn_ref_bwd(x, gg, mean_rstd, gamma):
    """fp64 BatchNorm backward (no activation) from the kernel's own mean / rstd and the masked upstream gradient gg:
    dx = gamma rstd (gg - mean(gg) - xhat mean(gg xhat)).  Returns dx, dbeta, dgamma and their magnitudes."""
    M, C = x.shape
    x64, g64 = x.double(), gg.double()
    mu, rs = mean_rstd[:C].double(), mean_rstd[C:].double()
    xh = (x64 - mu) * rs
    db, dg = g64.sum(0), (g64 * xh).sum(0)
    db_m, dg_m = g64.abs().sum(0), (g64 * xh).abs().sum(0)
    dx = gamma.double() * rs * (g64 - db / M - xh * dg / M)
    dx_m = (gamma.double() * rs).abs() * (g64.abs() + db_m / M + xh.abs() * dg_m / M)
    return dx, dx_m, (db, db_m), (dg, dg_m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [512, 80, 20])
def test_batchnorm_dropout(dev, dtype, C):
    """p = 0.5 (PostNet's dropout): the forward keeps exactly twice the p = 0 outputs; the backward (pass 1 at 4 channels per
    thread, pass 2 at bn_vec) applies the same mask as the forward (8 channels per thread for bf16 at C % 8 == 0)."""
    ops = _ops()
    torch.manual_seed(43)
    M = 700
    x = (torch.randn(M, C) * 2 + 0.5).to(dtype)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    seed = 1234
    o0, mr0 = ops.bn_train_fwd(xd, gd, bd, None, None, ops.ACT_NONE, 0.0, seed)
    o5, mr5 = ops.bn_train_fwd(xd, gd, bd, None, None, ops.ACT_NONE, 0.5, seed)
    assert torch.equal(mr0, mr5)
    o0, o5 = o0.cpu(), o5.cpu()
    keep = o5 != 0
    assert torch.equal(o5[keep], (2 * o0.float()).to(dtype)[keep]), "kept outputs are not exactly twice the p = 0 outputs"
    assert torch.all((o0 == 0) | keep | (o5 == 0))
    frac = keep.float().mean().item()
    assert abs(frac - 0.5) < 0.02
    dout = torch.randn(M, C).to(dtype)
    dx, dgam, dbet = ops.bn_bwd(xd, dout.to(dev), mr5, gd, bd, ops.ACT_NONE, 0.5, seed)
    mask = keep.double() * 2
    rdx, mdx, (rdb, mdb), (rdg, mdg) = _bn_ref_bwd(x.float(), dout.float() * mask, mr5.cpu(), gamma)
    c_sum = M + 4                                              # any association of M terms; xhat (2) and g * xhat (1) rounded
    _rep(f"bn_bwd dbeta p=0.5 {dtype} C={C}", R.check(dbet, rdb, mdb, c_sum, what="bn dbeta"), c_sum)
    _rep(f"bn_bwd dgamma p=0.5 {dtype} C={C}", R.check(dgam, rdg, mdg, c_sum, what="bn dgamma"), c_sum)
    c_dx = c_sum + 8                                           # the sums' error, then 2 divisions, 4 products, 2 subtractions
    _rep(f"bn_bwd dx p=0.5 {dtype} C={C}", R.check(dx, rdx, mdx, c_dx, dtype, what="bn dx"), c_dx)
    # bn_bwd_acc == bn_bwd + the accumulation (the same ordered sums, one fp32 add onto the buffers)
    ws = ops.bn_workspace(C, dev).fill_(float("nan"))
    ig, ib = torch.randn(C), torch.randn(C)
    ag, ab = ig.to(dev), ib.to(dev)
    dx2 = ops.bn_bwd_acc(xd, dout.to(dev), mr5, gd, bd, ops.ACT_NONE, 0.5, seed, ws, ag, ab)
    _eq(dx2, dx, f"bn_bwd_acc dx == bn_bwd dx {dtype} C={C}")
    _eq(ag, ig + dgam.cpu(), f"bn_bwd_acc dgamma {dtype} C={C}")
    _eq(ab, ib + dbet.cpu(), f"bn_bwd_acc dbeta {dtype} C={C}")


def _bn_stat_bounds(x, M):
    """fp64 mean / unbiased variance and bounds for the shifted one-pass sums (shift = row 0): sum = S1 + M sh, ssd = S2 - S1^2/M,
    each sum a chain of at most M additions in any association."""
    x64 = x.double()
    sh = x64[0]
    d = x64 - sh
    mean = x64.mean(0)
    mean_m = (d.abs().sum(0) + M * sh.abs()) / M
    ssd = ((x64 - mean) ** 2).sum(0)
    ssd_m = (d * d).sum(0) + d.sum(0) ** 2 / M
    return mean, mean_m, ssd, ssd_m


@pytest.mark.parametrize("dtype", DTYPES)
def test_batchnorm_persistent_workspace(dev, dtype):
    """the engine's ws= form: one workspace per width, reused by successive layers; NaN-filled before every call, results
    unchanged (every slab word read was written by the same launch); running stats and num_batches_tracked over 4 calls.
    It is held to the same fp64 bounds as the plain form, not to bit-identity with it: the plain form adds the slab rows in four
    interleaved chains (bn_slab_sum_kernel), the ws form in pairwise groups of eight (bn_fix_finalize_kernel)."""
    ops = _ops()
    torch.manual_seed(44)
    for C, M in ((512, 700), (80, 3000)):
        ws = ops.bn_workspace(C, dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        gamma, beta = (torch.rand(C) + 0.5).to(dev), (torch.randn(C) * 0.1).to(dev)
        for k in range(4):
            x = (torch.randn(M, C) * 0.5 + 3.0 * (k - 1)).to(dtype)
            xd = x.to(dev)
            ws.zero_()
            o_z, mr_z = ops.bn_train_fwd(xd, gamma, beta, rm.clone(), rv.clone(), ops.ACT_TANH, 0.0, 0, ws=ws,
                                         num_batches_tracked=nbt.clone())
            ws.fill_(float("nan"))
            o, mr = ops.bn_train_fwd(xd, gamma, beta, rm, rv, ops.ACT_TANH, 0.0, 0, ws=ws, num_batches_tracked=nbt)
            assert torch.equal(o, o_z) and torch.equal(mr, mr_z), "a NaN-filled workspace changed the result"
            assert torch.isfinite(mr).all() and int(nbt.item()) == k + 1
            o_p, mr_p = ops.bn_train_fwd(xd, gamma, beta, None, None, ops.ACT_TANH, 0.0, 0)
            mean, mean_m, ssd, ssd_m = _bn_stat_bounds(x.float(), M)
            for name, mr_ in (("ws", mr), ("plain", mr_p)):
                R.check(mr_[:C], mean, mean_m, M + 4, what=f"bn mean {name}")
                var = ssd / M
                rs_ref = (var + 1e-5).rsqrt()
                rs_lim = rs_ref * (0.5 * (M + 6) * R.U32 * ssd_m / M / (var + 1e-5) + 4 * R.U32)
                assert bool(((mr_[C:].cpu().double() - rs_ref).abs() <= rs_lim).all()), f"bn rstd {name}"
            rm64 = 0.9 * rm64 + 0.1 * mean
            rv64 = 0.9 * rv64 + 0.1 * ssd / (M - 1)
            R.check(rm, rm64, 0.9 * rm64.abs() + 0.1 * mean_m * (M + 8), 4 * (k + 1), what="running_mean")
            R.check(rv, rv64, 0.9 * rv64.abs() + 0.1 * ssd_m / (M - 1) * (M + 8), 4 * (k + 1), what="running_var")
        print(f"[elem] bn ws form {dtype} C={C}: NaN-filled == zero-filled workspace over 4 calls, num_batches_tracked = 4")


def test_batchnorm_acc_alternating_widths(dev):
    """bn_bwd_acc calls of C = 512 and C = 80 alternate on ONE workspace (allowed by its header), NaN-filled in between"""
    ops = _ops()
    torch.manual_seed(45)
    ws = ops.bn_workspace(512, dev)
    cases = {}
    for C, M in ((512, 900), (80, 1300)):
        x = torch.randn(M, C, device=dev)
        gm, bt = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        _, mr = ops.bn_train_fwd(x, gm, bt, None, None, ops.ACT_TANH, 0.0, 0)
        dout = torch.randn(M, C, device=dev)
        dx, dg, db = ops.bn_bwd(x, dout, mr, gm, bt, ops.ACT_TANH, 0.5, 99)
        cases[C] = (x, dout, mr, gm, bt, dx, dg.clone(), db.clone())
    accg = {C: torch.zeros(C, device=dev) for C in cases}
    accb = {C: torch.zeros(C, device=dev) for C in cases}
    for rnd in range(2):
        for C in (512, 80):
            x, dout, mr, gm, bt, dx, dg, db = cases[C]
            ws.fill_(float("nan"))
            dx2 = ops.bn_bwd_acc(x, dout, mr, gm, bt, ops.ACT_TANH, 0.5, 99, ws, accg[C], accb[C])
            assert torch.equal(dx2, dx), (C, rnd)
    for C in cases:
        dg, db = cases[C][6], cases[C][7]
        assert torch.equal(accg[C], dg + dg) and torch.equal(accb[C], db + db)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_deferred_reduce(dev, dtype):
    ops = _ops()
    from fastspeech2_amd import _lib
    torch.manual_seed(46)
    B, S, C = 4, 300, 256
    gamma, beta = (torch.rand(C) + 0.5).to(dev), torch.randn(C).to(dev)
    runs = []
    for k in range(2):
        y = torch.randn(B * S, C).to(dtype).to(dev)
        z = y.clone()
        _, mean, rstd = ops.ln_fwd(z, None, gamma, beta, None, B, S)
        dout = torch.randn(B * S, C).to(dtype).to(dev)
        dg_i, db_i = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        d1_i, _ = ops.ln_bwd(z, dout, gamma, None, mean, rstd, dg_i, db_i, B, S)
        d1, _, ws = ops.ln_bwd(z, dout, gamma, None, mean, rstd, None, None, B, S, defer=True)
        assert torch.equal(d1, d1_i)
        runs.append((z, dout, mean, rstd, ws, dg_i, db_i))
    ig, ib = torch.randn(C), torch.randn(C)
    for z, dout, mean, rstd, ws, dg_i, db_i in runs:       # two deferred reductions outstanding at once
        dg, db = ig.to(dev), ib.to(dev)
        ops.ln_bwd_reduce(ws, C, dg, db)
        xh = (z.cpu().double() - mean.cpu().double().unsqueeze(1)) * rstd.cpu().double().unsqueeze(1)
        g64 = dout.cpu().double()
        c = B * S + 4                                      # any association of B*S terms; xhat (2) and g * xhat (1) rounded
        for name, got, imm, r, m, i0 in (("dgamma", dg, dg_i, (g64 * xh).sum(0), (g64 * xh).abs().sum(0), ig),
                                         ("dbeta", db, db_i, g64.sum(0), g64.abs().sum(0), ib)):
            _rep(f"ln_bwd_reduce {name} {dtype}", R.check(got, r + i0.double(), m + i0.double().abs(), c, what=name), c)
            R.check(imm, r, m, c, what=f"immediate {name}")
    # a zero-row call: the later reduce must leave dgamma / dbeta unchanged (allocated buffers: an empty tensor is a null pointer)
    buf = torch.randn(64 * C, device=dev).to(dtype)
    mr = torch.ones(64, device=dev)
    ws = torch.full((1024 * 2 * C + 4,), float("nan"), device=dev)
    _lib.call("fs2_ln_bwd_sum", buf.data_ptr(), buf.data_ptr(), None, gamma.data_ptr(), None, mr.data_ptr(), mr.data_ptr(), None,
              buf.data_ptr(), None, None, None, ws.data_ptr(), 0, S, C, 0.0, 0, 0.0, 0, None, 0, ops.dt(dtype), ops._stream())
    dg, db = ig.to(dev), ib.to(dev)
    ops.ln_bwd_reduce(ws, C, dg, db)
    assert torch.equal(dg.cpu(), ig) and torch.equal(db.cpu(), ib)


def test_seed_dev_equals_seed_offset(dev):
    """seed_dev holding k draws exactly the masks of seed + k (LayerNorm forward / backward, BatchNorm apply / backward)"""
    ops = _ops()
    torch.manual_seed(47)
    k = 0x1234567890
    kd = torch.tensor([k], dtype=torch.int64, device=dev)
    B, S, C = 2, 50, 256
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    for dtype in DTYPES:
        y = torch.randn(B * S, C, device=dev).to(dtype)
        za, zb = y.clone(), y.clone()
        oa, ma, ra = ops.ln_fwd(za, None, gamma, beta, None, B, S, p_pre=0.3, seed_pre=17 + k, p_post=0.2, seed_post=5 + k)
        ob, mb, rb = ops.ln_fwd(zb, None, gamma, beta, None, B, S, p_pre=0.3, seed_pre=17, p_post=0.2, seed_post=5, seed_dev=kd)
        assert torch.equal(za, zb) and torch.equal(oa, ob) and torch.equal(ma, mb)
        dout = torch.randn(B * S, C, device=dev).to(dtype)
        da = ops.ln_bwd(za, dout, gamma, None, ma, ra, None, None, B, S, want_d2=True, p_pre=0.3, seed_pre=17 + k, p_post=0.2,
                        seed_post=5 + k, defer=True)
        db = ops.ln_bwd(zb, dout, gamma, None, mb, rb, None, None, B, S, want_d2=True, p_pre=0.3, seed_pre=17, p_post=0.2,
                        seed_post=5, seed_dev=kd, defer=True)
        assert torch.equal(da[0], db[0]) and torch.equal(da[1], db[1])
        x = torch.randn(600, 80, device=dev).to(dtype)
        g8, b8 = torch.rand(80, device=dev) + 0.5, torch.randn(80, device=dev)
        oa, mra = ops.bn_train_fwd(x, g8, b8, None, None, ops.ACT_TANH, 0.5, 77 + k)
        ob, mrb = ops.bn_train_fwd(x, g8, b8, None, None, ops.ACT_TANH, 0.5, 77, seed_dev=kd)
        assert torch.equal(oa, ob)
        d = torch.randn(600, 80, device=dev).to(dtype)
        xa = ops.bn_bwd(x, d, mra, g8, b8, ops.ACT_TANH, 0.5, 77 + k)
        xb = ops.bn_bwd(x, d, mra, g8, b8, ops.ACT_TANH, 0.5, 77, seed_dev=kd)
        assert all(torch.equal(a, b) for a, b in zip(xa, xb))
