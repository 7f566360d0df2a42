"""fp64 references and per-element bounds for the memory-bound and reducing kernels of the train step: gathers, casts, the
loss, the optimiser and the affine-gradient sums (fs2_elem.hip, fs2_loss.hip, fs2_optim.hip, fs2_norm.hip).

Two kinds of check, both elementwise and never normalised by a maximum or a norm:
  * a kernel that is ONE correctly rounded fp32 operation (a gather plus one add, a cast, a masked store) must be bit-exact:
    the reference is the same fp32 operation on the CPU, rounded to bf16 with round-to-nearest-even where the output is bf16;
  * a reduction is bounded by  |got - ref| <= c * u * mag  (+ one bf16 rounding of the result where it is stored as bf16),
    with u = 2^-24, `ref` the exact (fp64) sum of the values the kernel read and `mag` the same sum over absolute values.
    c is the length of the kernel's longest chain of dependent fp32 additions onto one output, read from the code:
    a chain of k roundings moves a sum by at most k * u * (sum of the magnitudes it carried).  A product that is rounded
    before it is added (bf16 x fp32 operands) adds one more u.

Every c below is derived, not fitted; tests/test_elem_gpu.py prints the observed maxima of err / (u mag).  On the MI355X
(beyond the bf16 output rounding, both dtypes): embed_bwd 2.39, rowvec_bwd 1.86, rowdot_fwd 1.43, rowdot_bwd dw 2.37 / db 0.59,
bucket_embed_bwd 2.11, lr_gather_bwd 2.44, sumsq 0.55, loss_fwd 7.27 (c >= 62), Adam m 2.55 / v 3.94 / p 3.18,
BatchNorm dbeta 0.35 / dgamma 0.41 / dx 2.79, LayerNorm deferred dgamma 0.42 / dbeta 0.35.
"""
import math

import torch

U32 = 2.0 ** -24            # unit roundoff of fp32
U_BF16 = 2.0 ** -8          # unit roundoff of bf16 (8-bit significand, round-to-nearest-even)
F64 = torch.float64


def rne_bf16(x):
    """fp32 -> bf16 round-to-nearest-even on the CPU (NaN stays NaN)"""
    return x.float().cpu().to(torch.bfloat16)


def store(x32, dtype):
    """an fp32 CPU result as the kernel stores it"""
    return x32 if dtype == torch.float32 else rne_bf16(x32)


def bits(x):
    """the bit patterns of a CPU tensor, for exact comparison that treats equal NaNs and -0 / +0 as they are"""
    x = x.cpu().contiguous()
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- bounds
def allowed(ref, mag, c, out_dtype=torch.float32):
    """the per-element bound c * u * mag, plus the one bf16 rounding of the stored result"""
    ref, mag = ref.to(F64), mag.to(F64)
    c = torch.as_tensor(c, dtype=F64)
    a = c * U32 * mag
    if out_dtype == torch.bfloat16:
        a = a + U_BF16 * (ref.abs() + a)
    return a


def check(got, ref, mag, c, out_dtype=torch.float32, what=""):
    """assert |got - ref| <= allowed(...) everywhere; returns the largest err / (u mag) (0 where mag == 0) for the record"""
    got = got.detach().cpu().to(F64)
    ref, mag = ref.cpu().to(F64), mag.cpu().to(F64)
    err = (got - ref).abs()
    lim = allowed(ref, mag, torch.as_tensor(c, dtype=F64).cpu(), out_dtype)
    bad = ~(err <= lim)
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first #{i}: got "
                             f"{got.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} lim "
                             f"{lim.reshape(-1)[i].item():.3g}")
    return ratio(got, ref, mag, out_dtype)


def within(got, ref, mag, c, out_dtype=torch.float32):
    got = got.detach().cpu().to(F64)
    return bool(((got - ref.to(F64)).abs() <= allowed(ref, mag, c, out_dtype)).all())


def ratio(got, ref, mag, out_dtype=torch.float32):
    """max err / (u mag); for a bf16 result, the error beyond its own output rounding (U_BF16 |ref|)"""
    err = (got.detach().cpu().to(F64) - ref.cpu().to(F64)).abs()
    if out_dtype == torch.bfloat16:
        err = (err - U_BF16 * ref.cpu().to(F64).abs()).clamp_min(0)
    mag = mag.cpu().to(F64)
    r = torch.where(mag > 0, err / (U32 * mag.clamp_min(1e-300)), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------- gathers (bit-exact)
def valid_ids(tok, V):
    """out-of-range ids read row 0 (embed_pe_kernel, add_rowvec_kernel)"""
    t = tok.long().cpu()
    return torch.where((t < 0) | (t >= V), torch.zeros_like(t), t)


def embed_pe(tok, emb, pe, dtype):
    B, L = tok.shape
    e = emb.cpu().float()[valid_ids(tok, emb.shape[0])]
    return store((e + pe.cpu().float()[:L].unsqueeze(0)).reshape(B * L, -1), dtype)


def add_rowvec(x, table, idx, B, S):
    rows = table.cpu().float()[valid_ids(idx, table.shape[0])]
    x32 = x.cpu().float().view(B, S, -1)
    return store((x32 + rows.unsqueeze(1)).reshape(B * S, -1), x.dtype)


def bucketize(vals, scale, bins):
    """torch.bucketize(right=False) of the fp32 product vals * scale, as the reference's pitch / energy embedding"""
    v = vals.cpu().float() * torch.tensor(scale, dtype=torch.float32)
    return torch.bucketize(v, bins.cpu().float())


def lr_gather(x, idx, pe, B, L, T):
    """out[b, t] = (idx >= 0 ? x[b, idx] : 0) (+ pe[t]) in fp32, stored in x's dtype"""
    C = x.shape[-1]
    xs = x.cpu().float().view(B, L, C)
    ix = idx.cpu().long().view(B, T)
    g = torch.gather(xs, 1, ix.clamp_min(0).unsqueeze(-1).expand(B, T, C))
    g = torch.where((ix >= 0).unsqueeze(-1), g, torch.zeros(()))
    if pe is not None:
        g = g + pe.cpu().float()[:T].unsqueeze(0)
    return store(g.reshape(B * T, C), x.dtype)


# ------------------------------------------------------------------------------------------------------------- reductions
def embed_bwd(tok, dy, V, pad_idx, init):
    """demb = init + sum of dy rows per id; ids out of range and pad_idx add nothing.  One fp32 atomic per row and channel:
    the chain onto demb[id] is (number of rows with that id) additions, in any order."""
    t = tok.reshape(-1).long().cpu()
    d = dy.cpu().to(F64)
    keep = (t >= 0) & (t < V) & (t != pad_idx)
    ref = init.cpu().to(F64).clone().index_add_(0, t[keep], d[keep])
    mag = init.cpu().to(F64).abs().index_add_(0, t[keep], d[keep].abs())
    cnt = torch.zeros(V, dtype=F64).index_add_(0, t[keep], torch.ones(int(keep.sum()), dtype=F64))
    return ref, mag, cnt.unsqueeze(1)


def rowvec_bwd(dy, idx, B, S, V, init):
    """dtable[id] = init + sum over the sequences b with that id of sum_t dy[b, t].  rowvec_bwd_kernel: a sequential fp32 sum
    over the S rows (S - 1 additions) then one atomic per sequence: chain = S - 1 + (sequences sharing the id)."""
    ids = valid_ids(idx, V)
    per_seq = dy.cpu().to(F64).view(B, S, -1)
    ref = init.cpu().to(F64).clone().index_add_(0, ids, per_seq.sum(1))
    mag = init.cpu().to(F64).abs().index_add_(0, ids, per_seq.abs().sum(1))
    share = torch.zeros(V, dtype=F64).index_add_(0, ids, torch.ones(B, dtype=F64))
    return ref, mag, (S - 1 + share).unsqueeze(1)


BUCKET_RPS = 1024            # rows per split of bucket_embed_bwd_kernel


def bucket_embed_bwd(idx, dy, nb, init):
    """demb[bin] = init + sum of the dy rows in that bin.  bucket_embed_bwd_kernel: per split of 1024 rows the 4 waves take
    every 4th matching row of each 256-row chunk (sum over chunks of ceil(n/4), minus 1, additions per lane), the 4 wave
    partials meet in 3 additions, and one atomic per (bin, split that saw a match) adds onto demb:
    chain = max_split sum_chunks ceil(n/4) + 2 + (splits with a match)."""
    i = idx.reshape(-1).long().cpu()
    d = dy.cpu().to(F64)
    ref = init.cpu().to(F64).clone().index_add_(0, i, d)
    mag = init.cpu().to(F64).abs().index_add_(0, i, d.abs())
    rows = i.numel()
    c = torch.zeros(nb, dtype=F64)
    per = torch.zeros(nb, dtype=F64)
    hits = torch.zeros(nb, dtype=F64)
    for s0 in range(0, rows, BUCKET_RPS):
        lane = torch.zeros(nb, dtype=F64)
        for k0 in range(s0, min(rows, s0 + BUCKET_RPS), 256):      # a wave's share of each 256-row chunk's matches
            lane += torch.ceil(torch.bincount(i[k0:min(rows, s0 + BUCKET_RPS, k0 + 256)], minlength=nb).to(F64) / 4)
        per = torch.maximum(per, lane)
        hits += (lane > 0).to(F64)
    c = torch.where(hits > 0, per + 2 + hits, torch.zeros(nb, dtype=F64))
    return ref, mag, c.unsqueeze(1)


def lr_gather_bwd(dy, cum, B, L, T, init=None):
    """dx[b, i] = (init) + sum_{t = cum[i]}^{min(cum[i+1], T) - 1} dy[b, t]: a sequential fp32 chain of that many additions
    (plus one when accumulating), the result stored in dy's dtype."""
    C = dy.shape[-1]
    d = dy.cpu().to(F64).view(B, T, C)
    cu = cum.cpu().long().view(B, L + 1).clamp(max=T)
    ref = torch.zeros(B, L, C, dtype=F64)
    mag = torch.zeros(B, L, C, dtype=F64)
    n = torch.zeros(B, L, 1, dtype=F64)
    for b in range(B):
        cs = torch.cat([torch.zeros(1, C, dtype=F64), d[b].cumsum(0)])
        ca = torch.cat([torch.zeros(1, C, dtype=F64), d[b].abs().cumsum(0)])
        t0, t1 = cu[b, :-1], cu[b, 1:]
        ref[b] = cs[t1] - cs[t0]
        mag[b] = ca[t1] - ca[t0]
        n[b, :, 0] = (t1 - t0).to(F64)
    ref, mag = ref.reshape(B * L, C), mag.reshape(B * L, C)
    c = n.reshape(B * L, 1)                      # from 0 the first addition is exact; onto `init` it is not
    if init is not None:
        ref = ref + init.cpu().to(F64)
        mag = mag + init.cpu().to(F64).abs()
    else:
        c = (c - 1).clamp(min=0)
    return ref, mag, c


def rowdot_fwd(x, w, bias, lens, B, S):
    """out[r] = x[r] . w + b on rows t < len, exact 0 on padded rows.  rowdot_fwd_kernel: per lane ceil(C/256) float4 steps
    of 4 products (4 additions each, one rounded product per term), a 6-level wave tree, + bias:
    c = 4 ceil(C/256) + 1 + 6 + 1."""
    C = x.shape[-1]
    xs, w64 = x.cpu().to(F64), w.cpu().to(F64)
    ref = xs @ w64 + float(bias.reshape(-1)[0])
    mag = xs.abs() @ w64.abs() + abs(float(bias.reshape(-1)[0]))
    pad = padding(lens, B, S).reshape(-1)
    ref = torch.where(pad, torch.zeros_like(ref), ref)
    mag = torch.where(pad, torch.zeros_like(mag), mag)
    return ref, mag, 4 * math.ceil(C / 256) + 8


def padding(lens, B, S):
    """True on rows t >= len (a None lens pads nothing)"""
    if lens is None:
        return torch.zeros(B, S, dtype=torch.bool)
    return torch.arange(S).unsqueeze(0) >= lens.cpu().long().view(B, 1)


def rowdot_bwd(x, w, g, lens, B, S, dw0, db0):
    """dx = bf16/fp32 store of the fp32 product gm * w (bit-exact); dw = dw0 + sum_r gm[r] x[r]; db = db0 + sum_r gm[r],
    gm = g masked.  rowdot_bwd_kernel: min(rows, 512) blocks, each a sequential chain over its ceil(rows / grid) rows (one
    rounded product per term), then one atomic per block: c = ceil(rows / grid) + 1 + grid."""
    rows = B * S
    gm = torch.where(padding(lens, B, S), torch.zeros(()), g.cpu().float().view(B, S)).reshape(rows)
    dx = store(gm.unsqueeze(1) * w.cpu().float().unsqueeze(0), x.dtype)
    xs = x.cpu().to(F64)
    g64 = gm.to(F64)
    dw = dw0.cpu().to(F64) + g64 @ xs
    dw_mag = dw0.cpu().to(F64).abs() + g64.abs() @ xs.abs()
    db = db0.cpu().to(F64) + g64.sum()
    db_mag = db0.cpu().to(F64).abs() + g64.abs().sum()
    grid = min(rows, 512)
    c = math.ceil(rows / grid) + 1 + grid
    return dx, (dw, dw_mag), (db, db_mag), c


SUMSQ_BLOCKS = 1024


def sumsq(x, out0):
    """out = out0 + sum x^2.  fs2_sumsq: each of min(ceil(n/1024), 1024) blocks runs a per-thread chain of 4 rounded squares per
    float4 (the block-0 scalar tail adds up to 3 more), a 6-level wave tree and 2 more additions; the final block does the same
    over the partials and adds to out: c = 4 it + 4 + 1 + 8 + ceil(blocks / 256) + 8 + 1."""
    n = x.numel()
    x64 = x.cpu().to(F64)
    ref = float(out0) + float((x64 * x64).sum())
    mag = abs(float(out0)) + float((x64 * x64).sum())
    blocks = max(1, min(SUMSQ_BLOCKS, (n // 4 + 255) // 256))
    it = math.ceil((n // 4) / (blocks * 256))
    c = 4 * it + 4 + 1 + 8 + math.ceil(blocks / 256) + 8 + 1
    return ref, mag, c


# -------------------------------------------------------------------------------------------------------------------- Adam
def adam(p, g, m, v, gnorm_sq, max_norm, hyper, b1, b2, eps, wd):
    """fp64 restatement of adam_kernel (torch.optim.Adam after clip_grad_norm_), with the fp32 values of every scalar the kernel
    reads, and per-element bounds from the operation count:
        coef  = min(1, max_norm / (sqrt(gnorm_sq) + 1e-6))             sqrt, add, divide          -> 3 u relative
        gi    = g coef (+ wd p)                                        1 (+2)                      -> 6 u relative on mag_g
        m'    = b1 m + (1 - b1) gi                                     (1 - b1 exact) 2 products, 1 add
        v'    = b2 v + (1 - b2) gi^2                                   gi^2 carries 2 x 6 u
        denom = sqrt(v') rbc2 + eps,  rbc2 = rsqrtf(bc2)               rsqrtf: 1 ulp = 2 u; sqrt 1; product 1; add 1
        p'    = p - (lr / bc1) (m' / denom)                            3 more roundings, then the subtraction
    Returns (ref, mag, c) for m', v', p'.  The update's magnitude carries m's (m' may cancel): mag_p = (lr / bc1) mag_m / denom,
    and p' is bounded by c_p u mag_p + u |p'| (the final subtraction)."""
    f = lambda t: torch.as_tensor(t).cpu().to(torch.float32).to(F64)    # noqa: E731  (the fp32 value the kernel reads)
    p64, g64, m64, v64 = f(p), f(g), f(m), f(v)
    b1, b2, eps, wd = (float(torch.tensor(s, dtype=torch.float32)) for s in (b1, b2, eps, wd))
    lr, bc1, bc2 = (float(s) for s in f(hyper)[:3])
    coef = 1.0
    if gnorm_sq is not None and max_norm > 0:
        coef = min(1.0, float(torch.tensor(max_norm, dtype=torch.float32)) / (math.sqrt(float(gnorm_sq)) + float(torch.tensor(1e-6, dtype=torch.float32))))
    gi = g64 * coef + wd * p64
    gi_mag = (g64 * coef).abs() + abs(wd) * p64.abs()
    m1 = b1 * m64 + (1 - b1) * gi
    m_mag = b1 * m64.abs() + (1 - b1) * gi_mag
    v1 = b2 * v64 + (1 - b2) * gi * gi
    v_mag = b2 * v64.abs() + (1 - b2) * gi_mag * gi_mag
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (lr / bc1) * (m1 / denom)
    p1 = p64 - upd
    # m': 6 (gi) + 1 (product) + 1 (add) ; v': 2 x 6 (gi^2) + 1 + 1 + 1 ; update: m' 8 + v' 15 / 2 + sqrt 1 + rsqrtf 2 + 1 + 1
    # (eps add) + divide 1 + step 1 + product 1 ~ 24
    return dict(m=(m1, m_mag, 8), v=(v1, v_mag, 15), p=(p1, (lr / bc1) * m_mag / denom, 24))


# -------------------------------------------------------------------------------------------------------------------- loss
def loss_terms(mel, post, mel_t, mel_lens, src_lens, p_pred, p_t, e_pred, e_t, logd, dur, p_frame, e_frame):
    """fp64 sums of the five loss terms over valid positions (t < min(len, T)), their magnitudes and the valid counts.
    Returns {name: (sum, mag, n_terms)} for mel, post, pitch, energy, duration."""
    B, T, n_mel = mel.shape
    L = logd.shape[1]
    ml = mel_lens.cpu().long().clamp(max=T)
    sl = src_lens.cpu().long().clamp(max=L)
    fm = torch.arange(T).unsqueeze(0) < ml.unsqueeze(1)
    fs = torch.arange(L).unsqueeze(0) < sl.unsqueeze(1)
    d64 = lambda t: t.detach().cpu().to(F64)          # noqa: E731
    mt = d64(mel_t[:, :T])
    z = torch.zeros((), dtype=F64)
    am = torch.where(fm.unsqueeze(-1), (d64(mel) - mt).abs(), z)          # (padding may hold NaN: select, never multiply)
    ap = torch.where(fm.unsqueeze(-1), (d64(post) - mt).abs(), z)
    out = dict(mel=(am.sum(), am.sum(), am.numel()), post=(ap.sum(), ap.sum(), ap.numel()))
    for name, pr, tg, frame in (("pitch", p_pred, p_t, p_frame), ("energy", e_pred, e_t, e_frame)):
        msk = fm if frame else fs
        n = pr.shape[1]
        dd = torch.where(msk, (d64(pr) - d64(tg[:, :n])) ** 2, z)
        out[name] = (dd.sum(), dd.sum(), n)
    ld = torch.log(dur.cpu().to(torch.float32) + 1).to(F64)          # the reference's target: log in fp32 (loss.py:40)
    dd = torch.where(fs, (d64(logd) - ld[:, :L]) ** 2, z)
    out["duration"] = (dd.sum(), dd.sum(), L)
    return out, int(fs.sum()), int(fm.sum())
