"""tests/elem_ref.py on the CPU: its references agree with the reference model's own torch formulation, each bound accepts a CPU
emulation of the kernel's fp32 summation order, and each bound rejects the same sum with one term dropped."""
import math

import torch
import torch.nn.functional as F

from tests import elem_ref as R


def _chain32(init, terms):
    """init + terms[0] + terms[1] + ... as a sequential fp32 chain (one rounding per addition), like an atomic or a loop"""
    acc = init.to(torch.float32).clone()
    for t in terms:
        acc = acc + t.to(torch.float32)
    return acc


# ------------------------------------------------------------------------------------------------- agreement with torch
def test_gathers_agree_with_torch():
    torch.manual_seed(1)
    V, C, B, L = 40, 80, 3, 11
    tok = torch.randint(0, V, (B, L))
    emb, pe = torch.randn(V, C), torch.randn(20, C)
    ref = F.embedding(tok, emb) + pe[:L]
    assert torch.equal(R.embed_pe(tok, emb, pe, torch.float32), ref.reshape(B * L, C))
    assert torch.equal(R.embed_pe(tok, emb, pe, torch.bfloat16), ref.reshape(B * L, C).bfloat16())
    bins = torch.linspace(-1, 1, 9)
    v = torch.tensor([-2.0, -1.0, 0.0, 0.25, 1.0, 3.0, float("inf"), float("-inf"), float("nan")])
    plain = [sum(1 for b in bins.tolist() if b < x) if not math.isnan(x) else len(bins) for x in v.tolist()]
    assert R.bucketize(v, 1.0, bins).tolist() == plain           # NaN -> len(bins), as torch.bucketize
    assert int(torch.bucketize(torch.tensor([float("nan")]), torch.tensor([0.0, 1.0, 2.0]))) == 3


def test_rne_bf16_ties_and_specials():
    f = torch.tensor([0x3F808000, 0x3F818000, 0x7F7F7FFF, 0x7F7F8000], dtype=torch.int64).to(torch.int32).view(torch.float32)
    got = R.bits(R.rne_bf16(f)).tolist()
    assert got == [0x3F80, 0x3F82, 0x7F7F, 0x7F80]               # tie down to even, tie up to even, largest finite, -> inf


def test_adam_reference_matches_torch_optim():
    torch.manual_seed(2)
    n = 4000
    p, g = torch.randn(n), torch.randn(n) * 3
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    m, v = torch.zeros(n), torch.zeros(n)
    pc = p.clone()
    for step in (1, 2, 3):
        pr.grad = g * step
        gsq = float((g.double() * step) ** 2 @ torch.ones(n, dtype=torch.float64))
        torch.nn.utils.clip_grad_norm_([pr], 1.0)
        opt.step()
        hyper = torch.tensor([1e-3, 1 - 0.9 ** step, 1 - 0.98 ** step])
        ref = R.adam(pc, g * step, m, v, gsq, 1.0, hyper, 0.9, 0.98, 1e-9, 0.0)
        pc, m, v = ref["p"][0].float(), ref["m"][0].float(), ref["v"][0].float()
    assert torch.allclose(pc, pr.detach(), rtol=0, atol=2e-6)


def _loss_inputs(p_frame):
    torch.manual_seed(3)
    B, T, L, n_mel = 4, 30, 9, 8
    mel_lens, src_lens = torch.tensor([30, 12, 41, 5]), torch.tensor([9, 3, 12, 1])
    mel, post = torch.randn(B, T, n_mel), torch.randn(B, T, n_mel)
    mel_t = torch.randn(B, T + 3, n_mel)
    Pn = T if p_frame else L
    En = L if p_frame else T
    return (mel, post, mel_t, mel_lens, src_lens, torch.randn(B, Pn), torch.randn(B, Pn + 2), torch.randn(B, En),
            torch.randn(B, En + 1), torch.randn(B, L), torch.randint(0, 7, (B, L)), p_frame, 1 - p_frame)


def test_loss_reference_matches_oracle():
    from oracle.fs2_oracle import fastspeech2_loss, mask_from_lengths
    for p_frame in (0, 1):
        mel, post, mel_t, ml, sl, pp, pt, ep, et, logd, dur, pf, ef = _loss_inputs(p_frame)
        B, T, _ = mel.shape
        L = logd.shape[1]
        terms, ns, nm = R.loss_terms(mel, post, mel_t, ml, sl, pp, pt, ep, et, logd, dur, pf, ef)
        feat = lambda f: {"feature": "frame_level" if f else "phoneme_level"}          # noqa: E731
        pcfg = {"preprocessing": {"pitch": feat(pf), "energy": feat(ef)}}
        sm, mm = mask_from_lengths(sl.clamp(max=L), L), mask_from_lengths(ml.clamp(max=T), T)
        preds = (mel, post, pp, ep, logd, None, sm, mm, None, None)
        Pn, En = pp.shape[1], ep.shape[1]
        o = fastspeech2_loss(pcfg, (mel_t, pt[:, :Pn], et[:, :En], dur), preds)
        den = dict(mel=nm * mel.shape[2], post=nm * mel.shape[2], pitch=nm if pf else ns, energy=nm if ef else ns, duration=ns)
        for k, name in enumerate(["mel", "post", "pitch", "energy", "duration"]):
            assert abs(float(terms[name][0]) / den[name] - float(o[k + 1])) <= 1e-5 * (1 + abs(float(o[k + 1]))), name


# ------------------------------------------------------------------------------- bounds: accept the kernel order, reject a drop
def test_embed_and_rowvec_bounds():
    torch.manual_seed(4)
    V, C, rows = 6, 16, 300
    tok = torch.randint(-1, V + 1, (rows,))
    tok[:120] = 2                                               # a heavily repeated id
    dy = torch.randn(rows, C).bfloat16()
    init = torch.randn(V, C)
    ref, mag, c = R.embed_bwd(tok, dy, V, 0, init)
    emu = init.clone()
    order = torch.randperm(rows)                                # atomics land in any order
    for r in order.tolist():
        t = int(tok[r])
        if 0 <= t < V and t != 0:
            emu[t] = emu[t] + dy[r].float()
    assert R.within(emu, ref, mag, c)
    emu[2] -= dy[int((tok == 2).nonzero()[5])].float()          # one row lost
    assert not R.within(emu, ref, mag, c)
    B, S = 5, 400
    idx = torch.tensor([1, 1, 3, 9, 1])
    dy = torch.randn(B * S, C)
    init = torch.randn(V, C)
    ref, mag, c = R.rowvec_bwd(dy, idx, B, S, V, init)
    emu = init.clone()
    for b in range(B):
        s = _chain32(torch.zeros(C), dy.view(B, S, C)[b])
        emu[int(R.valid_ids(idx, V)[b])] += s
    assert R.within(emu, ref, mag, c)
    emu[1] -= dy[S + 7]                                          # one frame lost
    assert not R.within(emu, ref, mag, c)


def test_bucket_and_lr_bounds():
    torch.manual_seed(5)
    nb, C, rows = 8, 8, 2500
    idx = torch.randint(0, 6, (rows,), dtype=torch.int32)
    idx[:300] = 4
    dy = torch.randn(rows, C)
    init = torch.randn(nb, C)
    ref, mag, c = R.bucket_embed_bwd(idx, dy, nb, init)
    emu = init.clone()
    for s0 in range(0, rows, R.BUCKET_RPS):                     # the kernel's order: 4 lanes, wave partials, one add per split
        for b in range(nb):
            lanes = [torch.zeros(C) for _ in range(4)]
            for k0 in range(s0, min(rows, s0 + R.BUCKET_RPS), 256):
                hit = [r for r in range(k0, min(rows, k0 + 256, s0 + R.BUCKET_RPS)) if int(idx[r]) == b]
                for j, r in enumerate(hit):
                    lanes[j % 4] = lanes[j % 4] + dy[r]
            if any(int(idx[r]) == b for r in range(s0, min(rows, s0 + R.BUCKET_RPS))):
                t = lanes[0]
                for q in (1, 2, 3):
                    t = t + lanes[q]
                emu[b] = emu[b] + t
    assert R.within(emu, ref, mag, c)
    emu[4] -= dy[299]                                           # the last row of a chunk skipped
    assert not R.within(emu, ref, mag, c)
    B, L, T = 2, 7, 20
    dur = torch.tensor([[3, 0, 5, 2, 4, 1, 6], [0, 0, 1, 9, 0, 2, 2]])
    cum = torch.cat([torch.zeros(B, 1, dtype=torch.long), dur.cumsum(1)], 1)
    dy = torch.randn(B * T, C).bfloat16()
    ref, mag, c = R.lr_gather_bwd(dy, cum, B, L, T)
    emu = torch.zeros(B * L, C)
    for b in range(B):
        for i in range(L):
            t0, t1 = min(int(cum[b, i]), T), min(int(cum[b, i + 1]), T)
            emu[b * L + i] = _chain32(torch.zeros(C), dy[b * T + t0:b * T + t1])
    emu = emu.bfloat16()
    assert R.within(emu, ref, mag, c, torch.bfloat16)
    drop = emu.float().clone()
    drop[3] -= dy[int(cum[0, 3]) + 1].float()
    assert not R.within(drop.bfloat16(), ref, mag, c, torch.bfloat16)


def test_rowdot_and_sumsq_bounds():
    torch.manual_seed(6)
    B, S, C = 3, 700, 32
    x = torch.randn(B * S, C).bfloat16()
    w, g = torch.randn(C), torch.randn(B, S)
    lens = torch.tensor([700, 0, 233])
    dw0, db0 = torch.randn(C), torch.randn(1)
    dx, (rdw, mdw), _, c = R.rowdot_bwd(x, w, g, lens, B, S, dw0, db0)
    gm = torch.where(R.padding(lens, B, S), torch.zeros(()), g).reshape(-1)
    grid = 512
    emu = dw0.clone()
    for blk in range(grid):                                     # per-block chains over rows blk, blk + 512, ... then one atomic each
        acc = torch.zeros(C)
        for r in range(blk, B * S, grid):
            acc = acc + gm[r] * x[r].float()
        emu = emu + acc
    assert R.within(emu, rdw, mdw, c)
    emu2 = emu - gm[5] * x[5].float()
    assert not R.within(emu2, rdw, mdw, c)
    n = 70001
    xs = torch.randn(n)
    ref, mag, c = R.sumsq(xs, 0.5)
    emu = torch.tensor(0.5)
    for k0 in range(0, n, 1000):                                # a chain of partial sums, like the per-block partials
        emu = emu + (xs[k0:k0 + 1000] * xs[k0:k0 + 1000]).sum()
    assert R.within(emu.view(1), torch.tensor([ref], dtype=R.F64), torch.tensor([mag], dtype=R.F64), c)
    bad = emu - xs.abs().max() ** 2                             # the largest square lost
    assert not R.within(bad.view(1), torch.tensor([ref], dtype=R.F64), torch.tensor([mag], dtype=R.F64), c)


def test_adam_bound_accepts_fp32_and_rejects_a_lost_update():
    torch.manual_seed(7)
    n = 5000
    p, g, m, v = torch.randn(n), torch.randn(n) * 1e-3, torch.randn(n) * 1e-3, torch.rand(n) * 1e-6
    hyper = torch.tensor([1e-3, 1 - 0.9 ** 3, 1 - 0.98 ** 3])
    ref = R.adam(p, g, m, v, 1e4, 1.0, hyper, 0.9, 0.98, 1e-9, 0.01)
    # the kernel's arithmetic in fp32
    b1, b2 = torch.tensor(0.9), torch.tensor(0.98)
    coef = torch.clamp(torch.tensor(1.0) / (torch.tensor(1e4).sqrt() + torch.tensor(1e-6)), max=1.0)
    gi = g * coef + torch.tensor(0.01) * p
    m1 = b1 * m + (1 - b1) * gi
    v1 = b2 * v + (1 - b2) * gi * gi
    denom = v1.sqrt() * torch.rsqrt(hyper[2]) + torch.tensor(1e-9)
    p1 = p - (hyper[0] / hyper[1]) * (m1 / denom)
    for name, got in (("m", m1), ("v", v1)):
        r, mag, c = ref[name]
        assert R.within(got, r, mag, c), name
    r, mag, c = ref["p"]
    ok = lambda q: bool(((q.double() - r).abs() <= c * R.U32 * mag + R.U32 * r.abs()).all())   # noqa: E731
    assert ok(p1)
    p_bad = p1.clone()
    p_bad[17] = p[17]                                           # one element not updated
    assert not ok(p_bad)
