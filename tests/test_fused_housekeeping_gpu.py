"""The entry points that took over the train step's cast / add / clear launches, each against the composition it replaced
(old kernel + cast / add / zero_).  Everything here must be BIT-IDENTICAL (torch.equal) for both compute dtypes: the new kernels
do the same fp32 arithmetic and round to the storage type at the same places, so there is no tolerance to choose.

The one place where the composition itself is not reproducible is the loss forward: its five sums are float atomics over the
workgroups, so two runs of the SAME kernel can differ in the last bit.  `test_loss_fwd_ws_equals_cleared` therefore feeds it
values whose partial sums are all exactly representable in fp32 (multiples of 1/4 of bounded size, durations 0 so that
log(d + 1) = 0): every summation order then gives the same bits, and bit identity is required there too."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from fastspeech2_amd import ops
    return ops


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
    # compare the bit patterns (NaN-safe, distinguishes -0 from +0)
    ia = a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32)
    ib = b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)
    n = int((ia != ib).sum())
    assert n == 0, f"{what}: {n} of {ia.numel()} elements differ"


# ------------------------------------------------------------------------------------------------- PostNet's last apply pass
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,act,p,with_res", [(80, 0, 0.0, True), (80, 0, 0.5, True), (512, 2, 0.5, False), (84, 2, 0.0, True)])
def test_bn_apply_out32_equals_apply_then_cast(dev, dtype, C, act, p, with_res):
    ops = _ops()
    torch.manual_seed(11)
    M = 3 * 301 + 5                                             # not a multiple of any row-group size
    x = (torch.randn(M, C) * 2).to(dtype).to(dev)
    res = torch.randn(M, C).to(dtype).to(dev) if with_res else None
    mean_rstd = torch.cat([torch.randn(C) * 0.1, torch.rand(C) + 0.5]).to(dev)
    gamma, beta = (torch.rand(C) + 0.5).to(dev), (torch.randn(C) * 0.1).to(dev)
    seed = 0x1234567
    old = torch.empty_like(x)
    ops._lib.call("fs2_bn_apply", x.data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                  res.data_ptr() if res is not None else None, old.data_ptr(), M, C, act, p, seed, None, ops.dt(x), ops._stream())
    old32 = old if dtype == torch.float32 else ops.cast(old, torch.float32)
    out, out32, res32 = ops.bn_apply_out32(x, mean_rstd, gamma, beta, res, act, p, seed, want_out=True)
    _same(out, old, "compute-dtype result")
    _same(out32, old32.view(M, C), "fp32 image of the result")
    if with_res:
        _same(res32, res.float(), "fp32 image of the residual operand")
    else:
        assert res32 is None
    # the form the engine uses: no compute-dtype result at all
    none, only32, _ = ops.bn_apply_out32(x, mean_rstd, gamma, beta, res, act, p, seed, want_out=False)
    assert none is None
    _same(only32, old32.view(M, C), "fp32 image, no compute-dtype store")


# ------------------------------------------------------------------------------------------------- length regulator backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("T", [64, 23])                         # 23 < the longest expansion: the decoder saw truncated sequences
def test_lr_gather_bwd_add_equals_gather_then_adds(dev, dtype, two, T):
    ops = _ops()
    torch.manual_seed(12)
    B, L, C = 4, 9, 256
    dur = torch.randint(0, 8, (B, L))
    dur[1, 5:] = 0                                              # ragged: padded phonemes expand to nothing
    dur[2] = 0
    dur[3, 0] = 40                                              # one segment longer than T = 23
    cum, _, _ = ops.lr_index(dur.to(dev), T)
    dy = torch.randn(B * T, C).to(dtype).to(dev)
    a1 = torch.randn(B * L, C).to(dtype).to(dev)
    a2 = torch.randn(B * L, C).to(dtype).to(dev) if two else None
    r0 = ops.lr_gather_bwd(dy, cum, B, L, T)
    r1 = ops.add(r0, a1)
    r2 = ops.add(r1, a2) if two else None
    dx0, dx1, dx2 = ops.lr_gather_bwd_add(dy, cum, a1, a2, B, L, T)
    _same(dx0, r0, "segment sums")
    _same(dx1, r1, "first add")
    if two:
        _same(dx2, r2, "second add")
    else:
        assert dx2 is None


# ------------------------------------------------------------------------------------------------- loss
def _loss_case(dev, p_frame, e_frame, exact=False):
    """ragged lengths, targets longer than the predictions (the decoder truncated: T < T of the targets), strided target views"""
    torch.manual_seed(13)
    B, T, L, n_mel = 5, 37, 11, 80
    mel_lens = torch.tensor([37, 50, 1, 20, 0])                 # one longer than T (clamped), one empty
    src_lens = torch.tensor([11, 11, 1, 6, 0])
    q = (lambda t: (t * 4).round() / 4) if exact else (lambda t: t)
    mel, post = q(torch.randn(B, T, n_mel)), q(torch.randn(B, T, n_mel))
    mel_t = q(torch.randn(B, T + 7, n_mel))
    mel[:, :2] = mel_t[:, :2]                                   # d = 0 -> gradient exactly 0
    Pn, En = (T if p_frame else L), (T if e_frame else L)
    p_pred, e_pred, logd = q(torch.randn(B, Pn)), q(torch.randn(B, En)), q(torch.randn(B, L))
    p_big, e_big = q(torch.randn(B, Pn + 9)), q(torch.randn(B, En + 4))
    dur_big = torch.zeros(B, L + 3, dtype=torch.int64) if exact else torch.randint(0, 9, (B, L + 3))
    cnt = torch.tensor([float(src_lens.clamp(max=L).sum()), float(mel_lens.clamp(max=T).sum())])
    D = lambda t: t.to(dev)                                     # noqa: E731
    return (D(mel), D(post), D(mel_t), D(mel_lens), D(src_lens), D(p_pred), D(p_big)[:, 2:2 + Pn + 5], D(e_pred),
            D(e_big)[:, 1:1 + En + 3], D(logd), D(dur_big)[:, 3:], D(cnt))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p_frame,e_frame", [(False, False), (True, True), (True, False)])
def test_loss_bwd_lp_equals_bwd_then_cast(dev, dtype, p_frame, e_frame):
    ops = _ops()
    args = _loss_case(dev, p_frame, e_frame)
    B, T, n_mel = args[0].shape
    for g6 in ([1.0, 0.3, -0.2, 0.1, 0.7, 0.5], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0, 0.0, -1.5]):
        g = torch.tensor(g6, device=dev)
        old = ops.loss_bwd(*args, g, p_frame, e_frame)
        for drop_zeros in (False, True):                        # a term nobody differentiated arrives as None, not as a zero
            gs = [None if (drop_zeros and v == 0.0) else g[k].clone() for k, v in enumerate(g6)]
            new = ops.loss_bwd_lp(*args, gs, p_frame, e_frame, dtype)
            for k, name in enumerate(("dmel", "dpost")):
                ref = old[k].view(B * T, n_mel)
                ref = ref if dtype == torch.float32 else ops.cast(ref.contiguous(), dtype)
                _same(new[k], ref, f"{name} g={g6} none={drop_zeros}")
            for k, name in ((2, "dp"), (3, "de"), (4, "dlogd")):
                _same(new[k], old[k], f"{name} g={g6} none={drop_zeros}")


@pytest.mark.parametrize("p_frame,e_frame", [(False, False), (True, True)])
def test_loss_fwd_ws_equals_cleared(dev, p_frame, e_frame):
    """inputs whose partial sums are exact in fp32 (module docstring): any order of the atomics gives the same bits"""
    ops = _ops()
    args = _loss_case(dev, p_frame, e_frame, exact=True)
    mel, logd = args[0], args[9]
    B, T, n_mel = mel.shape
    L = logd.shape[1]

    def run(entry, sums):
        losses = torch.full((6,), float("nan"), device=dev)
        ops._lib.call(entry, mel.data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[2].stride(0), args[3].data_ptr(),
                      args[4].data_ptr(), args[5].data_ptr(), args[6].data_ptr(), args[6].stride(0), args[7].data_ptr(),
                      args[8].data_ptr(), args[8].stride(0), logd.data_ptr(), args[10].data_ptr(), args[10].stride(0),
                      args[11].data_ptr(), B, T, L, n_mel, int(p_frame), int(e_frame), sums.data_ptr(), losses.data_ptr(), ops._stream())
        return losses

    old = run("fs2_loss_fwd", torch.full((5,), float("nan"), device=dev))       # clears its sums itself
    ws = torch.zeros(8, device=dev)
    for i in range(3):                                          # the workspace is left zero: the next call needs no clear
        new = run("fs2_loss_fwd_ws", ws)
        _same(new, old, f"losses, call {i}")
        assert torch.equal(ws.cpu(), torch.zeros(8)), "workspace not left zero"
    assert torch.isfinite(old).all() and float(old[0]) > 0
    _same(ops.loss_fwd(*args, p_frame, e_frame), old, "ops.loss_fwd")


# ------------------------------------------------------------------------------------------------- gradient norm
def test_sumsq_set_equals_zero_then_sumsq(dev):
    ops = _ops()
    torch.manual_seed(14)
    for n in (8, 4096 + 4, 1_000_003):
        x = torch.randn(n + 4, device=dev)[4:4 + n]             # 16-byte aligned view
        old = torch.full((1,), float("nan"), device=dev)
        old.zero_()
        ops.sumsq(x, old)
        new = torch.full((1,), float("nan"), device=dev)         # any contents: the kernel stores
        ops.sumsq(x, new, set=True)
        _same(new, old, f"sumsq n={n}")


@pytest.mark.parametrize("lowp", [False, True])
def test_adam_step_with_launch_arguments_equals_device_vector(dev, lowp):
    ops = _ops()
    torch.manual_seed(15)
    n = 40_004
    lr, bc1, bc2 = 0.000731, 1 - 0.9 ** 7, 1 - 0.98 ** 7       # doubles, as ScheduledOptim computes them
    res = []
    for form in ("device", "args"):
        g0 = torch.Generator().manual_seed(3)
        p, g, m = (torch.randn(n, generator=g0).to(dev) for _ in range(3))
        v = torch.rand(n, generator=g0).to(dev)
        nsq = (g * g).sum().reshape(1)
        lp = torch.zeros(n, device=dev, dtype=torch.bfloat16) if lowp else None
        hyper = torch.tensor([lr, bc1, bc2, 0.0], dtype=torch.float32).to(dev) if form == "device" else (lr, bc1, bc2)
        ops.adam_step(p, g, m, v, nsq, 1.0, hyper, 0.9, 0.98, 1e-9, 0.0, p_lowp=lp, zero_grad=True)
        res.append((p, m, v, g) + ((lp,) if lowp else ()))
    for a, b, name in zip(res[0], res[1], ("p", "m", "v", "g (cleared)", "bf16 shadow")):
        _same(b, a, f"adam {name}")


# ------------------------------------------------------------------------------------------------- the hand-over in the model
def _model_case(dev, cdt, frame_level, max_seq_len):
    from oracle.weights import seeded_state_dict, synthetic_batch
    from tests.golden import configs
    from tests.helpers import make_model
    from fastspeech2_amd.model import FastSpeech2Loss

    pcfg, mcfg = configs.make(dropout=False, dec_layers=1, enc_layers=1, frame_level=frame_level, max_seq_len=max_seq_len or 1000)
    model = make_model(pcfg, mcfg, cdt)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 5))
    model.to(dev).train()
    model.disable_dropout = True
    b = synthetic_batch(21, 4, 12, dur_lo=4, dur_hi=8, frame_level=frame_level)       # (ragged: min_len_frac = 0.6)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    batch12 = (None, None, d["speakers"], d["texts"], d["src_lens"], d["max_src_len"], d["mels"], d["mel_lens"], d["max_mel_len"],
               d["pitches"], d["energies"], d["durations"])
    return model, FastSpeech2Loss(pcfg, mcfg), batch12


@pytest.mark.parametrize("frame_level,max_seq_len", [(False, None), (False, 40), (True, None)])
def test_bf16_step_hands_mel_gradients_over_in_bf16(dev, frame_level, max_seq_len):
    """bf16 step (ragged lengths; decoder shorter than the targets; frame-level features): the loss writes d mel / d postnet in bf16
    into the engine's sink, equal to cast(fp32 gradient of the old entry point), autograd carries nothing for them, and the whole
    backward runs from it."""
    ops = _ops()
    model, loss_fn, batch12 = _model_case(dev, "bf16", frame_level, max_seq_len)
    out = model(*batch12[2:])
    mel, post = out[0], out[1]
    assert mel.dtype == torch.float32 and post.dtype == torch.float32
    B, T, n_mel = mel.shape
    if max_seq_len is not None:
        assert T == max_seq_len < batch12[8], "case must truncate the decoder"
    sink = mel._fs2_sink
    assert sink is post._fs2_sink and sink.dtype == torch.bfloat16
    losses = loss_fn(batch12, out)
    assert sink.claimed
    # the loss node alone (gradients w.r.t. the model's prediction outputs stop in front of the engine's node)
    gp, ge, gd = torch.autograd.grad(losses[0], [out[2], out[3], out[4]], retain_graph=True)
    dmel, dpost = sink.dmel, sink.dpost
    assert dmel.dtype == torch.bfloat16 and dmel.shape == (B * T, n_mel)
    mel_t = batch12[6]
    cnt = out[9]._fs2_counts[0]
    g = torch.tensor([1.0, 0, 0, 0, 0, 0], device=dev)
    old = ops.loss_bwd(mel.detach(), post.detach(), mel_t, out[9].to(torch.int64), out[8].to(torch.int64), out[2].detach(),
                       batch12[9].float(), out[3].detach(), batch12[10].float(), out[4].detach(), batch12[11], cnt, g,
                       frame_level, frame_level)
    _same(dmel, ops.cast(old[0].view(B * T, n_mel), torch.bfloat16), "sink d mel")
    _same(dpost, ops.cast(old[1].view(B * T, n_mel), torch.bfloat16), "sink d postnet")
    _same(gp, old[2], "d pitch"); _same(ge, old[3], "d energy"); _same(gd, old[4], "d log-duration")
    losses[0].backward()
    torch.cuda.synchronize()
    assert sink.dmel is None, "Engine.backward did not take the hand-over"
    for n in ("mel_linear.weight", "postnet.convolutions.4.0.conv.weight", "encoder.src_word_emb.weight"):
        gr = dict(model.named_parameters())[n].grad
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0, n


def test_second_loss_on_the_same_outputs_goes_through_autograd(dev):
    """only the first loss owns the hand-over; a second one adds its gradient through autograd: the step's gradient is the sum"""
    model, loss_fn, batch12 = _model_case(dev, "bf16", False, None)
    out = model(*batch12[2:])
    (loss_fn(batch12, out)[0] + loss_fn(batch12, out)[0]).backward()
    g2 = model.mel_linear.bias.grad.clone()
    model.flat_gradients().zero_()
    out = model(*batch12[2:])
    loss_fn(batch12, out)[0].backward()
    g1 = model.mel_linear.bias.grad
    torch.cuda.synchronize()
    # d mel of the L1 terms is +-k or 0 and doubles exactly; the PostNet path is linear in the gradient up to bf16 rounding
    assert torch.allclose(g2, 2 * g1, rtol=2e-2, atol=1e-6 + 2e-2 * float(g1.abs().max()))
