"""MelGAN generator (Kumar et al., NeurIPS 2019; the reference's `vocoder.model: "MelGAN"`) over the HIP kernel library.

The network, as published (this docstring is the specification the tests' fp64 restatement is written from).  Input x is
(B, 80, T) float32 - the mel ALREADY divided by ln 10 (the reference feeds `mels / np.log(10)`, utils/model.py:78).  With ngf = 32 and
ratios (8, 8, 2, 2) the `nn.Sequential` named `model` is

    0  ReflectionPad1d(3)
    1  WNConv1d(80, 512, k=7)
    for i, r in enumerate((8, 8, 2, 2)):          # C_in = 512 >> i, C = C_in / 2
       2+5i  LeakyReLU(0.2)
       3+5i  WNConvTranspose1d(C_in, C, k=2r, stride=r, padding=r//2 + r%2, output_padding=r%2)
       4+5i, 5+5i, 6+5i  ResnetBlock(C, dilation = 1, 3, 9)
    22 LeakyReLU(0.2)   23 ReflectionPad1d(3)   24 WNConv1d(32, 1, k=7)   25 Tanh
    ResnetBlock(x) = shortcut(x) + block(x)
       shortcut = WNConv1d(C, C, k=1)
       block    = [0 LeakyReLU(0.2), 1 ReflectionPad1d(d), 2 WNConv1d(C, C, k=3, dilation=d), 3 LeakyReLU(0.2), 4 WNConv1d(C, C, k=1)]

WN is torch.nn.utils.weight_norm with its old key names: `model.1.{weight_g,weight_v,bias}`, `model.3.*`, `model.4.block.2.*`,
`model.4.block.4.*`, `model.4.shortcut.*`, ..., `model.24.*`; weight_g is (C_out, 1, 1) for Conv1d and (C_in, 1, 1) for
ConvTranspose1d.  The released `linda_johnson.pt` / `multi_speaker.pt` are described as a plain state_dict of this module; that schema
is taken from the publication and has NOT been checked against the files (they were never available where this was written).
Output: (B, 1, 256 T) in [-1, 1].  Reflection is at the ends of the batch tensor's time axis; T < 4 is a ValueError (torch refuses a
reflection pad >= the input length).

Underneath (time-major rows, as hifigan.py):
  * every activation buffer is [B][G + S + G][C]: G guard rows per batch item, filled by `fs2_melgan_guard_rows` - by reflection in
    front of a reflection-padded convolution, with zeros in front of a transposed one - so the zero-padding contraction kernels run
    unchanged over S + 2G rows per item (what they compute for the guard rows is never read);
  * conv 1 and the transposed convolutions (polyphase form, hifigan.Generator._pack_convt) are fs2_conv_gemm launches;
  * a ResnetBlock is two launches: conv3 (leaky-ReLU on operand load and on the accumulators) writes t beside x in a [x | t] buffer,
    and shortcut + conv4 are ONE contraction over K = 2C: [x | t] . [W_shortcut ; W_4] + (b_shortcut + b_4);
  * the narrow stages (C = 64, 32) in bf16 run their three blocks in one launch (`fs2_melgan_stage_fwd`) when `fuse_stages` is set
    (off by default: the fused stage has not been timed against the chain yet - tools/bench_melgan.py does that);
  * a stage's output is STORED leaky-ReLU'd (slope 0.2): its only consumer is the next transposed convolution, or conv 24, and both
    read lrelu(value).  So the last stage's launch applies the final LeakyReLU(0.2) and `fs2_conv_post_pcm` reads it as it is
    (in_slope = 1: its prologue `v > 0 ? v : v * in_slope` is then the identity), after a reflection guard fill.
GPU only, inference only.
"""
import torch
import torch.nn as nn

from . import _lib, ops
from .hifigan import Generator as _HifiGenerator, _WNConv
from .ops import ACT_LRELU, ACT_NONE

LRELU_SLOPE = 0.2
RATIOS = (8, 8, 2, 2)
DILATIONS = (1, 3, 9)
GUARD = 9                  # guard rows of a stage's buffers: the largest dilation (and >= 3, conv 24's reach)
MIN_FRAMES = 4             # ReflectionPad1d(3) needs more than 3 frames


class _NoParams(nn.Module):
    """a parameterless position of the published nn.Sequential (padding, activation): keeps the state-dict indices"""


class _ResnetBlock(nn.Module):
    def __init__(self, dim, dilation):
        super().__init__()
        self.dilation = dilation
        self.block = nn.Sequential(_NoParams(), _NoParams(), _WNConv((dim, dim, 3), dim * 3), _NoParams(), _WNConv((dim, dim, 1), dim))
        self.shortcut = _WNConv((dim, dim, 1), dim)

    def convs(self):
        return self.block[2], self.block[4], self.shortcut


class Generator(nn.Module):
    """the published MelGAN generator; same surface as hifigan.Generator."""

    def __init__(self, n_mel=80, ngf=32, n_residual_layers=3, compute_dtype="fp32"):
        super().__init__()
        assert n_residual_layers == len(DILATIONS), "the published generator has three residual layers per stage (dilation 1, 3, 9)"
        self.n_mel, self.ngf = n_mel, ngf
        self.hop = 1
        for r in RATIOS:
            self.hop *= r
        c0 = ngf * 2 ** len(RATIOS)
        layers = [_NoParams(), _WNConv((c0, n_mel, 7), n_mel * 7)]
        for i, r in enumerate(RATIOS):
            cin, c = c0 >> i, c0 >> (i + 1)
            # ConvTranspose1d weight is (Cin, Cout, k): weight_norm's dim-0 norm is per INPUT channel
            layers += [_NoParams(), _WNConv((cin, c, 2 * r), c * 2 * r, norm_dim0=c)]
            layers += [_ResnetBlock(c, d) for d in DILATIONS]
        layers += [_NoParams(), _NoParams(), _WNConv((1, ngf, 7), ngf * 7), _NoParams()]
        self.model = nn.Sequential(*layers)
        self.set_compute_dtype(compute_dtype)
        # True: the narrow stages' three blocks in one launch where fs2_melgan_stage_supported; False: the chain of single launches.
        # The chain is the default until tools/bench_melgan.py has shown the fused stage to be the faster one
        self.fuse_stages = False
        self.stage_probe = None          # a list: _run appends (raw output rows (B, S, C) fp32, S) of conv 1 and of every stage (tests)
        self.register_load_state_dict_post_hook(lambda m, k: m._invalidate())

    set_compute_dtype = _HifiGenerator.set_compute_dtype
    _invalidate = _HifiGenerator._invalidate
    prepare = _HifiGenerator.prepare

    def _wn_layers(self):
        for m in self.model.modules():
            if isinstance(m, _WNConv):
                yield m

    def remove_weight_norm(self):
        for l in self._wn_layers():
            l.remove_weight_norm()
        self._invalidate()

    # ------------------------------------------------------------------ weight packing (once per load / device)
    def _weights(self, dev):
        key = (dev, self.compute_dtype)
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        cdt = self.compute_dtype
        lib = _lib.load()
        pack_conv, pack_convt = _HifiGenerator._pack_conv, _HifiGenerator._pack_convt
        W = {"pre": pack_conv(self.model[1], dev, cdt)}
        for i, r in enumerate(RATIOS):
            W[f"up{i}"] = pack_convt(self.model[3 + 5 * i], r, 2 * r, dev, cdt)
            fused_w, fused_b = [], []
            for j in range(len(DILATIONS)):
                c3, c4, sc = self.model[4 + 5 * i + j].convs()
                W[f"rb{i}.{j}.3"] = pack_conv(c3, dev, cdt)
                w3, w4, ws = (l.effective_weight().detach().to(dev, torch.float32) for l in (c3, c4, sc))
                b3, b4, bs = (l.bias.detach().to(dev, torch.float32) for l in (c3, c4, sc))
                # shortcut + conv4 as one contraction over [x | t]: [Cout][1][2C]
                W[f"rb{i}.{j}.11"] = (torch.cat([ws, w4], dim=1).permute(0, 2, 1).contiguous().to(cdt), (bs + b4).contiguous())
                fused_w.append(torch.cat([w3.permute(2, 0, 1).reshape(-1, w3.shape[1]), ws[:, :, 0], w4[:, :, 0]], dim=0))
                fused_b.append(torch.stack([b3, bs + b4]))
            C = fused_b[0].shape[1]
            if lib.fs2_melgan_stage_supported(C, ops.dt(cdt)):
                W[f"stage{i}"] = (torch.stack(fused_w).contiguous().to(cdt), torch.stack(fused_b).contiguous())
        wpost = self.model[24].effective_weight().detach().to(dev, torch.float32)      # (1, C, 7)
        W["post"] = (wpost[0].t().contiguous(), self.model[24].bias.detach().to(dev, torch.float32).contiguous())
        self._packed = (key, W)
        return W

    # ------------------------------------------------------------------ forward
    def _run(self, x_rows, B, T, want_wav, want_pcm, max_wav_value):
        """x_rows: [B*T][n_mel] in the compute dtype.  Returns (wav f32 (B, T*hop) | None, pcm int16 (B, T*hop) | None), views of the
        guarded sample buffers."""
        W = self._weights(x_rows.device)
        dev, cdt = x_rows.device, x_rows.dtype
        SL, G = LRELU_SLOPE, GUARD

        def raw(t):
            """fp32 copy of a stored (leaky-ReLU'd) activation in its RAW form (tests' stage probe only)"""
            t = t.float()
            return torch.where(t > 0, t, t / SL)

        # 0, 1: reflection guard rows (3 per side) around the mel rows, conv 1 over them; stored leaky-ReLU'd (2: its only consumer)
        S, Gin = T, 3
        a = torch.empty(B, S + 2 * Gin, self.n_mel, device=dev, dtype=cdt)
        ops.melgan_guard_rows(x_rows.view(B, S, self.n_mel), a, Gin, reflect=True, interior=True)
        wp, bp = W["pre"]
        h = ops.conv_gemm(a.view(-1, self.n_mel), wp, bp, S + 2 * Gin, taps=7, pad=3, act=ACT_LRELU, slope=SL)
        if self.stage_probe is not None:
            self.stage_probe.append((raw(h.view(B, S + 2 * Gin, -1)[:, Gin:Gin + S]), S))
        for i, r in enumerate(RATIOS):
            wu, bu, taps, pad = W[f"up{i}"]
            C = wu.shape[0] // r
            # 3+5i: the transposed convolution zero-pads: zero guard rows, then its polyphase form over all S + 2 Gin rows per item
            h3 = h.view(B, S + 2 * Gin, -1)
            ops.melgan_guard_rows(h3[:, Gin:Gin + S], h3, Gin, reflect=False, interior=False)
            u = ops.conv_gemm(h, wu, bu, S + 2 * Gin, taps=taps, pad=pad)
            Sn = S * r
            u3 = u.view(B, (S + 2 * Gin) * r, C)[:, Gin * r:Gin * r + Sn]          # the up-sampled rows [0, Sn) of every item
            out = torch.empty(B, Sn + 2 * G, C, device=dev, dtype=cdt)             # the stage's output, stored leaky-ReLU'd
            out_rows = out[:, G:G + Sn]
            st = W.get(f"stage{i}") if self.fuse_stages else None
            if st is not None and Sn >= 32:
                ops.melgan_stage_fwd(u3, st[0], st[1], out_rows, DILATIONS, slope=SL, out_slope=SL)
            else:
                cat = [torch.empty(B, Sn + 2 * G, 2 * C, device=dev, dtype=cdt) for _ in range(2)]       # [x | t], ping-pong
                ops.melgan_guard_rows(u3, cat[0][:, :, :C], G, reflect=True, interior=True)
                for j, d in enumerate(DILATIONS):
                    cur = cat[j % 2]
                    cur2 = cur.view(-1, 2 * C)
                    if j > 0:
                        ops.melgan_guard_rows(cur[:, G:G + Sn, :C], cur[:, :, :C], G, reflect=True, interior=False)
                    w3, b3 = W[f"rb{i}.{j}.3"]
                    w11, b11 = W[f"rb{i}.{j}.11"]
                    # t = lrelu(conv3(lrelu(x))) beside x
                    ops.conv_gemm(cur2, w3, b3, Sn + 2 * G, taps=3, dil=d, pad=d, act=ACT_LRELU, slope=SL, in_act=ACT_LRELU, in_slope=SL,
                                  Cin=C, out=cur2[:, C:])
                    last = j == len(DILATIONS) - 1
                    dst = out.view(-1, C) if last else cat[(j + 1) % 2].view(-1, 2 * C)[:, :C]
                    ops.conv_gemm(cur2, w11, b11, Sn + 2 * G, taps=1, act=ACT_LRELU if last else ACT_NONE, slope=SL if last else 0.0, out=dst)
            h, S, Gin = out.view(-1, C), Sn, G
            if self.stage_probe is not None:
                self.stage_probe.append((raw(out_rows), S))
        # 22-25: the stored rows are lrelu'd already; reflection guard rows, conv 24 + tanh (+ PCM)
        h3 = h.view(B, S + 2 * G, -1)
        ops.melgan_guard_rows(h3[:, G:G + S], h3, G, reflect=True, interior=False)
        wpost, bpost = W["post"]
        M = B * (S + 2 * G)
        wav = torch.empty(B, S + 2 * G, device=dev, dtype=torch.float32) if want_wav else None
        pcm = torch.empty(B, S + 2 * G, device=dev, dtype=torch.int16) if want_pcm else None
        _lib.call("fs2_conv_post_pcm", h.data_ptr(), h.stride(0), wpost.data_ptr(), bpost.data_ptr(), 1.0,
                  wav.data_ptr() if want_wav else None, pcm.data_ptr() if want_pcm else None, float(max_wav_value), M, S + 2 * G,
                  h.shape[1], wpost.shape[0], 3, ops.dt(h), ops._stream())
        return (wav[:, G:G + S] if want_wav else None), (pcm[:, G:G + S] if want_pcm else None)

    def _rows(self, x):
        """(B, n_mel, T) float32 -> rows [B*T][n_mel] in the compute dtype."""
        if x.dim() != 3 or x.shape[1] != self.n_mel:
            raise ValueError(f"melgan.Generator: expected (B, {self.n_mel}, T), got {tuple(x.shape)}")
        if x.shape[2] < MIN_FRAMES:
            raise ValueError(f"melgan.Generator: T = {x.shape[2]} frames; ReflectionPad1d(3) needs at least {MIN_FRAMES}")
        if not x.is_cuda:
            raise RuntimeError("fastspeech2_amd.melgan.Generator runs on an AMD GPU only (no CPU fallback)")
        B, C, T = x.shape
        x = x.contiguous().float()
        rows = torch.empty(B * T, C, device=x.device, dtype=self.compute_dtype)
        _lib.call("fs2_chan_to_rows", x.data_ptr(), rows.data_ptr(), B, C, T, ops.dt(rows), ops._stream())
        return rows, B, T

    def forward(self, x):
        rows, B, T = self._rows(x)
        wav, _ = self._run(rows, B, T, True, False, 32768.0)
        return wav.unsqueeze(1)

    def infer_pcm(self, x, max_wav_value=32768.0):
        """forward + `(wav * max_wav_value).astype("int16")` (utils/model.py:82-85) fused on the device.  x: the mel divided by ln 10.
        Returns int16 (B, T*hop)."""
        rows, B, T = self._rows(x)
        _, pcm = self._run(rows, B, T, False, True, max_wav_value)
        return pcm
