"""fp64 references and per-element bounds for the inference / corpus side: the HBM-bound kernels around the vocoder and the mel
front end (fastspeech2_amd/csrc/fs2_vocoder.hip), the polyphase pack of the transposed convolutions (hifigan.Generator._pack_convt)
and the fused residual block (csrc/fs2_resblock.hip).  No GPU is used here; tests/test_vocoder_ref_cpu.py pins every function to
torch / numpy and shows that each bound passes a faithful CPU emulation and rejects a wrong one, tests/test_vocoder_elem_gpu.py runs
the kernels.  Bounds are those of tests/elem_ref.py (`allowed`: c * u * mag, u = 2^-24, + one bf16 rounding of a bf16 result) and of
tests/gemm_ref.py (`assert_rounding_only`) - never normalised by a maximum.

Bit-exact kernels (chan_to_rows, reflect_pad, reflect_pad_ragged): the same indexing on the CPU, compared bit for bit.

conv_post (conv_post_kernel): acc = bias, then for every tap inside the utterance and every channel one fmaf(lrelu(x), w, acc) onto the
ONE accumulator: a chain of taps * C dependent fmafs, one rounding each; lrelu(x) = x * in_slope is a rounded fp32 product for x < 0,
which moves every term by at most u of its magnitude, one more u on the whole sum:  c = taps * C + 1  on
mag = |bias| + sum |w| |lrelu(x)|.  tanh is 1-Lipschitz, so the output carries the same absolute bound, plus tanhf's own error
TANHF_ULPS * u * |tanh|.  PCM is the truncation of the kernel's own wav (bit-exact, the project's rule); against the reference it
may differ by ceil(bound * 32768) + 1 steps.

tanhf / logf: ROCm ships no accuracy statement for its device library's tanhf and logf, so both were measured once on the MI355X
against fp64 on the same fp32 arguments (test_tanhf_logf_measured: a 1-tap identity conv_post launch over 2^20 arguments in
[-2.3, 2.3] and denser near 0; a stft_mel launch with unit one-bin filters over 2^20 magnitudes in [2e-5, 1e4) and around 1):
    tanhf: max |err| / (u |tanh|) = 2.383,   logf: max |err| / (u |log|) = 3.000      (TANHF_SEEN, LOGF_SEEN)
and twice the observed maximum is allowed (TANHF_ULPS, LOGF_ULPS).

stft_mel (stft_mel_kernel), all terms non-negative so mag == ref:
  * magnitude sqrtf(re * re + im * im): a rounded square, an fmaf (or a second square and an add), a correctly rounded sqrtf:
    relative error <= (3 / 2 + 1) u <= 3 u;
  * mel bin k: a chain of span_k = hi - lo fmafs onto one accumulator: the sum's relative error is (span_k + 3) u, which is the
    same ABSOLUTE error after the log (-log1p(-e) to be exact), plus logf's own LOGF_ULPS * u * |log|.  A sum that is exactly 0
    (empty span, zero magnitudes) gives logf(clamp_min) and nothing else; the reference refuses inputs whose sums fall in
    (0, 2 clamp_min), so no case depends on which side of the clamp a rounding falls;
  * energy: per lane ceil(NF / 64) fmafs of squared magnitudes (each square 2 x 2.5 u = 5 u), the 6-level wave_sum, so the sum of
    squares is within (ceil(NF / 64) + 6 + 5) u; the square root halves that and adds its own rounding:
    c = (ceil(NF / 64) + 11) / 2 + 1.

Polyphase transposed convolution: `convt_polyphase` runs _pack_convt's image through gemm_ref.conv_reference and reads the
[B*T][u*Cout] rows as [B*T*u][Cout]; `convt_reference` is F.conv_transpose1d(stride = u, padding = (k - u) // 2) in fp64.

Fused residual block (`resblock_reference`): the block in fp64 with a per-element first-order error bound carried forward,
following resblock_fused_kernel line by line:
  * write_act rounds what a convolution READS to bf16: lrelu(y) and t = lrelu(conv1).  An operand known to within d becomes known to
    within d + u |op| (the fp32 product with the slope) + 2^-9 (|op| + d).  2^-9 is the AVERAGE size of a bf16 rounding (half an
    ulp at the top of a binade), not its worst case 2^-8: this one term is not a bound on a single operand.  It is used because an
    operand's error reaches an output only through a |W|-weighted sum over K = C k >= 96 operands, where it is still far above
    what independent roundings add up to (sqrt(K) of them);
  * a convolution maps d through |W| (the abs-weight convolution with the same zero padding) and adds (K + 1) u (|bias| + sum |W||op|)
    for the MFMA's fp32 accumulation (K products onto one accumulator that starts from the bias);
  * conv2 accumulates onto the running sum y in the same registers: (K + 2) u (|y| + |bias| + sum |W||t|); y itself is NEVER rounded;
  * leaky-ReLU is 1-Lipschitz;
  * xs = bf16(xs + out_scale * y): 2 u of fp32 arithmetic and one bf16 rounding per block (elem_ref.allowed); post_slope > 0 multiplies
    the stored bf16 value in fp32 and rounds to bf16 once more.
The bound is worst case in K and therefore loose by about sqrt(K), but local.  Whether a dropped or misplaced tap lands outside it
depends on the operands: see RB_WEIGHT_GAIN and the "coherent" family at resblock_case, and the mutants of
tests/test_vocoder_ref_cpu.py, which fail it in either convolution of every pair at every case configuration.  On the CPU emulation (tests/test_vocoder_ref_cpu.py) the largest err / bound is 0.96, the
final bf16 rounding; on the MI355X (RECORDED_RATIOS below, one passing run of all 87 cases) 0.976, the same rounding.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import elem_ref as R
from tests import gemm_ref as G

F64 = torch.float64
U32 = R.U32

# measured on the MI355X (see the docstring); allowed = 2 x seen
TANHF_SEEN, LOGF_SEEN = 2.383, 3.000
TANHF_ULPS, LOGF_ULPS = 2 * TANHF_SEEN, 2 * LOGF_SEEN

# max err / bound observed on the MI355X by tests/test_vocoder_elem_gpu.py (the "[voc] ..." lines)
RECORDED_RATIOS = {"conv_post wav taps=7": 0.149, "conv_post wav taps=1": 0.347,
                   "stft_mel mel (hand-built spans, all NF / n_mel)": 0.547, "stft_mel energy (hand-built spans)": 0.296,
                   "stft_mel mel (Slaney basis)": 0.387, "stft_mel energy (Slaney basis)": 0.107,
                   "framed DFT magnitude": 0.014, "polyphase convT fp32": 0.030, "polyphase convT bf16": 0.923,
                   "resblock random": 0.976, "resblock coherent": 0.853, "resstage random": 0.801, "resstage coherent": 0.486}


# ------------------------------------------------------------------------------------------------------- bit-exact kernels
def special_values():
    """-0.0, a denormal, bf16 ties (down to even, up to even), the largest finite value that stays finite in bf16"""
    return torch.tensor([0x80000000 - (1 << 32), 0x00000123, 0x3F808000, 0x3F818000, 0x7F7F7FFF, 0x3F800001],
                        dtype=torch.int64).to(torch.int32).view(torch.float32)


def chan_to_rows(x, dtype):
    """(B, C, T) fp32 -> rows [B*T][C], stored as fp32 (the input's bits) or bf16 (round-to-nearest-even)"""
    B, C, T = x.shape
    return R.store(x.float().transpose(1, 2).reshape(B * T, C).contiguous(), dtype)


def reflect_pad(y, P, row_len):
    """xp[b][i] = y[b][reflect(i - P)] for i < min(row_len, N + 2P), 0 beyond (F.pad(mode="reflect") plus zeros)"""
    B, N = y.shape
    assert N > P
    xp = F.pad(y.float().unsqueeze(1), (P, P), mode="reflect").squeeze(1) if P else y.float()
    out = torch.zeros(B, row_len, dtype=torch.float32)
    n = min(row_len, N + 2 * P)
    out[:, :n] = xp[:, :n]
    return out


def reflect_pad_ragged(y, lens, P, row_len):
    """row b: reflect_pad of its first lens[b] samples alone; all zero where lens[b] <= P (nothing of y is read there)"""
    out = torch.zeros(y.shape[0], row_len, dtype=torch.float32)
    for b, n in enumerate(lens):
        if n > P:
            out[b] = reflect_pad(y[b:b + 1, :n], P, row_len)[0]
    return out


# -------------------------------------------------------------------------------------------------------------- conv_post
def conv_post(x, w, bias, in_slope, S, taps, pad):
    """x [M][C] (the values the kernel reads, any float type), w [taps][C] fp32, bias (1,) fp32 or None ->
    (pre-activation fp64 [M], its magnitude, c)."""
    M, C = x.shape
    x64, w64 = x.to(F64), w.to(F64).view(1, taps, C)
    b64 = bias.to(F64).view(1) if bias is not None else None
    pre = G.conv_reference(x64, w64, b64, S, pad=pad, in_act=G.ACT_LRELU, in_slope=in_slope)[:, 0]
    a = torch.where(x64 > 0, x64, x64 * G.f32(in_slope)).abs()
    mag = G.conv_acc(a, w64.abs(), S, pad=pad)[:, 0] + (b64.abs() if b64 is not None else 0.0)
    return pre, mag, taps * C + 1


def conv_post_bound(pre, mag, c):
    """the absolute bound on wav = tanhf(acc): tanh is 1-Lipschitz, + tanhf's own error"""
    a = R.allowed(pre, mag, c)
    return a + TANHF_ULPS * U32 * (torch.tanh(pre).abs() + a)


def pcm_trunc(wav, max_wav=32768.0):
    """numpy astype('int16') of the fp32 product on x86: truncate toward zero to int32, keep the low 16 bits"""
    s = (wav.float() * torch.tensor(max_wav, dtype=torch.float32)).numpy()
    return (s.astype(np.int32) & 0xffff).astype(np.uint16).view(np.int16)


# --------------------------------------------------------------------------------------------------------------- stft_mel
def spans_of(basis):
    """[lo, hi) of each filter's non-zero band, (0, 0) for an all-zero filter (audio.TacotronSTFT builds the same table)"""
    span = torch.zeros(basis.shape[0], 2, dtype=torch.int32)
    for k in range(basis.shape[0]):
        idx = torch.nonzero(basis[k] != 0).flatten()
        if idx.numel():
            span[k, 0], span[k, 1] = int(idx[0]), int(idx[-1]) + 1
    return span


def stft_mel(ft, NF, frames, melb, span, clamp_min):
    """ft (B, S, ldft) fp32 (anything outside rows < frames and columns < 2 NF is ignored); melb (n_mel, NF) fp32; span (n_mel, 2).
    -> dict(mel=(ref, bound) (B, n_mel, frames), energy=(ref, mag, c) (B, frames), sums=..., clamped=bool mask)."""
    re, im = ft[:, :frames, :NF].to(F64), ft[:, :frames, NF:2 * NF].to(F64)
    mag = (re * re + im * im).sqrt()                                           # (B, frames, NF)
    energy = (mag * mag).sum(-1).sqrt()
    n_mel = melb.shape[0]
    w = torch.zeros(n_mel, NF, dtype=F64)
    width = torch.zeros(n_mel, dtype=F64)
    for k in range(n_mel):
        lo, hi = int(span[k, 0]), int(span[k, 1])
        w[k, lo:hi] = melb[k, lo:hi].to(F64)
        width[k] = hi - lo
    assert (w >= 0).all(), "the bound assumes non-negative filters"
    sums = torch.einsum("kq,bfq->bkf", w, mag)
    cm = float(torch.tensor(clamp_min, dtype=torch.float32))
    assert ((sums == 0) | (sums >= 2 * cm)).all(), "a filter sum inside (0, 2 clamp_min): the case would depend on a rounding"
    ref = sums.clamp_min(cm).log()
    rel = (width + 3).view(1, -1, 1) * U32
    a = torch.where(sums == 0, torch.zeros_like(sums), -torch.log1p(-rel).expand_as(sums))
    bound = a + LOGF_ULPS * U32 * (ref.abs() + a)
    return dict(mel=(ref, bound), energy=(energy, energy, (math.ceil(NF / 64) + 11) / 2 + 1), sums=sums, clamped=sums == 0)


def stft_numpy(y, filter_length, hop, win_length):
    """audio/stft.py in fp64 numpy: reflect pad by filter/2, frames of `filter_length` every `hop`, periodic Hann window of
    win_length centre-padded, DFT -> magnitude (B, cutoff, 1 + N // hop)."""
    from scipy.signal import get_window
    y = np.asarray(y, dtype=np.float64)
    B, N = y.shape
    P = filter_length // 2
    win = get_window("hann", win_length, fftbins=True)
    lpad = (filter_length - win_length) // 2
    win = np.pad(win, (lpad, filter_length - win_length - lpad))
    xp = np.pad(y, ((0, 0), (P, P)), mode="reflect")
    frames = N // hop + 1
    idx = np.arange(frames)[:, None] * hop + np.arange(filter_length)[None, :]
    n = np.arange(filter_length)
    k = np.arange(filter_length // 2 + 1)
    dft = np.exp(-2j * np.pi * k[:, None] * n[None, :] / filter_length)       # (cutoff, filter)
    spec = np.einsum("kn,bfn->bkf", dft, xp[:, idx] * win)
    return np.abs(spec)


# ------------------------------------------------------------------------------------ polyphase transposed convolution
class ConvtLayer:
    """what _pack_convt reads of a layer: effective_weight() (Cin, Cout, k) and bias (Cout,)"""

    def __init__(self, w, bias):
        self.w, self.bias = w, bias

    def effective_weight(self):
        return self.w


def convt_polyphase(x, wp, bias, taps, pad, u, S, post_slope=0.0):
    """the packed image [u*Cout][taps][Cin] as the (taps)-tap convolution it is, fp64, rows [B*S][u*Cout] read as [B*S*u][Cout]"""
    y = G.conv_reference(x.to(F64), wp.to(F64), bias.to(F64), S, pad=pad, post_slope=post_slope)
    return y.reshape(x.shape[0] * u, wp.shape[0] // u)


def convt_reference(x, w, bias, u, k, B, T, post_slope=0.0):
    """F.conv_transpose1d(stride = u, padding = (k - u) // 2) of rows x [B*T][Cin], fp64 -> rows [B*L][Cout] and L"""
    xc = x.to(F64).view(B, T, -1).transpose(1, 2)
    y = F.conv_transpose1d(xc, w.to(F64), bias.to(F64), stride=u, padding=(k - u) // 2)
    if post_slope > 0:
        y = torch.where(y > 0, y, y * G.f32(post_slope))
    L = y.shape[2]
    return y.transpose(1, 2).reshape(B * L, -1), L


# -------------------------------------------------------------------------------------------------- fused residual block
RB_E = {32: 1024, 64: 512}            # RbCfg<C>::E (fs2_resblock.hip: "tile rows")
RB_GUARD = 26                         # RbCfg<C>::GUARD


def rb_halo(k, dil):
    """rb_halo(): H = (k - 1) / 2 * (d0 + d1 + d2 + 3)"""
    return (k - 1) // 2 * (sum(dil) + 3)


def rb_rows(C, ks, dil):
    """(H, R) of a launch over blocks of kernel sizes ks: resblocks_impl takes the widest halo, R = E - 2 H"""
    H = max(rb_halo(k, dil) for k in ks)
    return H, RB_E[C] - 2 * H


def rb_supported(C, k, dil):
    """fs2_resblock_supported (bf16 only), restated"""
    if C not in RB_E or k < 1 or k > 11 or k % 2 == 0 or min(dil) < 1:
        return False
    if (k - 1) // 2 * max(dil) > RB_GUARD - 1:
        return False
    return RB_E[C] - 2 * rb_halo(k, dil) >= 64


def rb_lengths(H, R):
    return [1, H, R - 1, R, R + 1, 2 * R, 2 * R + 1]


def _lrelu64(t, slope):
    return torch.where(t > 0, t, t * slope)


def _operand(v, d, slope):
    """what write_act stores of a value v known to within d: lrelu in fp32, rounded to bf16"""
    a = _lrelu64(v, slope)
    return a, d + U32 * a.abs() + 2.0 ** -9 * (a.abs() + d)


def _conv64(a, w, b, dil, k):
    """a (B, C, S) fp64, w [C][k][C] (cout, tap, cin), zero padding (k - 1) / 2 * dil"""
    return F.conv1d(a, w.permute(0, 2, 1), b, dilation=dil, padding=(k - 1) // 2 * dil)


def resblock_reference(x, blocks, B, S, dil, xs0=None, out_scale=1.0 / 3, slope=0.1, post_slope=0.0):
    """x [B*S][C] bf16; blocks = [(w1 [3][C][k][C] bf16, w2, b1 [3][C] f32, b2, k)] (one entry: fs2_resblock_fwd, three:
    fs2_resstage_fwd); xs0 [B*S][C] bf16 or None.  -> (ref, bound), fp64 [B*S][C]: the exact result on these operands and the
    per-element bound on a bf16 result computed as the kernel computes it."""
    C = x.shape[1]
    sl, ps, osc = G.f32(slope), G.f32(post_slope), G.f32(out_scale)
    rows = lambda t: t.transpose(1, 2).reshape(B * S, C)                      # noqa: E731
    x64 = x.to(F64).view(B, S, C).transpose(1, 2)
    xs = xs0.to(F64) if xs0 is not None else torch.zeros(B * S, C, dtype=F64)
    dxs = torch.zeros_like(xs)
    for w1, w2, b1, b2, k in blocks:
        K = C * k
        y, dy = x64, torch.zeros_like(x64)
        for m in range(3):
            W1, W2, B1, B2 = w1[m].to(F64), w2[m].to(F64), b1[m].to(F64), b2[m].to(F64)
            a, da = _operand(y, dy, sl)
            t = _conv64(a, W1, B1, dil[m], k)
            dt = _conv64(da, W1.abs(), None, dil[m], k) + (K + 1) * U32 * _conv64(a.abs(), W1.abs(), B1.abs(), dil[m], k)
            t, dt = _operand(t, dt, sl)
            y_new = _conv64(t, W2, B2, 1, k) + y
            dy = dy + _conv64(dt, W2.abs(), None, 1, k) + (K + 2) * U32 * (_conv64(t.abs(), W2.abs(), B2.abs(), 1, k) + y.abs())
            y = y_new
        v = xs + osc * rows(y)
        d = dxs + osc * rows(dy) + 2 * U32 * (xs.abs() + osc * rows(y).abs())
        xs, dxs = v, R.allowed(v, d / U32, 1.0, torch.bfloat16)
    if ps > 0:
        xs = _lrelu64(xs, ps)
        dxs = R.allowed(xs, (dxs + U32 * xs.abs()) / U32, 1.0, torch.bfloat16)
    return xs, dxs


# The bound's first-order propagation multiplies an operand's error by sum |W| per convolution.  At the customary weight scale
# 1 / sqrt(K) that is 0.8 sqrt(K) per convolution, K per conv1 / conv2 pair: the bound of the third pair then exceeds a whole dropped
# tap (measured: err / bound of the tap mutant 0.09 at C = 32, k = 3).  With sigma = 0.6 / K, sum |W| ~ 0.5, the bound stays at the
# level of one operand rounding and every mutant of tests/test_vocoder_ref_cpu.py lands outside it at every (C, k).  The existing
# test_resblock_fused_matches_convolution_chain_and_exact keeps the 1 / sqrt(K) scale under its own assertions.
RB_WEIGHT_GAIN = 0.6


# A second family of operands, "coherent", makes a WHOLE TAP of conv1 - the dilated convolution whose halo and zero padding the seam
# lengths exist for - visible: x > 0 and conv1's weights > 0 (sum |W| = RB_COHERENT_GAIN per output), so a tap's C terms add up instead
# of cancelling, a dropped tap or a neighbour's row read for a zero moves t by 1 / k of its value; conv2 is the identity on its
# centre tap plus positive weights of sum 0.5, so t goes into the running sum unattenuated and conv2's own taps still count.  Every tenth channel has a bias that drives
# conv1 negative (the leaky-ReLU's other branch).  With random signs the same tap is sqrt(C) / (0.8 K) of sum |W||a| and, behind a
# random conv2, ends below the final bf16 rounding.
RB_COHERENT_GAIN = 1.0
RB_KINDS = ("random", "coherent")


def resblock_case(C, ks, S, seed, B=2, ld_extra=8, kind="random"):
    """seeded operands of a residual-block launch.  x and xs0 are column slices [:, :C] of [B*S][C + ld_extra] buffers whose padding
    columns hold NaN (nothing may read them)."""
    g = torch.Generator().manual_seed(seed)
    M = B * S
    coh = kind == "coherent"
    xv = torch.randn(M, C, generator=g) * 0.7
    xb = torch.full((M, C + ld_extra), float("nan")).to(torch.bfloat16)
    xb[:, :C] = ((xv.abs() * 0.7 + 0.25) if coh else xv).to(torch.bfloat16)
    xsb = torch.full((M, C + ld_extra), float("nan")).to(torch.bfloat16)
    xsb[:, :C] = torch.randn(M, C, generator=g).to(torch.bfloat16)
    blocks = []
    for k in ks:
        K = C * k
        w1 = torch.randn(3, C, k, C, generator=g)
        w2 = torch.randn(3, C, k, C, generator=g)
        b1, b2 = torch.randn(3, C, generator=g) * 0.1, torch.randn(3, C, generator=g) * 0.1
        if coh:
            w1 = w1.abs() * (RB_COHERENT_GAIN / (0.8 * K))
            w2 = w2.abs() * (0.5 / (0.8 * K))
            w2[:, torch.arange(C), (k - 1) // 2, torch.arange(C)] = 1.0
            b1, b2 = b1 * 0.2, b2 * 0.2
            b1[:, ::10] = -3.0
        else:
            w1, w2 = w1 * (RB_WEIGHT_GAIN / K), w2 * (RB_WEIGHT_GAIN / K)
        blocks.append((w1.to(torch.bfloat16), w2.to(torch.bfloat16), b1, b2, k))
    return xb, xsb, blocks


def ratio(got, ref, bound):
    """max err / bound (inf for a NaN; 0 where both are exactly 0)"""
    err = (got.detach().cpu().to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.nan_to_num(nan=math.inf, posinf=math.inf).max()) if r.numel() else 0.0


def assert_within(got, ref, bound, what):
    err = (got.detach().cpu().to(F64) - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first #{i}: got "
                             f"{got.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} lim {bound.reshape(-1)[i].item():.3g}")
    return ratio(got, ref, bound)


# ------------------------------------------------------------------------------------------------------------ case tables
RB_DILS = [(3, (1, 3, 5)), (7, (1, 3, 5)), (11, (1, 3, 5)), (3, (1, 1, 1)), (7, (1, 1, 1)), (11, (1, 1, 1)), (3, (5, 3, 1)), (7, (5, 3, 1))]
RB_CONFIGS = [(C, k, d) for C in (32, 64) for k, d in RB_DILS]
RB_FORMS = [(False, 0.0), (False, 0.1), (True, 0.0), (True, 0.1)]           # (accumulate, post_slope)
CONVT_PAIRS = [(8, 16), (2, 4), (4, 8), (3, 9), (5, 11), (3, 7), (1, 3), (2, 2), (8, 8)]
POST_LENGTHS = [(3, 1), (4, 2), (5, 3), (2, 7), (3, 255), (2, 256), (3, 257)]


def conv_post_case(dtype, C, taps, in_slope, has_bias, ldx, B, S, seed):
    """x [M][ldx] (columns >= C hold NaN), w [taps][C], bias (1,) | None.  Utterances alternate between scale 1 and scale 100, and
    the weights are scaled so that the largest |pre-activation| is 2 (|tanh| <= 0.965: away from the PCM wrap at 1.0)."""
    g = torch.Generator().manual_seed(seed)
    M = B * S
    vals = torch.randn(B, S, C, generator=g) * torch.tensor([1.0, 100.0]).repeat(B)[:B].view(B, 1, 1)
    x = torch.full((M, ldx), float("nan")).to(dtype)
    x[:, :C] = vals.view(M, C).to(dtype)
    w = torch.randn(taps, C, generator=g)
    bias = torch.randn(1, generator=g) if has_bias else None
    pre, _, _ = conv_post(x[:, :C], w, bias, in_slope, S, taps, (taps - 1) // 2)
    s = 2.0 / float(pre.abs().max())
    return x, (w * s).float().contiguous(), (bias * s).float() if has_bias else None


def stft_mel_case(NF, n_mel, frames, S, ldft, B, seed, slaney=None):
    """ft (B, S, ldft): rows >= frames and columns >= 2 NF hold NaN; filters: hand-built contiguous spans - an empty one, one of
    length 1, one over all of [0, NF), the rest random - with NaN outside each span, or the given Slaney basis.  Bin q1 (the
    length-1 filter's) has zero magnitude in frame 0: that sum is exactly 0."""
    g = torch.Generator().manual_seed(seed)
    ft = torch.full((B, S, ldft), float("nan"))
    ft[:, :frames, :2 * NF] = torch.randn(B, frames, 2 * NF, generator=g)
    if slaney is not None:
        melb = torch.as_tensor(slaney, dtype=torch.float32).contiguous()
        return ft, melb, spans_of(melb)
    q1 = NF // 2
    ft[:, 0, q1] = 0.0
    ft[:, 0, NF + q1] = 0.0
    span = torch.zeros(n_mel, 2, dtype=torch.int32)
    span[0] = torch.tensor([2, 2])
    span[1] = torch.tensor([q1, q1 + 1])
    span[2] = torch.tensor([0, NF])
    for k in range(3, n_mel):
        lo = int(torch.randint(0, NF, (1,), generator=g))
        span[k] = torch.tensor([lo, min(NF, lo + 1 + int(torch.randint(0, 40, (1,), generator=g)))])
    melb = torch.full((n_mel, NF), float("nan"))
    for k in range(n_mel):
        lo, hi = int(span[k, 0]), int(span[k, 1])
        melb[k, lo:hi] = (0.25 + torch.rand(hi - lo, generator=g)) / max(1, hi - lo) ** 0.5
    return ft, melb, span
