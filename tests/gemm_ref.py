"""Exact-product reference of the implicit-GEMM contraction (fs2_conv_gemm and its split-K / stored-leaky-ReLU entry points), the
rounding-only bound it is compared with, and the table of launch descriptions tests/test_gemm_dispatch_gpu.py runs.

The op (fastspeech2_amd/csrc/fs2_gemm.hip): rows X[M][Cin] hold Bq sequences of S time steps, W[N][taps][Cin],
    acc[m][n] = sum_j sum_c act_in(X[m + j dil - pad][c]) W[n][j][c]        taps outside [0, S) of the row's own sequence give 0
and the epilogue, in the order gemm_store_tile applies it:
    v = act(acc + bias)                       none / ReLU / tanh / leaky-ReLU(slope); the ReLU GATE is applied with the operand:
    v = r > 0 ? v : 0   or   v = v + r        r = res (or, res_unlrelu > 0: res holds lrelu(r), undone as res > 0 ? res : res * res_unlrelu)
    v = v * out_scale;  rows >= lens -> 0;  v += old output (accumulate);  v = lrelu(v, post_slope);  rounded once to the storage type.

Reference: operands exactly as the kernel sees them (the bf16 / fp32 values it reads; the leaky-ReLU prologue applied in fp32 and
rounded to the storage type as the kernel's loader does), one matmul per tap in fp32 (bf16 x bf16 products are exact in fp32) -
fp64 when the operands arrive as fp64, which is how tests/test_gemm_ref_cpu.py pins it to F.conv1d -, taps summed in fp64, epilogue
in fp64 with the fp32 values of the scalar arguments.

Bound (`assert_rounding_only`, unchanged from tests/test_a_prodshape_gpu.py where it was calibrated on reductions up to K = 9216):
    |y - ref| <= ulp |ref| + floor max|ref|      ulp, floor = 2^-8, 2e-4 (bf16) / 2^-20, 2e-5 (fp32)
Every case of the table keeps K = taps x Cin <= 9216, so no further constant is needed.  A NaN in y fails the bound.
"""
import dataclasses
import math

import torch

ACT_NONE, ACT_RELU, ACT_TANH, ACT_LRELU, ACT_GATE = 0, 1, 2, 3, 4          # = fastspeech2_amd.ops.ACT_* (asserted by the GPU test)
PLAIN, DMA, RING, SKINNY, PERSIST, PERSIST_1TAP, WIDE_1TAP, STREAM_K256 = 1, 2, 3, 4, 5, 6, 7, 9
VARIANT_NAMES = {PLAIN: "plain", DMA: "dma", RING: "ring", SKINNY: "skinny", PERSIST: "persist", PERSIST_1TAP: "persist1",
                 WIDE_1TAP: "wide1", STREAM_K256: "streamk256"}
ULP = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -20}
FLOOR = {torch.bfloat16: 2e-4, torch.float32: 2e-5}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
K_MAX = 9216


def f32(v):
    """the fp32 value of a scalar argument (what the kernel receives for 0.1 or 1 / 3)"""
    return torch.tensor(float(v), dtype=torch.float32).item()


def _lrelu(t, slope):
    return torch.where(t > 0, t, t * slope)


def pad_rows(lens, Bq, S, device=None):
    """bool [Bq*S]: row t of sequence b with t >= lens[b]"""
    lens = torch.as_tensor(lens).to(device if device is not None else "cpu")
    return (torch.arange(S, device=lens.device).unsqueeze(0) >= lens.unsqueeze(1)).reshape(-1)


def conv_acc(x, w, S, dil=1, pad=0, in_act=ACT_NONE, in_slope=0.0, store=None):
    """fp64 [M][N] accumulator of the contraction.  x [M][Cin], w [N][taps][Cin] hold the values the kernel reads (any float
    type); store: the storage type the prologue rounds to (default: x's own)."""
    M, Cin = x.shape
    N, taps, _ = w.shape
    Bq = M // S
    assert Bq * S == M and 0 <= pad <= (taps - 1) * dil
    mm = torch.float64 if x.dtype == torch.float64 else torch.float32
    xs = x.to(mm)
    if in_act == ACT_LRELU:
        xs = _lrelu(x.float() if mm == torch.float32 else xs, f32(in_slope)).to(store or x.dtype).to(mm)
    else:
        assert in_act == ACT_NONE
    xs = xs.reshape(Bq, S, Cin)
    wm = w.to(mm)
    acc = torch.zeros(Bq, S, N, device=x.device, dtype=torch.float64)
    for j in range(taps):
        sh = j * dil - pad
        lo, hi = max(0, -sh), min(S, S - sh)
        if hi > lo:
            acc[:, lo:hi] += (xs[:, lo + sh:hi + sh] @ wm[:, j, :].t()).double()
    return acc.view(M, N)


def epilogue(acc, bias=None, act=ACT_NONE, slope=0.0, res=None, out_scale=1.0, lens=None, S=None, old=None, res_unlrelu=0.0,
             post_slope=0.0):
    """the kernel's epilogue on an fp64 accumulator, in fp64, in the kernel's order.  old: the previous output (accumulate)."""
    v = acc.double().clone()
    if bias is not None:
        v = v + bias.double()
    if act == ACT_RELU:
        v = torch.relu(v)
    elif act == ACT_TANH:
        v = torch.tanh(v)
    elif act == ACT_LRELU:
        v = _lrelu(v, f32(slope))
    else:
        assert act in (ACT_NONE, ACT_GATE)
    if res is not None:
        r = res.double()
        if res_unlrelu > 0:
            r = _lrelu(r, f32(res_unlrelu))
        v = torch.where(r > 0, v, torch.zeros_like(v)) if act == ACT_GATE else v + r
    else:
        assert act != ACT_GATE and not res_unlrelu
    v = v * f32(out_scale)
    if lens is not None:
        v[pad_rows(lens, acc.shape[0] // S, S, acc.device)] = 0
    if old is not None:
        v = v + old.double()
    if post_slope > 0:
        v = _lrelu(v, f32(post_slope))
    return v


def conv_reference(x, w, bias, S, dil=1, pad=0, lens=None, act=ACT_NONE, slope=0.0, in_act=ACT_NONE, in_slope=0.0, res=None,
                   out_scale=1.0, old=None, res_unlrelu=0.0, post_slope=0.0, store=None):
    return epilogue(conv_acc(x, w, S, dil, pad, in_act, in_slope, store), bias, act, slope, res, out_scale, lens, S, old,
                    res_unlrelu, post_slope)


def dgrad_weight(w):
    """the tap-flipped transposed pack fs2_pack_weight writes for the data gradient: Wd[c][j][n] = W[n][k-1-j][c]"""
    return w.flip(1).permute(2, 1, 0).contiguous()


def rounding_bound(ref, dtype):
    ref = ref.double()
    scale = ref.abs().max().item() if ref.numel() else 0.0
    return ULP[dtype] * ref.abs() + FLOOR[dtype] * scale


def rounding_ratio(y, ref, dtype):
    """max over elements of err / bound (inf for a NaN or an infinity in y; 0 when both are exactly 0 everywhere)"""
    if ref.numel() == 0:
        return 0.0
    ref = ref.double()
    err = (y.double() - ref).abs()
    bound = rounding_bound(ref, dtype)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return ratio.nan_to_num(nan=math.inf, posinf=math.inf).max().item()


def assert_rounding_only(y, ref, dtype, what):
    """|y - ref| <= 1 ulp of the storage type relative to |ref| (+ an absolute floor for cancelling sums); a NaN fails."""
    ref = ref.double()
    scale = ref.abs().max().item() if ref.numel() else 0.0
    err = (y.double() - ref).abs()
    bad = ~(err <= rounding_bound(ref, dtype))
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        r, c = divmod(i, ref.shape[-1]) if ref.dim() == 2 else (i, 0)
        raise AssertionError((what, int(bad.sum()), err.nan_to_num(nan=math.inf).max().item(), scale,
                              f"first at row {r} col {c}: got {y.reshape(-1)[i].item():.6g} want {ref.reshape(-1)[i].item():.6g}"))


# ---------------------------------------------------------------------------------------------------------------- the case table
@dataclasses.dataclass(frozen=True)
class Launch:
    family: str          # single | stft | edge | pair | ops13 | io
    dtype: str           # bf16 | fp32
    Bq: int
    S: int
    Cin: int
    N: int
    taps: int
    dil: int = 1
    pad: int = 0
    lens: bool = False           # the description itself carries lens (every form then runs with them) ...
    tmap: bool = False           # ... and the tile map
    base_res: bool = False       # the description carries a residual operand (its row stride is part of the dispatch)
    ldy_odd: bool = False        # ldy not a multiple of 8 (bf16) / 4 (fp32) elements: vec_ok false
    ldr_odd: bool = False        # ldr likewise
    out_shift: int = 0           # out's base offset by this many elements from a 16-byte boundary
    io: tuple = None             # (accumulate, res_unlrelu, post_slope): a fs2_conv_gemm_lrelu_io launch
    pair: str = None             # the predicate this description straddles ...
    side: str = None             # ... and on which side ("a" takes the kernel, "b" must not)
    note: str = ""

    @property
    def M(self):
        return self.Bq * self.S

    @property
    def epc(self):
        return 8 if self.dtype == "bf16" else 4

    @property
    def edge(self):
        """geometry edges, straddling pairs and the op-level shapes: full epilogue rotation and the data-gradient form, never thinned"""
        return self.family in ("edge", "pair", "ops13", "stft", "io")

    @property
    def ldy(self):
        return (self.N + self.epc - 1) // self.epc * self.epc + self.epc + (1 if self.ldy_odd else 0)

    @property
    def ldr(self):
        return (self.N + self.epc - 1) // self.epc * self.epc + self.epc + (1 if self.ldr_odd else 0)

    @property
    def shape(self):
        s = f"B{self.Bq}xS{self.S}-C{self.Cin}-N{self.N}-k{self.taps}d{self.dil}p{self.pad}"
        for flag, tag in ((self.lens, "lens"), (self.tmap, "tmap"), (self.base_res, "res"), (self.ldy_odd, "ldyodd"), (self.ldr_odd, "ldrodd"),
                          (self.out_shift, "yshift"), (self.io, "io" + "".join(str(int(bool(v))) for v in (self.io or ())))):
            if flag:
                s += "-" + tag
        return s

    @property
    def ks2(self):
        return ks2(self.dtype, self.M, self.N, self.Cin, self.taps)


def ks2(dtype, M, N, Cin, taps):
    """conv_gemm_pick's in-workgroup K split of the DMA kernel (p.ks2), restated: bf16, at most 160 tiles of 128 x 128, whole
    128-channel chunk pairs, at least 12 K-steps"""
    grid = -(-M // 128) * -(-N // 128)
    return dtype == "bf16" and grid <= 160 and Cin % 128 == 0 and taps * (Cin // 64) >= 12


# (Cin, Cout, k) of every contraction of the train step (tests/test_a_prodshape_gpu.py SHAPES; the variance predictor's two k = 3
# convolutions are its (256, 256, 3)) and the op-level shapes tests/test_ops_gpu.py has always run (B, S, Cin, Cout, k, dil)
MODEL_SHAPES = [(256, 1024, 9), (1024, 256, 1), (256, 768, 1), (256, 256, 1), (512, 512, 5), (80, 512, 5), (512, 80, 5), (256, 80, 1), (256, 256, 3)]
OPS_FWD_SHAPES = [(3, 50, 256, 256, 1, 1), (2, 77, 256, 1024, 9, 1), (2, 130, 80, 512, 5, 1), (1, 300, 512, 80, 5, 1), (2, 64, 128, 128, 3, 3),
                  (1, 200, 32, 8, 7, 1), (2, 33, 1024, 256, 1, 1), (1, 257, 64, 64, 11, 5)]
OPS_GRAD_SHAPES = [(2, 70, 256, 1024, 9, 1), (2, 61, 256, 256, 3, 1), (1, 140, 80, 512, 5, 1), (3, 40, 256, 768, 1, 1), (1, 300, 512, 80, 5, 1)]


def case_table(cus):
    """every launch description the dispatch tests run, for a device of `cus` compute units (the persistent, wide and streaming
    kernels' tile-count thresholds are fractions of it)."""
    half, eighth = cus // 2, cus // 8
    T = []

    def add(family, dtype, Bq, S, Cin, N, taps, dil=1, pad=None, **kw):
        if pad is None:
            pad = (taps - 1) * dil // 2
        assert taps * Cin <= K_MAX and Cin % (8 if dtype == "bf16" else 4) == 0
        T.append(Launch(family, dtype, Bq, S, Cin, N, taps, dil, pad, **kw))

    # ---- single-utterance and small-batch synthesis
    for dtype in ("bf16", "fp32"):
        for Cin, Cout, k in MODEL_SHAPES:
            for S in (1, 7, 50, 127, 128, 129, 257, 800):
                add("single", dtype, 1, S, Cin, Cout, k)
            add("single", dtype, 3, 130, Cin, Cout, k)
    # ---- the STFT's framed DFT (hop 256, filter 1024: 4 taps, no padding, 2 x 513 columns into rows of 1028) and its inverse
    for Bq, S in ((1, 403), (2, 53)):
        add("stft", "fp32", Bq, S, 256, 1026, 4, pad=0)
        add("stft", "fp32", Bq, S - 3, 1028, 1024, 1)
    # ---- the op-level shapes of tests/test_ops_gpu.py
    for dtype in ("bf16", "fp32"):
        for Bq, S, Cin, Cout, k, dil in OPS_FWD_SHAPES + OPS_GRAD_SHAPES:
            add("ops13", dtype, Bq, S, Cin, Cout, k, dil)
    # ---- geometry edges, one factor at a time around (S = 129, Cin = 72, N = 80, 3 taps)
    for dtype in ("bf16", "fp32"):
        for M in (127, 128, 129, 255, 256, 257):
            add("edge", dtype, 1, M, 72, 80, 3)
        add("edge", dtype, 3, 85, 72, 80, 3)                      # M = 255 as three sequences
        add("edge", dtype, 2, 128, 72, 136, 3)                    # M = 256 as two
        for N in (1, 3, 8, 80, 127, 128, 129, 136, 1026):
            add("edge", dtype, 1, 129, 72, N, 3)
            add("edge", dtype, 2, 100, 64, N, 1)
        for Cin in (8, 24, 72, 80, 136) + ((4, 12) if dtype == "fp32" else ()):
            add("edge", dtype, 1, 129, Cin, 80, 3)
            add("edge", dtype, 1, 129, Cin, 129, 1)
        for taps in (1, 2, 3, 4, 9, 17, 32, 33):
            for pad in sorted({0, (taps - 1) // 2, taps - 1}):
                add("edge", dtype, 2, 131, 72, 80, taps, pad=pad)
        for dil, taps in ((3, 7), (5, 11)):                      # dilated, all three pads
            for pad in (0, (taps - 1) * dil // 2, (taps - 1) * dil):
                add("edge", dtype, 2, 131, 72, 80, taps, dil, pad)
        for S, taps, pad in ((2, 9, 4), (3, 9, 4), (3, 9, 8), (5, 9, 0), (1, 3, 1), (1, 9, 8), (8, 17, 16), (20, 33, 32)):   # S < taps, S < pad, S = 1
            add("edge", dtype, 130 // S + 1, S, 72, 80, taps, pad=pad)
        add("edge", dtype, 2, 300, 64, 72, 3, ldy_odd=True)       # vec_ok false where it does not move the dispatch
        add("edge", dtype, 2, 300, 64, 72, 3, out_shift=1)
        add("edge", dtype, 2, 300, 64, 72, 3, base_res=True, ldr_odd=True)
    # ---- one straddling pair per eligibility predicate
    def pair(label, side, *a, dtype="bf16", **kw):
        add("pair", dtype, *a, pair=label, side=side, **kw)
    rows = -(-half // 8)                                          # x 8 column tiles of 128 = at least cus / 2 tiles of 256 x 128
    for dtype in ("bf16", "fp32"):
        pair("dma: (taps-1)*dil <= 16", "a", 2, 300, 64, 72, 17, dtype=dtype)
        pair("dma: (taps-1)*dil <= 16", "b", 2, 300, 64, 72, 18, 1, 8, dtype=dtype)
        pair("dma: (taps-1)*dil <= 16 (two taps)", "a", 2, 300, 64, 72, 2, 16, 8, dtype=dtype)
        pair("dma: (taps-1)*dil <= 16 (two taps)", "b", 2, 300, 64, 72, 2, 17, 8, dtype=dtype)
    pair("ring: (taps-1)*dil <= 16", "a", 22, 256, 64, 1024, 17, lens=True)
    pair("ring: (taps-1)*dil <= 16", "b", 22, 256, 64, 1024, 18, 1, 8, lens=True)
    for C in (64, 32):
        pair(f"skinny<{C}>: (taps-1)*dil <= 64", "a", 2, 300, C, C, 5, 16)
        pair(f"skinny<{C}>: (taps-1)*dil <= 64", "b", 2, 300, C, C, 6, 13, 32)
        pair(f"skinny<{C}>: (taps-1)*dil <= 64 (two taps)", "a", 2, 300, C, C, 2, 64, 32)
        pair(f"skinny<{C}>: (taps-1)*dil <= 64 (two taps)", "b", 2, 300, C, C, 2, 65, 32)
        pair(f"skinny<{C}>: N == Cin", "a", 2, 300, C, C, 3)
        pair(f"skinny<{C}>: N == Cin", "b", 2, 300, C, C + 8, 3)
        pair(f"skinny<{C}>: taps <= 16", "a", 2, 300, C, C, 16)
        pair(f"skinny<{C}>: taps <= 16", "b", 2, 300, C, C, 17)
    pair("skinny: vec_ok (ldy)", "a", 2, 300, 64, 64, 3)
    pair("skinny: vec_ok (ldy)", "b", 2, 300, 64, 64, 3, ldy_odd=True)
    pair("skinny: vec_ok (ldr)", "a", 2, 300, 64, 64, 3, base_res=True)
    pair("skinny: vec_ok (ldr)", "b", 2, 300, 64, 64, 3, base_res=True, ldr_odd=True)
    add("pair", "bf16", 2, 300, 64, 64, 3, out_shift=1, note="vec_ok false by an unaligned out (the query takes no base address)")
    pair("persist: (taps-1)*dil <= 64", "a", rows, 256, 64, 1024, 5, 16)
    pair("persist: (taps-1)*dil <= 64", "b", rows, 256, 64, 1024, 6, 13, 32)
    pair("persist: Cin % 64 == 0", "a", rows, 256, 64, 1024, 3)
    pair("persist: Cin % 64 == 0", "b", rows, 256, 72, 1024, 3)
    pair("persist: N % 8 == 0", "a", rows, 256, 64, 1024, 3)
    pair("persist: N % 8 == 0", "b", rows, 256, 64, 1020, 3)
    pair("persist: taps >= 3", "a", rows, 256, 64, 1024, 3)
    pair("persist: taps >= 3", "b", rows, 256, 64, 1024, 2, 1, 1)
    pair("persist: taps <= 32", "a", rows, 256, 64, 1024, 32, 2, 31)
    pair("persist: taps <= 32", "b", rows, 256, 64, 1024, 33)
    pair("persist: lens needs tmap", "a", rows, 256, 64, 1024, 3, lens=True, tmap=True)
    pair("persist: lens needs tmap", "b", rows, 256, 64, 1024, 3, lens=True)
    pair("persist: vec_ok (ldy)", "a", rows, 256, 64, 1024, 3)
    pair("persist: vec_ok (ldy)", "b", rows, 256, 64, 1024, 3, ldy_odd=True)
    pair("persist: vec_ok (ldr)", "a", rows, 256, 64, 1024, 3, base_res=True)
    pair("persist: vec_ok (ldr)", "b", rows, 256, 64, 1024, 3, base_res=True, ldr_odd=True)
    add("pair", "bf16", rows, 256, 64, 1024, 3, out_shift=1, note="vec_ok false by an unaligned out (the query takes no base address)")
    pair("persist: tiles >= cus/2", "a", half, 256, 64, 128, 3)
    pair("persist: tiles >= cus/2", "b", half - 1, 256, 64, 128, 3)
    pair("persist one-tap: tiles >= cus/2", "a", half, 256, 256, 128, 1)
    pair("persist one-tap: tiles >= cus/2", "b", half - 1, 256, 256, 128, 1)
    pair("persist one-tap: Cin >= 256", "a", half, 256, 256, 128, 1)
    pair("persist one-tap: Cin >= 256", "b", half, 256, 192, 128, 1)
    pair("persist long_conv: taps*(Cin/64) >= 96", "a", eighth, 256, 1024, 128, 6)
    pair("persist long_conv: taps*(Cin/64) >= 96", "b", eighth, 256, 1216, 128, 5)
    pair("persist long_conv: tiles >= cus/8", "a", eighth, 256, 1024, 128, 6)
    pair("persist long_conv: tiles >= cus/8", "b", eighth - 1, 256, 1024, 128, 6)
    pair("dma ks2: Cin % 128 == 0", "a", 2, 300, 128, 136, 6)
    pair("dma ks2: Cin % 128 == 0", "b", 2, 300, 64, 136, 12)
    pair("dma ks2: taps*(Cin/64) >= 12", "a", 2, 300, 128, 136, 6)
    pair("dma ks2: taps*(Cin/64) >= 12", "b", 2, 300, 128, 136, 5)
    pair("dma ks2: taps*(Cin/64) >= 12", "b", 2, 300, 64, 136, 11)
    pair("dma ks2: grid <= 160", "a", 160, 128, 128, 128, 6)
    pair("dma ks2: grid <= 160", "b", 161, 128, 128, 128, 6)
    pair("dma one-tap: Cin >= 768 and Cin % 128 == 0", "a", 160, 128, 768, 128, 1)
    pair("dma one-tap: Cin >= 768 and Cin % 128 == 0", "b", 160, 128, 704, 128, 1)
    pair("dma one-tap: Cin >= 768 and Cin % 128 == 0", "b", 160, 128, 640, 128, 1)
    pair("dma one-tap: grid <= 160", "a", 160, 128, 768, 128, 1)
    pair("dma one-tap: grid <= 160", "b", 161, 128, 768, 128, 1)
    pair("ring: big_tiles >= 170", "a", 170, 256, 64, 128, 3, lens=True)
    pair("ring: big_tiles >= 170", "b", 169, 256, 64, 128, 3, lens=True)
    pair("ring one-tap: big_tiles >= 170", "a", 170, 256, 1024, 128, 1, lens=True)
    pair("ring one-tap: big_tiles >= 170", "b", 169, 256, 1024, 128, 1, lens=True)
    pair("ring one-tap: Cin >= 1024", "a", 170, 256, 1024, 128, 1, lens=True)
    pair("ring one-tap: Cin >= 1024", "b", 170, 256, 960, 128, 1, lens=True)
    pair("wide: tiles >= 96", "a", 96, 256, 128, 256, 1)
    pair("wide: tiles >= 96", "b", 95, 256, 128, 256, 1)
    pair("wide: N % 256 == 0", "a", 96, 256, 128, 256, 1)
    pair("wide: N % 256 == 0", "b", 96, 256, 128, 264, 1)
    pair("wide: vec_ok (ldy)", "a", 96, 256, 128, 256, 1)
    pair("wide: vec_ok (ldy)", "b", 96, 256, 128, 256, 1, ldy_odd=True)
    pair("stream: (tile, group) pairs >= cus", "a", cus, 64, 256, 256, 1)
    pair("stream: (tile, group) pairs >= cus", "b", cus - 1, 64, 256, 256, 1)
    pair("stream: Cin == 256", "a", cus, 64, 256, 256, 1)
    pair("stream: Cin == 256", "b", cus, 64, 320, 256, 1)
    pair("stream: vec_ok (ldy)", "a", cus, 64, 256, 256, 1)
    pair("stream: vec_ok (ldy)", "b", cus, 64, 256, 256, 1, ldy_odd=True)
    # ---- the stored-leaky-ReLU entry: with a residual / accumulate operand and a short reduction the ring kernel, else the persistent one
    pair("lrelu_io res_short: residual operand", "a", 170, 256, 128, 128, 3, base_res=True, io=(False, 10.0, 0.1))
    pair("lrelu_io res_short: residual operand", "b", 170, 256, 128, 128, 3, io=(False, 0.0, 0.1))
    pair("lrelu_io res_short: accumulate", "a", 170, 256, 128, 128, 3, io=(True, 0.0, 0.1))
    pair("lrelu_io res_short: accumulate", "b", 170, 256, 128, 128, 3, io=(False, 0.0, 0.1))
    pair("lrelu_io res_short: taps*(Cin/64) <= 48", "a", 170, 256, 192, 128, 16, base_res=True, io=(False, 10.0, 0.1))
    pair("lrelu_io res_short: taps*(Cin/64) <= 48", "b", 170, 256, 192, 128, 17, base_res=True, io=(False, 10.0, 0.1))
    seen, out = set(), []
    for c in T:                                                   # a description used by several pairs is run once per pair label
        key = (c.shape, c.dtype, c.family, c.pair, c.side)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out
