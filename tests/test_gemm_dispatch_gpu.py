"""Every contraction kernel fs2_conv_gemm can dispatch to, elementwise, at the small and odd shapes and ON the eligibility
boundaries of its dispatcher (conv_gemm_pick and fs2_conv_gemm_{s,w,p}_ok in fastspeech2_amd/csrc).

tests/test_a_prodshape_gpu.py pins the kernels at the train step's M = 44 400; everything under the tile-count thresholds
(single-utterance synthesis, the STFT's fp32 forms, the fallback kernels) and the thresholds themselves are pinned here, to the
same standard: the exact-product reference and the rounding-only bound of tests/gemm_ref.py (checked on the CPU by
tests/test_gemm_ref_cpu.py), per element.

  * coverage (no launch): the case table reaches all eight kernels, bf16 DMA with and without its in-workgroup K split, fp32 PLAIN
    and fp32 DMA, and every straddling pair lands on two different kernels - a pair that no longer splits names the predicate
    that moved;
  * elementwise: every description x every epilogue / operand form (FORMS below) and the data-gradient form (tap-flipped pack);
    test ids are variant-dtype-shape, so a failure names the kernel;
  * buffer guards: out is NaN-filled before a non-accumulating launch and sits inside a larger buffer whose guard columns
    (ldy > N) and guard rows hold a sentinel that must be bit-unchanged; x and res sit inside larger buffers whose surroundings
    are NaN, so any use of a row or column outside the operand shows in the result (rows >= lens INSIDE the operand stay finite:
    they are legitimately read);
  * argument checks that return before any launch.

Wall time on the MI355X, one pytest process each: this file 15 s (422 tests; about 10 800 launches, each with its fp64 reference);
tests/test_a_prodshape_gpu.py at the parent commit 38 s.  The epilogue rotation is therefore not thinned (THIN below).
Largest err / bound seen there per kernel (bf16 / fp32): plain 0.947 / 0.267, dma 0.944 / 0.398, dma+ks2 0.935, ring 0.929, skinny 0.930,
persist 0.934, persist one-tap 0.931, wide 0.929, stream 0.931, split-K 0.917 - in bf16 that is the final rounding itself (half a
spacing is up to 2^-8 |ref|), no kernel adds to it.
Environment: FS2_GEMM_DISPATCH_REPORT=<path> makes the last test write the per-variant table (cases, forms, largest err / bound) as JSON.
"""
import json
import math
import os

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

# THIN stays off: this file is the faster one, so the interior single-utterance cases keep the whole rotation
WALL_TIME = "MI355X, one pytest process each: this file 15 s (422 tests, 13.1 s in pytest); tests/test_a_prodshape_gpu.py at the parent commit 38 s"

F32, BF16 = 0, 1


def _lib():
    from fastspeech2_amd import _lib
    return _lib.load()


def _ops():
    from fastspeech2_amd import ops
    return ops


def _cus():
    """compute units of the device the kernels will run on (what the dispatcher's own thresholds use); 256 without one - ids only"""
    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(0).multi_processor_count
    return 256


def _dt(c):
    return BF16 if c.dtype == "bf16" else F32


def base_variant(c, lib=None):
    """the kernel the description itself dispatches to (its own lens / tile map / residual stride / row strides)"""
    lib = lib or _lib()
    ldr = c.ldr if c.base_res else 0
    if c.io:
        acc, unl, post = c.io
        return lib.fs2_conv_gemm_lrelu_io_variant(c.Cin, c.ldy, ldr, int(acc), c.M, c.N, c.Cin, c.S, c.taps, c.dil, 0, unl, post, _dt(c))
    return lib.fs2_conv_gemm_variant(c.Cin, c.ldy, ldr, int(c.lens), int(c.tmap), c.M, c.N, c.Cin, c.S, c.taps, c.dil, 0, 0.0, _dt(c))


def _name(v, c):
    return G.VARIANT_NAMES.get(v, str(v)) + ("+ks2" if v == G.DMA and c.ks2 else "")


TABLE = G.case_table(_cus())


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        k = (c.dtype, c.shape)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


RUN = _unique(TABLE)


def _id(c):
    try:
        v = base_variant(c)
    except Exception:                                               # (library not built: the ids only lose the kernel's name)
        v = 0
    return f"{_name(v, c)}{'?' if c.out_shift else ''}-{c.dtype}-{c.shape}"


# ------------------------------------------------------------------------------------------------------------------- coverage
def test_case_table_reaches_every_kernel_and_every_pair_splits(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus == _cus()
    _coverage(G.case_table(cus), _lib())


def _coverage(table, lib):
    got = {}
    for c in table:
        if c.out_shift:
            continue                                                # (the query assumes aligned bases)
        got.setdefault((base_variant(c, lib), c.dtype, c.ks2 if base_variant(c, lib) == G.DMA else None), []).append(c)
    codes = {k[0] for k in got}
    print("variants reached:", {G.VARIANT_NAMES[v]: sum(len(cs) for k, cs in got.items() if k[0] == v) for v in sorted(codes)})
    assert codes == {1, 2, 3, 4, 5, 6, 7, 9}, f"the table reaches {sorted(codes)}, not all eight kernels"
    assert (G.DMA, "bf16", True) in got and (G.DMA, "bf16", False) in got, "bf16 DMA is not reached both with and without ks2"
    assert (G.PLAIN, "fp32", None) in got and (G.DMA, "fp32", False) in got, "fp32 PLAIN / fp32 DMA not reached"
    assert (G.PLAIN, "bf16", None) in got
    pairs = {}
    for c in table:
        if c.pair:
            v = base_variant(c, lib)
            pairs.setdefault(c.pair, {"a": [], "b": []})[c.side].append((c, (v, c.ks2 if v == G.DMA else None)))
    assert len(pairs) >= 40
    unsplit = []
    for label, sides in sorted(pairs.items()):
        assert sides["a"] and sides["b"], label
        for ca, sa in sides["a"]:
            for cb, sb in sides["b"]:
                print(f"{label:55s} {ca.dtype} {ca.shape} -> {_name(sa[0], ca):10s} | {cb.shape} -> {_name(sb[0], cb)}")
                if sa == sb:
                    unsplit.append(f"predicate '{label}' no longer splits: {ca.shape} and {cb.shape} ({ca.dtype}) both go to {_name(sa[0], ca)}")
    assert not unsplit, "\n".join(unsplit)
    # the side that takes the kernel really takes the kernel the label names
    want = {"dma": G.DMA, "ring": G.RING, "skinny": G.SKINNY, "persist": None, "wide": G.WIDE_1TAP, "stream": G.STREAM_K256, "lrelu_io": G.RING}
    for label, sides in pairs.items():
        kernel = label.split(":")[0].split(" ")[0].split("<")[0]
        for ca, sa in sides["a"]:
            ok = sa[0] in (G.PERSIST, G.PERSIST_1TAP) if want[kernel] is None else sa[0] == want[kernel]
            assert ok, f"'{label}': {ca.shape} goes to {_name(sa[0], ca)}, not to the {kernel} kernel"
            if kernel == "dma" and "ks2" in label:
                assert ca.ks2 and not any(cb.ks2 for cb, _ in sides["b"]), label


# ---------------------------------------------------------------------------------------------------------------- elementwise
FORMS = ["bias_relu", "plain", "bias_lrelu", "bias_tanh", "res", "gate", "accumulate", "in_act", "x_strided", "lens", "lens_tmap", "tail_ws",
         "ksplit", "lrelu_io"]
THIN = False          # True: interior single-utterance cases keep bias_relu, res and lens only (see WALL_TIME); edges and pairs never thin
RAN_IDS = set()
STATS = {}            # "variant dtype" -> {"cases": set, "forms": set, "launches": int, "worst": float, "at": str}
SENTINEL = 7.0
GUARD = 72            # rows around every operand: more than the widest halo (65)


def _interior(c):
    return c.family == "single" and c.S in (50, 257, 800)


def _lens_sets(c, gen):
    """lens vectors with one full, one empty and one length-1 sequence (fewer than three sequences: one launch per rotation)"""
    if c.Bq >= 3:
        l = torch.randint(1, c.S + 1, (c.Bq,), generator=gen)
        l[0], l[1], l[2] = c.S, 0, 1
        return [l.to(torch.int32)]
    base = [c.S, 0, 1]
    return [torch.tensor([base[(i + r) % 3] for i in range(c.Bq)], dtype=torch.int32) for r in range(3)]


class _Case:
    """operands of one description on the device, embedded in guarded buffers"""

    def __init__(self, c, dev, seed):
        self.c, self.dev = c, dev
        self.dtype = G.DTYPES[c.dtype]
        g = self.gen = torch.Generator().manual_seed(seed)
        M = c.M
        self.x = torch.randn(M, c.Cin, generator=g).to(dev).to(self.dtype)
        self.w = (torch.randn(c.N, c.taps, c.Cin, generator=g) / math.sqrt(c.Cin * c.taps)).to(dev)     # fp32 master, tap-major
        self.bias = torch.randn(c.N, generator=g).to(dev)
        self.res = torch.randn(M, c.N, generator=g).to(dev).to(self.dtype)
        self.old = torch.randn(M, c.N, generator=g).to(dev).to(self.dtype)
        self.wf, self.wd = _ops().pack_weight(self.w, self.dtype, want_dgrad=c.N % c.epc == 0)
        self.wf = self.wf.contiguous().view(c.N, c.taps, c.Cin)
        self.lens_sets = [l.to(dev) for l in _lens_sets(c, g)]

    def embed(self, t, ld, col0=0, fill=float("nan")):
        """t inside a [GUARD + M + GUARD][ld] buffer of `fill`, at column col0"""
        M, C = t.shape
        buf = torch.full((M + 2 * GUARD, ld), fill, device=self.dev, dtype=t.dtype)
        view = buf[GUARD:GUARD + M, col0:col0 + C]
        view.copy_(t)
        return view

    def out_buffer(self, N, ldy, shift, old=None):
        """(flat buffer, [M][N] view at element offset `shift` + GUARD rows, snapshot): guard rows / columns hold SENTINEL, the
        result region NaN (or `old` for an accumulating launch)"""
        M = self.c.M
        flat = torch.full(((M + 2 * GUARD) * ldy + 16,), SENTINEL, device=self.dev, dtype=self.dtype)
        view = flat[shift:shift + (M + 2 * GUARD) * ldy].view(M + 2 * GUARD, ldy)[GUARD:GUARD + M, :N]
        if old is None:
            view.fill_(float("nan"))
        else:
            view.copy_(old)
        return flat, view, flat.clone()

    @staticmethod
    def guards_intact(flat, view, before):
        after = flat.clone()
        mask = torch.zeros_like(flat, dtype=torch.bool)
        mv = mask[view.storage_offset():].as_strided(view.shape, view.stride())
        mv.fill_(True)
        it = torch.int16 if flat.dtype == torch.bfloat16 else torch.int32
        return torch.equal(after.view(it)[~mask], before.view(it)[~mask])


def _record(vname, c, form, ratio, cid):
    s = STATS.setdefault(vname, {"cases": set(), "forms": set(), "launches": 0, "worst": 0.0, "at": ""})
    s["cases"].add(cid)
    s["forms"].add(form)
    s["launches"] += 1
    if ratio > s["worst"]:
        s["worst"], s["at"] = ratio, f"{cid} [{form}]"


def _run_form(k, form, cid, lens=None, dgrad=False):
    """one launch of description k.c in `form`, checked against the reference.  Returns False if the API documents the form as
    illegal for the description (nothing launched)."""
    c, ops, lib, dev, dtype = k.c, _ops(), _lib(), k.dev, k.dtype
    M, S, dil = c.M, c.S, c.dil
    if dgrad:
        if c.N % c.epc:
            return False                                            # (the data gradient's Cin is N: not a multiple of 16 bytes - FS2_EINVAL)
        x, w, N, Cin, pad = k.old, k.wd.contiguous().view(c.Cin, c.taps, c.N), c.Cin, c.N, (c.taps - 1) * dil - c.pad
        wref = G.dgrad_weight(k.wf)
        assert torch.equal(w, wref), "fs2_pack_weight's data-gradient pack is not the tap-flipped transpose"
        res_full = k.x
    else:
        x, w, N, Cin, pad, wref, res_full = k.x, k.wf, c.N, c.Cin, c.pad, k.wf, k.res
    epc = c.epc
    ldy = (N + epc - 1) // epc * epc + epc + (1 if c.ldy_odd else 0)
    ldr = (N + epc - 1) // epc * epc + epc + (1 if c.ldr_odd else 0)
    kw = dict(act=ops.ACT_NONE, slope=0.0, in_act=ops.ACT_NONE, in_slope=0.0, out_scale=1.0, res_unlrelu=0.0, post_slope=0.0)
    bias, use_res, acc, tmap, tail, ksplit = k.bias[:N] if not dgrad else None, c.base_res, False, False, False, 1
    if lens is None and c.lens:
        lens = k.lens_sets[0]
        tmap = c.tmap
    ldx, col0 = Cin, 0
    if form == "bias_relu":
        kw.update(act=ops.ACT_RELU)
    elif form == "plain":
        bias = None
    elif form == "bias_lrelu":
        kw.update(act=ops.ACT_LRELU, slope=0.1)
    elif form == "bias_tanh":
        kw.update(act=ops.ACT_TANH)
    elif form == "res":
        use_res = True
    elif form == "gate":
        bias, use_res = None, True
        kw.update(act=ops.ACT_GATE)
    elif form == "accumulate":
        acc = True
        kw.update(out_scale=1.0 / 3)
    elif form == "in_act":
        kw.update(in_act=ops.ACT_LRELU, in_slope=0.1)
    elif form == "x_strided":
        kw.update(act=ops.ACT_RELU)
        ldx, col0 = Cin + 24, 8
    elif form == "lens":
        kw.update(act=ops.ACT_RELU)
        tmap = False
    elif form == "lens_tmap":
        kw.update(act=ops.ACT_RELU)
        tmap = True
    elif form == "tail_ws":
        kw.update(act=ops.ACT_RELU)
        tail = True
    elif form == "ksplit":
        use_res, ksplit = True, 2
        # fs2_conv_gemm_splitk's documented domain: bf16, Cin % (64 ksplit) == 0, N % 8 == 0, 16-byte rows, lens only with a tile map
        if c.dtype != "bf16" or Cin % 128 or N % 8 or c.ldy_odd or c.ldr_odd or c.out_shift or (lens is not None and not tmap):
            return False
    elif form == "lrelu_io":
        use_res = True
        kw.update(out_scale=1.0 / 3, res_unlrelu=10.0, post_slope=0.1)
        lens = None
    elif form == "io_base":                                          # the description's own fs2_conv_gemm_lrelu_io launch
        acc, unl, post = c.io
        kw.update(res_unlrelu=unl, post_slope=post, out_scale=1.0 / 3)
        lens = None
    else:
        raise ValueError(form)
    if dgrad:
        bias = None
    xv = k.embed(x, ldx, col0)
    rv = k.embed(res_full, ldr) if use_res else None
    old = (k.old if not dgrad else k.x) if acc else None
    flat, yv, before = k.out_buffer(N, ldy, c.out_shift, old)
    lens_d = lens
    tm = ops.tile_map(lens_d, c.Bq, S) if (tmap and lens_d is not None) else None
    tws = ops.tail_workspace(dev).fill_(float("nan")) if tail else None
    ws = torch.full((ksplit, M, N), float("nan"), device=dev) if ksplit > 1 else None
    io = bool(kw["res_unlrelu"] or kw["post_slope"])
    # which kernel this launch goes to
    if ksplit > 1:
        var = G.PERSIST if c.taps > 1 else G.PERSIST_1TAP
    elif io:
        var = lib.fs2_conv_gemm_lrelu_io_variant(ldx, ldy, ldr if use_res else 0, int(acc), M, N, Cin, S, c.taps, dil, kw["act"],
                                                 kw["res_unlrelu"], kw["post_slope"], _dt(c))
    else:
        var = lib.fs2_conv_gemm_variant(ldx, ldy, ldr if use_res else 0, int(lens_d is not None), int(tm is not None), M, N, Cin, S, c.taps,
                                        dil, kw["in_act"], kw["in_slope"], _dt(c))
    vname = G.VARIANT_NAMES[var] + ("+ks2" if var == G.DMA and G.ks2(c.dtype, M, N, Cin, c.taps) else "")
    if ksplit > 1:
        vname += "(splitk)"
    if c.out_shift:
        vname = "unaligned-out"
    try:
        got = ops.conv_gemm(xv, w, bias, S, taps=c.taps, dil=dil, pad=pad, lens=lens_d, res=rv, out=yv, accumulate=acc, tmap=tm,
                            ksplit=ksplit, ws=ws, tail_ws=tws, **kw)
    except ValueError as e:
        if ksplit > 1 and "shape not supported" in str(e):
            return False                                            # FS2_EINVAL before any launch: "the caller falls back to fs2_conv_gemm"
        raise
    assert got.data_ptr() == yv.data_ptr()
    ref = G.conv_reference(x, wref, bias, S, dil=dil, pad=pad, lens=lens_d, res=(res_full if use_res else None), old=old, **kw)
    what = (cid, "dgrad" if dgrad else "fwd", form, vname)
    ratio = G.rounding_ratio(yv, ref, dtype)
    print(f"{cid} {'dgrad ' if dgrad else ''}{form} -> {vname}: err/bound {ratio:.3f}")
    G.assert_rounding_only(yv, ref, dtype, what)
    if lens_d is not None and not acc:
        assert (yv[G.pad_rows(lens_d, c.Bq, S, dev)] == 0).all(), (what, "rows >= lens are not exact zeros")
    assert k.guards_intact(flat, yv, before), (what, "guard rows / columns of out were written")
    _record(f"{vname} {c.dtype}", c, ("dgrad:" if dgrad else "") + form, ratio, cid)
    RAN_IDS.add(cid)
    return True


@pytest.mark.parametrize("c", RUN, ids=_id)
def test_every_form_elementwise(dev, c):
    cid = _id(c)
    k = _Case(c, dev, seed=sum(ord(ch) for ch in c.shape + c.dtype))
    forms = ["io_base"] + FORMS if c.io else FORMS
    if THIN and _interior(c):
        forms = ["bias_relu", "res", "lens"]
    ran = []
    for form in forms:
        sets = k.lens_sets if form in ("lens", "lens_tmap") else [None]
        for lens in sets:
            if _run_form(k, form, cid, lens=lens):
                ran.append(form)
    # every form but the split-K entry is legal for every description
    assert set(ran) >= set(forms) - {"ksplit"}, set(forms) - set(ran)
    if c.edge:
        for form in ("plain", "res", "gate", "lens_tmap"):           # the data gradient as the engine launches it
            for lens in (k.lens_sets if form == "lens_tmap" else [None]):
                _run_form(k, form, cid, lens=lens, dgrad=True)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_before_any_launch(dev):
    ops = _ops()
    x = torch.zeros(64, 64, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(16, 1, 64, device=dev, dtype=torch.bfloat16)
    y = torch.full((64, 16), 5.0, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.conv_gemm(x, w, None, 48, out=y)                                    # M % S != 0
    with pytest.raises(ValueError):
        ops.conv_gemm(x[:, :60], w[:, :, :60], None, 64, out=y, Cin=60)        # bf16 Cin not a multiple of 8
    xf, wf, yf = x.float(), w.float(), y.float()
    with pytest.raises(ValueError):
        ops.conv_gemm(xf[:, :62], wf[:, :, :62], None, 64, out=yf, Cin=62)     # fp32 Cin not a multiple of 4
    with pytest.raises(ValueError):
        ops.conv_gemm(x, w, None, 64, out=y, res_unlrelu=10.0)                 # res_unlrelu without res
    torch.cuda.synchronize()
    assert (y == 5.0).all() and (yf == 5.0).all()                              # nothing was launched


def test_constants_match_the_library():
    ops = _ops()
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH, ops.ACT_LRELU, ops.ACT_GATE) == (G.ACT_NONE, G.ACT_RELU, G.ACT_TANH, G.ACT_LRELU, G.ACT_GATE)
    assert (ops.F32, ops.BF16) == (F32, BF16)


def test_zz_report_per_variant_table(dev):
    """not a check of the kernels: prints (and optionally writes) what the elementwise tests of this session covered"""
    rows = []
    for v, s in sorted(STATS.items()):
        rows.append({"variant": v, "cases": len(s["cases"]), "forms": len(s["forms"]), "launches": s["launches"], "worst": s["worst"], "at": s["at"]})
        print(f"{v:22s} cases {len(s['cases']):4d}  forms {len(s['forms']):3d}  launches {s['launches']:5d}  worst err/bound {s['worst']:.3f}  at {s['at']}")
    path = os.environ.get("FS2_GEMM_DISPATCH_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)
    if len(RAN_IDS) == len(RUN):                                    # the whole file ran in this process: every kernel was LAUNCHED
        ran = {v.split(" ")[0].split("+")[0].split("(")[0] for v in STATS}
        assert ran >= set(G.VARIANT_NAMES.values()), ran
        assert {"dma+ks2 bf16", "dma bf16", "dma fp32", "plain fp32", "plain bf16"} <= set(STATS) and any("(splitk)" in v for v in STATS)
