"""CPU: the C-ABI library loads without a GPU and exports every symbol include/fs2hip.h declares (no compute
calls); argument validation returns the documented error codes before any launch."""
import ctypes
import os
import re
import subprocess

import pytest

from fastspeech2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    protos = _lib.parse_header()
    assert len(protos) >= 33
    for name in protos:
        assert hasattr(lib, name), name
    # and nothing the header promises is missing from the dynamic symbol table
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\b(fs2_\w+)\b", out))
    assert set(protos) <= exported
    # every exported fs2_* entry point is declared (no undocumented ABI)
    undeclared = {s for s in exported if not s.startswith("fs2_set_error")} - set(protos)
    assert not undeclared, undeclared


def test_version_and_error_string():
    lib = _lib.load()
    assert lib.fs2_version() >= 100
    assert isinstance(lib.fs2_last_error(), bytes)


def test_bad_arguments_are_rejected_before_launch():
    """FS2_EINVAL (-1) -> ValueError, FS2_EDTYPE (-2) -> TypeError: mirrors the reference's assert/ValueError style."""
    with pytest.raises(ValueError):
        _lib.call("fs2_conv_gemm", None, 0, None, None, None, 0, None, 0, None, None, 0, 0, 0, 0, 1, 1, 0, 0, 0.0, 0, 0.0, 0, 1.0,
                  0, None)
    with pytest.raises((TypeError, ValueError)):
        _lib.call("fs2_cast", None, 7, None, 9, 16, None)


def test_header_is_plain_c():
    """include/fs2hip.h must compile as C (extern "C" boundary, no C++/torch types)."""
    src = '#include "fs2hip.h"\nint main(void){return fs2_version()>0?0:1;}\n'
    p = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_product_forward_refuses_cpu_tensors():
    import torch
    from tests.golden import configs
    from fastspeech2_amd.model import FastSpeech2

    pcfg, mcfg = configs.make(dec_layers=1, enc_layers=1)
    m = FastSpeech2(pcfg, mcfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, dtype=torch.long), torch.ones(1, 4, dtype=torch.long), torch.tensor([4]), 4)


def test_dispatch_queries_are_pure_host_functions():
    """fs2_conv_gemm_variant / fs2_conv_gemm_lrelu_io_variant answer without a device (bench.py attributes its HIP-event durations
    to kernel names with them): HiFi-GAN's stored-leaky-ReLU launches with a residual / accumulate operand and a short reduction
    go to the ring kernel (3), the same shapes without one to the persistent kernel (5); the FFN convolution stays on 5."""
    lib = _lib.load()
    BF16 = 1
    for (B, S, C, k) in [(4, 12000, 128, 7), (8, 5600, 256, 11), (4, 12000, 128, 3)]:
        M = B * S
        assert lib.fs2_conv_gemm_lrelu_io_variant(C, C, C, 0, M, C, C, S, k, 1, 0, 10.0, 0.1, BF16) == 3
        assert lib.fs2_conv_gemm_lrelu_io_variant(C, C, 0, 1, M, C, C, S, k, 1, 0, 0.0, 0.1, BF16) == 3
        assert lib.fs2_conv_gemm_lrelu_io_variant(C, C, 0, 0, M, C, C, S, k, 1, 0, 0.0, 0.1, BF16) == 5
    assert lib.fs2_conv_gemm_variant(256, 1024, 0, 0, 0, 48 * 925, 1024, 256, 925, 9, 1, 0, 0.0, BF16) == 5
    assert lib.fs2_conv_gemm_variant(256, 768, 0, 0, 0, 48 * 925, 768, 256, 925, 1, 1, 0, 0.0, BF16) == 9


# The dispatch of every contraction the bench runs, recorded before tests/test_gemm_dispatch_gpu.py was added: a predicate narrowed
# for a small or odd shape must leave these where they are.  (name, Cin, Cout, k, S, codes) at M = 48 S; codes: bf16 then fp32, each
# forward (Cin -> Cout) then data gradient (Cout -> Cin), each without lens / with lens / with lens and tile map.  256 compute
# units: the library's answer without a device, and the MI355X's.
BENCH_DISPATCH = [
    ("ffn w_1 k9", 256, 1024, 9, 925, (5, 3, 5, 5, 3, 5, 2, 2, 2, 2, 2, 2)),
    ("ffn w_2 k1", 1024, 256, 1, 925, (7, 7, 7, 9, 9, 9, 1, 1, 1, 1, 1, 1)),
    ("qkv", 256, 768, 1, 925, (9, 9, 9, 7, 7, 7, 1, 1, 1, 1, 1, 1)),
    ("fc", 256, 256, 1, 925, (9, 9, 9, 9, 9, 9, 1, 1, 1, 1, 1, 1)),
    ("postnet k5", 512, 512, 5, 925, (5, 3, 5, 5, 3, 5, 2, 2, 2, 2, 2, 2)),
    ("postnet in", 80, 512, 5, 925, (2, 2, 2, 5, 3, 5, 2, 2, 2, 2, 2, 2)),
    ("postnet out", 512, 80, 5, 925, (5, 3, 5, 2, 2, 2, 2, 2, 2, 2, 2, 2)),
    ("mel", 256, 80, 1, 925, (6, 1, 6, 1, 1, 1, 1, 1, 1, 1, 1, 1)),
    ("enc w_1 k9", 256, 1024, 9, 128, (5, 3, 5, 5, 2, 5, 2, 2, 2, 2, 2, 2)),
    ("predictor k3", 256, 256, 3, 128, (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2)),
]
# the bf16 vocoder at batch-synthesis size (C, N, k, dil, S, B): (leaky-ReLU prologue, residual operand) -> code
VOCODER_DISPATCH = [
    (256, 256, 7, 3, 7200, 8, (5, 5)), (128, 128, 11, 5, 57600, 4, (5, 5)), (128, 128, 3, 1, 57600, 4, (5, 5)), (256, 256, 11, 1, 7200, 8, (5, 5)),
    (512, 2048, 3, 1, 900, 8, (5, 5)), (256, 1024, 3, 1, 7200, 8, (5, 5)), (128, 128, 3, 1, 57600, 8, (5, 5)),
    (64, 64, 3, 1, 115200, 8, (4, 4)), (64, 64, 7, 3, 115200, 8, (4, 4)), (64, 64, 11, 5, 115200, 8, (4, 4)),
    (32, 32, 3, 1, 230400, 8, (4, 4)), (32, 32, 7, 3, 230400, 8, (4, 4)), (32, 32, 11, 5, 230400, 8, (4, 4)),
]


def test_dispatch_of_the_bench_and_vocoder_shapes_is_pinned():
    lib = _lib.load()
    for name, Cin, Cout, k, S, codes in BENCH_DISPATCH:
        M = 48 * S
        got = tuple(lib.fs2_conv_gemm_variant(ci, co, 0, hl, hm, M, co, ci, S, k, 1, 0, 0.0, dt)
                    for dt in (1, 0) for ci, co in ((Cin, Cout), (Cout, Cin)) for hl, hm in ((0, 0), (1, 0), (1, 1)))
        assert got == codes, (name, got, codes)
    for C, N, k, dil, S, B, codes in VOCODER_DISPATCH:
        M = B * S
        got = (lib.fs2_conv_gemm_variant(C, N, 0, 0, 0, M, N, C, S, k, dil, 3, 0.1, 1), lib.fs2_conv_gemm_variant(C, N, N, 0, 0, M, N, C, S, k, dil, 0, 0.0, 1))
        assert got == codes, ((C, N, k, dil, S, B), got, codes)


def test_no_copy_of_an_in_flight_fragment_register_in_the_persistent_kernel():
    """The persistent contraction kernel tracks its LDS fragment reads by hand (inline-asm ds_read_b128 + counted lgkmcnt); the
    compiler does not know that such a register may still be in flight, so a register-to-register copy of one between its read and
    the wait that lands it carries stale data (round 6: the eight-consumer-wave form came out 1 % wrong, timing-dependent, when its
    K loop was two nested loops).  tools/check_frag_copies.py compiles the kernel to ISA and lists such copies: there must be none."""
    import shutil
    import subprocess
    import sys
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_frag_copies.py"), os.path.join(ROOT, "fastspeech2_amd", "csrc", "fs2_gemm_p.hip")],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "conv_gemm_p_kernel<false, false, 0, 8>" in r.stdout and "conv_gemm_p_kernel<false, false, 0, 4>" in r.stdout
