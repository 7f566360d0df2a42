"""Attention kernels (fs2_attn_fwd / fs2_attn_bwd, bf16 and fp32) elementwise against the fp64 reference of tests/attn_ref.py
at every tile edge and score regime: each valid element of ctx, dq, dk, dv within c * u * mag of the reference (a running-
error bound, not a max- or norm-normalised one), lse within LSE_TOL (1 + |lse|), rows >= len of dqkv exactly 0.

What the kernels do only at edges, and where it is reached here:
  * lengths: every residue of len mod 8 / 32 / 64 / 128 (partial and fully padded 128-query tiles, the last-tile key mask of the
    forward, dQ's masked 32-key block with its threshold len - k0 - 32 kb - 4 h2 and its `break` on fully padded blocks), empty
    sequences, lens = None, S from 1 to max_seq_len;
  * scores: flat, peaked, and rising / falling keys, where the bf16 forward's lazy running maximum must be raised (and the
    accumulators rescaled) in later tiles for some queries of a wave and not for others;
  * padding: rows [len, S) of K / V are really read (tiles are clamped to row S-1, not zero-filled) and are poisoned so that a
    leaked key dominates the softmax, or so that its probability overflows fp32;
  * the XCD-aware block map at 1 .. 17 (sequence, head) pairs of 1, 2 and 8 tiles, H = 1 and 3;
  * every output written (NaN-filled outputs and scratch), two calls bit-identical;
  * the production batch (B = 48, S = 925, ragged lens) in bf16.
Each test prints the observed maxima of err / (u mag) ("attn-bound" lines) - the margin under attn_ref.C."""
import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float32, id="fp32")]


def _ops():
    from fastspeech2_amd import ops
    return ops


def _report(what, dtype, r):
    print(f"attn-bound {'bf16' if dtype == torch.bfloat16 else 'fp32'} {what}: "
          + " ".join(f"{k} {v:.3g}" for k, v in r.items()))


def _run_check(dev, B, S, H, lens, dtype, seed, regime="randn", pad="leak", what=""):
    """one forward + backward through ops on make_inputs data, every bound checked; returns the ratios"""
    ops = _ops()
    qkv, dctx = A.make_inputs(B, S, H, lens, dtype, dev, seed, regime=regime, pad=pad)
    ld = None if lens is None else lens.to(dev)
    ctx, lse = ops.attn_fwd(qkv, ld, B, S, H)
    dqkv = ops.attn_bwd(qkv, ctx, dctx, lse, ld, B, S, H)
    ref = A.reference(qkv, lens, B, S, H, dctx)
    r = A.check_all(ref, ctx, lse, dqkv, dtype, H, what=what)
    for b, n in enumerate(ref["lens"]):
        if n == 0:                                                 # an empty sequence: exact zeros (and a finite lse: check_all)
            assert not ctx[b * S:(b + 1) * S].any(), (what, "ctx of an empty sequence", b)
    _report(what, dtype, r)
    return r


# ------------------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_length_at_S200(dev, dtype):
    """one batch holding every length 1 .. 200 and an empty sequence, H = 2; and the same S without lens"""
    S, H = 200, 2
    lens = torch.tensor(list(range(S, 0, -1)) + [0], dtype=torch.int32)
    _run_check(dev, len(lens), S, H, lens, dtype, seed=100, what="S=200 every len")
    _run_check(dev, 2, S, H, None, dtype, seed=101, what="S=200 lens=None")


@pytest.mark.parametrize("S", [1, 2, 31, 64, 129, 257, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lengths_at_tile_edges(dev, dtype, S):
    cand = [S, S - 1, S - 2, S // 2 + 1, 128, 127, 65, 64, 63, 33, 32, 31, 9, 8, 7, 1, 0]
    lens = torch.tensor(sorted({n for n in cand if 0 <= n <= S}, reverse=True), dtype=torch.int32)
    _run_check(dev, len(lens), S, 2, lens, dtype, seed=200 + S, what=f"S={S} edges")


# ------------------------------------------------------------------------------------------------------------ score regimes
@pytest.mark.parametrize("B,S,lens", [(4, 257, [257, 200, 129, 64]), (2, 1000, [1000, 700])])
@pytest.mark.parametrize("regime", ["randn", "flat", "peaked", "rising"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_regimes(dev, dtype, regime, B, S, lens):
    _run_check(dev, B, S, 2, torch.tensor(lens, dtype=torch.int32), dtype, seed=300 + S, regime=regime, pad="randn",
               what=f"{regime} S={S}")


# ------------------------------------------------------------------------------------------------------------ poisoned padding
@pytest.mark.parametrize("pad", ["leak", "overflow"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_padding(dev, dtype, pad):
    """rows [len, S) of K score PAD_LEAK_SCORE above the valid keys (a leaked key is an O(100) error: V there is ~1e2), or
    PAD_OVERFLOW_SCORE - far enough above a valid query's lse that exp overflows fp32: the kernels' contract (rows >= len:
    only finiteness matters) still gives a masked key exactly nothing and its dK / dV rows exact zeros"""
    S = 300
    lens = torch.tensor([300, 299, 257, 256, 200, 193, 129, 128, 127, 64, 33, 1, 0], dtype=torch.int32)
    _run_check(dev, len(lens), S, 2, lens, dtype, seed=400, pad=pad, what=f"padding {pad}")


# ------------------------------------------------------------------------------------------------------------ writes / reads
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_output_written_no_scratch_read(dev, dtype):
    """ctx, lse, dqkv and the delta scratch NaN-filled before the calls: everything comes out finite, dqkv rows >= len exactly
    0, identical to the ops.* results; a second call is bit-identical (no atomics anywhere)"""
    from fastspeech2_amd import _lib
    ops = _ops()
    B, S, H = 5, 300, 2
    lens = torch.tensor([300, 257, 130, 1, 0], dtype=torch.int32)
    ld = lens.to(dev)
    qkv, dctx = A.make_inputs(B, S, H, lens, dtype, dev, seed=500, pad="leak")
    nan = float("nan")

    def raw():
        ctx = torch.full((B * S, H * A.DK), nan, device=dev, dtype=dtype)
        lse = torch.full((B, H, S), nan, device=dev)
        _lib.call("fs2_attn_fwd", ops._p(qkv), ops._p(ctx), ops._p(lse), ops._p(ld), B, S, H, A.DK, A.DK ** -0.5, ops.dt(qkv),
                  ops._stream())
        dqkv = torch.full_like(qkv, nan)
        delta = torch.full((B, H, S), nan, device=dev)
        _lib.call("fs2_attn_bwd", ops._p(qkv), ops._p(ctx), ops._p(dctx), ops._p(lse), ops._p(delta), ops._p(dqkv), ops._p(ld),
                  B, S, H, A.DK, A.DK ** -0.5, ops.dt(qkv), ops._stream())
        return ctx, lse, dqkv

    ctx, lse, dqkv = raw()
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    valid = (torch.arange(S, device=dev).unsqueeze(0) < ld.unsqueeze(1)).reshape(-1)
    assert not dqkv[~valid].any()
    c2, l2 = ops.attn_fwd(qkv, ld, B, S, H)
    assert torch.equal(ctx, c2) and torch.equal(lse, l2)
    assert torch.equal(dqkv, ops.attn_bwd(qkv, c2, dctx, l2, ld, B, S, H))
    c3, l3, d3 = raw()
    assert torch.equal(ctx, c3) and torch.equal(lse, l3) and torch.equal(dqkv, d3)
    ref = A.reference(qkv, lens, B, S, H, dctx)
    _report("NaN-filled outputs", dtype, A.check_all(ref, ctx, lse, dqkv, dtype, H, what="NaN-filled outputs"))


# ------------------------------------------------------------------------------------------------------------ block map
PAIRS = {1: (1, 1), 3: (1, 3), 7: (7, 1), 8: (8, 1), 9: (3, 3), 17: (17, 1)}       # (sequence, head) pairs -> (B, H)


@pytest.mark.parametrize("S", [100, 200, 1000])                                 # 1, 2 and 8 tiles per pair
@pytest.mark.parametrize("pairs", sorted(PAIRS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_block_map_pair_counts(dev, dtype, pairs, S):
    B, H = PAIRS[pairs]
    g = torch.Generator().manual_seed(600 + 31 * pairs + S)
    lens = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = S
    _run_check(dev, B, S, H, lens, dtype, seed=601 + pairs * S, what=f"{pairs} pairs S={S} H={H}")


# ------------------------------------------------------------------------------------------------------------ production
def test_production_batch_bf16_elementwise(dev):
    """B = 48, S = 925 with the ragged lens of the production-shape tests, bf16, every valid element of ctx / lse / dq / dk / dv
    (test_a_prodshape_gpu.py::test_attention_backward_bf16_at_full_length checks 8 sequences by rel-Frobenius norm)"""
    from tests.test_a_prodshape_gpu import B, ragged_lens
    S = 925
    _run_check(dev, B, S, 2, ragged_lens(S), torch.bfloat16, seed=700, pad="leak", what="B=48 S=925")
