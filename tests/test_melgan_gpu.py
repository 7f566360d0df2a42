"""GPU: fastspeech2_amd.melgan.Generator against the fp64 restatement of the published network (tests/melgan_ref.py), random weights.

Shapes (B, T) = (1, 4), (3, 5), (2, 9), (1, 37).  The fused narrow stages output R = E - 26 rows per tile (C = 64: E = 256, R = 230 on
S = 128 T rows; C = 32: E = 512, R = 486 on S = 256 T rows):
  T = 4   the smallest legal input - every reflection of conv 1 is active; 512 / 1024 rows = 3 tiles each, 52-row last tiles;
  T = 5   B = 3 (an item between two others); 640 / 1280 rows, short last tiles of 180 / 308 rows;
  T = 9   1152 = 5 x 230 + 2: the C = 64 stage ends in a TWO-row tile whose reflected rows all lie in its halo; 2304 = 4 x 486 + 360;
  T = 37  21 / 20 tiles: the dilation-9 halo crosses interior tile edges while both ends reflect.
The bars come from tests/golden/melgan_bars.json (made on the CPU by make_melgan_bars.py from the number formats alone)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from tests import melgan_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "melgan_bars.json")))["shapes"]


@functools.lru_cache(maxsize=None)
def case(B, T):
    """seed-0 weights and input of a shape + the fp64 answer per stage (computed once per session, never modified)"""
    sd, x = R.make_case(0, B, T)
    with torch.no_grad():
        exact = R.forward(R.plain_weights(sd), x.double())
    return sd, x, exact


def make_gen(sd, dev, cdt, fuse=True):
    from fastspeech2_amd import melgan
    gen = melgan.Generator(compute_dtype=cdt)
    gen.load_state_dict(sd)
    gen.eval()
    gen.remove_weight_norm()
    gen.to(dev)
    gen.fuse_stages = fuse
    return gen


def run_probed(gen, x, dev):
    gen.stage_probe = []
    with torch.no_grad():
        wav = gen(x.to(dev))
    torch.cuda.synchronize()
    probe, gen.stage_probe = gen.stage_probe, None
    out = {name: rows.transpose(1, 2).cpu() for name, (rows, S) in zip(R.STAGES[:-1], probe)}      # (B, S, C) rows -> (B, C, S)
    out["wav"] = wav.squeeze(1).cpu()
    return out


@pytest.mark.parametrize("cdt,fuse", [("fp32", False), ("bf16", True), ("bf16", False)])
@pytest.mark.parametrize("B,T", R.SHAPES)
def test_generator_matches_fp64_restatement_per_stage(dev, B, T, cdt, fuse):
    sd, x, exact = case(B, T)
    got = run_probed(make_gen(sd, dev, cdt, fuse), x, dev)
    bars = BARS[f"{B}x{T}"][cdt]
    assert got["wav"].shape == (B, 256 * T) and got["wav"].abs().max() <= 1.0
    errs = {s: R.rel(got[s], exact[s]) for s in R.STAGES}
    print(f"B={B} T={T} {cdt} fuse={fuse}: " + "  ".join(f"{s} {errs[s]:.2e} (bar {bars[s]['bar']:.2e})" for s in R.STAGES))
    for s in R.STAGES:
        assert got[s].shape == exact[s].shape, s
        assert errs[s] <= bars[s]["bar"], (s, errs[s], bars[s]["bar"])


def _stage_chain(x, w3, b3, w11, b11, B, S, C, G=9):
    """a stage's three ResnetBlocks as melgan.Generator._run's chain of single launches; x (B, S, C) bf16 -> (B, S, C) raw"""
    from fastspeech2_amd import ops
    cat = [torch.empty(B, S + 2 * G, 2 * C, device=x.device, dtype=x.dtype) for _ in range(2)]
    out = torch.empty(B, S + 2 * G, C, device=x.device, dtype=x.dtype)
    ops.melgan_guard_rows(x, cat[0][:, :, :C], G, reflect=True, interior=True)
    for j, d in enumerate((1, 3, 9)):
        cur = cat[j % 2]
        cur2 = cur.view(-1, 2 * C)
        if j > 0:
            ops.melgan_guard_rows(cur[:, G:G + S, :C], cur[:, :, :C], G, reflect=True, interior=False)
        ops.conv_gemm(cur2, w3[j], b3[j], S + 2 * G, taps=3, dil=d, pad=d, act=ops.ACT_LRELU, slope=0.2, in_act=ops.ACT_LRELU, in_slope=0.2,
                      Cin=C, out=cur2[:, C:])
        dst = out.view(-1, C) if j == 2 else cat[(j + 1) % 2].view(-1, 2 * C)[:, :C]
        ops.conv_gemm(cur2, w11[j], b11[j], S + 2 * G, taps=1, out=dst)
    return out[:, G:G + S]


# S at the tile edges of the fused kernel (R = 230 rows per tile at C = 64, 486 at C = 32): the smallest S it takes, one row less than /
# exactly / one row more than a tile, two tiles + less than a dilation-9 reach, several tiles
@pytest.mark.parametrize("C,S", [(64, 32), (64, 229), (64, 230), (64, 231), (64, 467), (64, 1000),
                                 (32, 32), (32, 486), (32, 487), (32, 979), (32, 1500)])
def test_fused_stage_matches_single_launch_chain_and_exact(dev, C, S):
    """fs2_melgan_stage_fwd against (a) the same three blocks as single launches over reflection guard rows and (b) fp64 on the same
    bf16 input and weights.  The fused stage rounds what the chain rounds except the value between blocks, which it keeps in fp32: it
    may not be further from the exact result than the chain is (the form of test_resblock_fused_matches_convolution_chain_and_exact)."""
    from fastspeech2_amd import ops
    B = 2
    g = torch.Generator().manual_seed(C * 10000 + S)
    x = (torch.randn(B, S, C, generator=g) * 0.7).to(torch.bfloat16)
    w3 = (torch.randn(3, C, 3, C, generator=g) * (1.0 / (3 * C) ** 0.5)).to(torch.bfloat16)            # [block][cout][tap][cin]
    wsc = (torch.randn(3, C, C, generator=g) * (0.7 / C ** 0.5)).to(torch.bfloat16)
    w4 = (torch.randn(3, C, C, generator=g) * (0.7 / C ** 0.5)).to(torch.bfloat16)
    b3, bsc, b4 = (torch.randn(3, C, generator=g) * 0.1 for _ in range(3))
    xd = x.to(dev)
    w11 = torch.cat([wsc, w4], dim=2).unsqueeze(2).contiguous()                                          # [block][cout][1][2C]
    chain = _stage_chain(xd, w3.to(dev), b3.to(dev), w11.to(dev), (bsc + b4).to(dev), B, S, C)
    wf = torch.cat([w3.permute(0, 2, 1, 3).reshape(3, 3 * C, C), wsc, w4], dim=1).contiguous()          # [block][5C][C]
    bf = torch.stack([b3, bsc + b4], dim=1).contiguous()
    fused = torch.empty(B, S, C, device=dev, dtype=torch.bfloat16)
    ops.melgan_stage_fwd(xd, wf.to(dev), bf.to(dev), fused, (1, 3, 9), slope=0.2, out_slope=0.0)
    fused_l = torch.empty(B, S, C, device=dev, dtype=torch.bfloat16)
    ops.melgan_stage_fwd(xd, wf.to(dev), bf.to(dev), fused_l, (1, 3, 9), slope=0.2, out_slope=0.2)
    torch.cuda.synchronize()
    y = x.double().transpose(1, 2)
    for j, d in enumerate((1, 3, 9)):
        t = F.conv1d(F.pad(F.leaky_relu(y, 0.2), (d, d), mode="reflect"), w3[j].double().permute(0, 2, 1), b3[j].double(), dilation=d)
        y = F.conv1d(y, wsc[j].double().unsqueeze(2), bsc[j].double()) + F.conv1d(F.leaky_relu(t, 0.2), w4[j].double().unsqueeze(2), b4[j].double())
    exact = y.transpose(1, 2)
    e_f, e_c = R.rel(fused, exact), R.rel(chain, exact)
    print(f"C={C} S={S}: fused-to-exact {e_f:.2e}  chain-to-exact {e_c:.2e}")
    assert e_f <= 1.1 * e_c + 1e-4, (e_f, e_c)
    # elementwise: no row (tile seam, reflected end) is off by more than a few bf16 steps of the tensor's scale
    scale = exact.abs().max().item()
    assert (fused.double().cpu() - exact).abs().max().item() <= 0.04 * scale
    # the stored-lrelu form rounds leaky_relu(v) of the SAME fp32 value v once: where v >= 0 the two stores are the same bits; where
    # v < 0, fused = v (1 + e1) and fused_l = 0.2 v (1 + e2)(1 + e3), |e1|, |e2| <= 2^-8 (bf16: 8 significant bits, round to nearest),
    # |e3| <= 2^-24 (the fp32 product), so fused_l / (0.2 fused) lies within 2^-7 (1 + 2^-7) of 1; and it meets the same elementwise bound
    f64, l64 = fused.double().cpu(), fused_l.double().cpu()
    pos = f64 >= 0
    assert torch.equal(l64[pos], f64[pos])
    assert ((l64 - 0.2 * f64).abs() <= 2.0 ** -7 * (1 + 2.0 ** -7) * (0.2 * f64).abs())[~pos].all()
    assert (l64 - F.leaky_relu(exact, 0.2)).abs().max().item() <= 0.04 * scale


@pytest.mark.parametrize("cdt,fuse", [("fp32", False), ("bf16", True), ("bf16", False)])
def test_batch_items_are_independent_bit_for_bit(dev, cdt, fuse):
    """item 1 of a B = 3 run equals a B = 1 run of that item: a reflection never reads a neighbour's rows"""
    sd, x, _ = case(3, 5)
    gen = make_gen(sd, dev, cdt, fuse)
    with torch.no_grad():
        full = gen(x.to(dev))
        one = gen(x[1:2].to(dev))
        pcm3 = gen.infer_pcm(x.to(dev))
        pcm1 = gen.infer_pcm(x[1:2].to(dev))
    assert torch.equal(full[1], one[0]) and torch.equal(pcm3[1], pcm1[0])


@pytest.mark.parametrize("cdt,fuse", [("fp32", False), ("bf16", True)])
def test_two_runs_are_bit_identical(dev, cdt, fuse):
    sd, x, _ = case(2, 9)
    gen = make_gen(sd, dev, cdt, fuse)
    with torch.no_grad():
        a, b = gen(x.to(dev)).clone(), gen(x.to(dev)).clone()
        pa, pb = gen.infer_pcm(x.to(dev)).clone(), gen.infer_pcm(x.to(dev)).clone()
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_infer_pcm_has_astype_int16_semantics(dev):
    """infer_pcm == (forward x 32768).astype(int16): exactly against the product's own float waveform, within 4 LSB of the fp64 one
    (the allowance tests/test_vocoder_stft_gpu.py gives HiFi-GAN against its oracle)"""
    sd, x, exact = case(1, 37)
    gen = make_gen(sd, dev, "fp32", False)
    with torch.no_grad():
        pcm = gen.infer_pcm(x.to(dev), 32768.0)
        wav = gen(x.to(dev)).squeeze(1)
    assert pcm.dtype == torch.int16 and pcm.shape == (1, 256 * 37)
    assert np.array_equal(pcm.cpu().numpy(), (wav.cpu().numpy() * 32768.0).astype("int16"))
    ref = (exact["wav"].numpy() * 32768.0).astype("int16")
    diff = np.abs(pcm.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
    assert diff.max() <= 4, diff.max()


def test_synthesize_cli_batch_mode_with_melgan(dev, tmp_path):
    """synthesize.py --mode batch as a child process with `vocoder.model: MelGAN` in model.yaml, a random-init vocoder, a tiny synthetic
    checkpoint and a two-line source file: wavs of frames x 256 samples"""
    import copy
    from scipy.io import wavfile
    from fastspeech2_amd.model import FastSpeech2
    from tests.golden import configs
    from tests.helpers import make_preprocessed_dir
    root = str(tmp_path)
    data = make_preprocessed_dir(os.path.join(root, "data"), seed=31, n_train=8, n_val=2, lo=6, hi=12)
    pcfg, mcfg = configs.make(dec_layers=1, enc_layers=1)
    pcfg["path"]["preprocessed_path"] = data
    mcfg["vocoder"] = {"model": "MelGAN", "speaker": "universal"}
    tcfg = copy.deepcopy(configs.TRAIN)
    tcfg["path"] = {k: os.path.join(root, "out", k.split("_")[0]) for k in ("ckpt_path", "log_path", "result_path")}
    paths = []
    for name, cfg in (("preprocess.yaml", pcfg), ("model.yaml", mcfg), ("train.yaml", tcfg)):
        paths.append(os.path.join(root, name))
        with open(paths[-1], "w") as f:
            yaml.safe_dump(cfg, f)
    os.makedirs(tcfg["path"]["ckpt_path"])
    torch.manual_seed(11)
    msd = FastSpeech2(pcfg, mcfg).state_dict()
    # an untrained duration predictor says log(d + 1) ~ 0, i.e. no frames at all: a bias of 1.5 makes it 3 - 4 frames per phoneme
    key = "variance_adaptor.duration_predictor.linear_layer.bias"
    msd[key] = torch.full_like(msd[key], 1.5)
    torch.save({"model": msd}, os.path.join(tcfg["path"]["ckpt_path"], "1.pth.tar"))
    src = os.path.join(data, "val.txt")
    names = [l.split("|")[0] for l in open(src).read().strip().split("\n")]
    assert len(names) == 2
    p = subprocess.run([sys.executable, os.path.join(ROOT, "synthesize.py"), "--restore_step", "1", "--mode", "batch", "--source", src,
                        "-p", paths[0], "-m", paths[1], "-t", paths[2], "--random_vocoder", "--melgan_dir", os.path.join(root, "none"),
                        "--batch_size", "2", "--vocoder_dtype", "bf16"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    for n in names:
        sr, wav = wavfile.read(os.path.join(tcfg["path"]["result_path"], n + ".wav"))
        assert sr == 22050 and wav.dtype == np.int16 and len(wav) >= 4 * 256 and len(wav) % 256 == 0
