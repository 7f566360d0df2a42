"""GPU F0 (fastspeech2_amd.pitch, csrc/fs2_f0.hip): known answers, amplitude invariance, agreement with the numpy oracle
tests/f0_ref.py (dio, stonemask and both), real speech, ragged batches with poisoned padding, and the preprocessor end to end."""
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import pitch
from fastspeech2_amd import preprocess as P
from tests import f0_ref as R
from tests.f0_signals import (FRAME_PERIOD, FS, TONE_F0, far_from_signal, glide, interior, speech, tone, tones_with_silence)

pytestmark = pytest.mark.gpu
RTOL = 1e-6


def _batch(xs, dev, poison=0.0):
    lens = [len(x) for x in xs]
    y = torch.full((len(xs), max(max(lens), 1)), poison, dtype=torch.float32)
    for b, x in enumerate(xs):
        y[b, :len(x)] = torch.from_numpy(np.asarray(x, np.float32))
    return y.to(dev), lens


def _signals():
    x_sp, sr = speech()
    assert sr == FS
    return [tone(f) for f in TONE_F0] + [glide()[0], tones_with_silence(), x_sp]


def _agree(got, want, what):
    """identical voicing, every voiced frame within RTOL"""
    assert got.shape == want.shape, what
    assert np.array_equal(got > 0, want > 0), (what, np.nonzero((got > 0) != (want > 0))[0])
    v = want > 0
    if v.any():
        rel = np.abs(got[v] / want[v] - 1).max()
        assert rel <= RTOL, (what, rel)


@pytest.fixture(scope="module")
def gpu_result(dev):
    xs = _signals()
    y, lens = _batch(xs, dev, poison=float("nan"))
    f0_dio, t, frames = pitch.dio(y, lens, FS, FRAME_PERIOD)
    f0_sm = pitch.stonemask(y, lens, f0_dio, frames, FS, FRAME_PERIOD)
    return xs, f0_dio.cpu().numpy(), f0_sm.cpu().numpy(), t, frames.numpy()


def test_known_answers(gpu_result):
    xs, _, f0, t, frames = gpu_result
    for b, f in enumerate(TONE_F0):
        tb = t[:frames[b]]
        v = f0[b, :frames[b]][interior(tb, len(xs[b]))]
        assert np.mean(v > 0) >= 0.98, f
        assert np.all(np.abs(v[v > 0] / f - 1) <= 0.005), (f, np.abs(v[v > 0] / f - 1).max())
    b = len(TONE_F0)
    _, true = glide()
    tb = t[:frames[b]]
    m = interior(tb, len(xs[b]))
    fb = f0[b, :frames[b]][m]
    assert np.mean((fb > 0) & (np.abs(fb / true(tb[m]) - 1) <= 0.02)) >= 0.95
    b += 1
    tb = t[:frames[b]]
    far = far_from_signal(xs[b], tb)
    assert far.sum() >= 10 and np.all(f0[b, :frames[b]][far] == 0)
    for b in range(len(xs)):
        assert np.all(f0[b, frames[b]:] == 0) and np.all(np.isfinite(f0[b]))


def test_against_oracle(gpu_result):
    """dio alone, stonemask alone (fed the oracle's own DIO contour) and both, on every signal"""
    xs, f0_dio, f0_sm, t, frames = gpu_result
    dev = torch.device("cuda:0")
    y, lens = _batch(xs, dev)
    ref_dio, ref_sm = [], []
    for b, x in enumerate(xs):
        want_sm, want_dio, tt = R.dio_stonemask(x, FS, FRAME_PERIOD)
        assert len(tt) == frames[b] and np.array_equal(tt, t[:frames[b]])
        _agree(f0_dio[b, :frames[b]], want_dio, ("dio", b))
        _agree(f0_sm[b, :frames[b]], want_sm, ("dio+stonemask", b))
        ref_dio.append(want_dio)
        ref_sm.append(want_sm)
    fin = torch.zeros(len(xs), f0_dio.shape[1], dtype=torch.float64)
    for b, d in enumerate(ref_dio):
        fin[b, :len(d)] = torch.from_numpy(d)
    got = pitch.stonemask(y, lens, fin.to(dev), frames, FS, FRAME_PERIOD).cpu().numpy()
    for b, want in enumerate(ref_sm):
        _agree(got[b, :frames[b]], want, ("stonemask", b))


def test_real_speech_plausible(gpu_result):
    xs, _, f0, _, frames = gpu_result
    b = len(xs) - 1
    v = f0[b, :frames[b]]
    assert np.mean(v > 0) > 0.3
    assert 150.0 <= np.median(v[v > 0]) <= 280.0, np.median(v[v > 0])


def test_amplitude_invariance(dev):
    xs = [tone(150), glide()[0], speech()[0]]
    y, lens = _batch(xs, dev)
    a, _, _ = pitch.dio_stonemask(y, lens, FS, FRAME_PERIOD)
    b, _, _ = pitch.dio_stonemask(y * 0.05, lens, FS, FRAME_PERIOD)
    for r in range(len(xs)):
        _agree(b[r], a[r], ("scale 0.05", r))


def test_ragged_rows_bitwise_alone(dev):
    """each row of a mixed batch == that row alone, bitwise; padding poisoned with NaN / huge values never reaches an output"""
    x_sp = speech()[0]
    rng = np.random.RandomState(4)
    xs = [x_sp[:30000], tone(200)[:256], tone(330)[:1], np.zeros(0, np.float32), tone(450)[:200], tone(110)[:5000],
          (0.3 * rng.randn(257)).astype(np.float32), x_sp[7000:20000], tone(80)[:257 * 40]]
    for poison in (float("nan"), 3.0e30):
        y, lens = _batch(xs, dev, poison=poison)
        f0, t, frames = pitch.dio_stonemask(y, lens, FS, FRAME_PERIOD)
        assert frames.tolist() == [pitch.frame_count(n, FS, FRAME_PERIOD) for n in lens]
        assert np.all(np.isfinite(f0))
        for b, x in enumerate(xs):
            y1, l1 = _batch([x], dev, poison=-poison)
            g1, _, fr1 = pitch.dio_stonemask(y1, l1, FS, FRAME_PERIOD)
            assert fr1[0] == frames[b]
            assert np.array_equal(f0[b, :frames[b]], g1[0, :frames[b]]), b
            assert np.all(f0[b, frames[b]:] == 0)
    assert np.any(f0[0] > 0) and np.any(f0[-1] > 0)


def test_api_checks(dev):
    y, lens = _batch([tone(200)], dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch.dio(y.cpu(), lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pitch.dio(y.double(), lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pitch.dio(y[0], lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pitch.dio(y, [y.shape[1] + 1], FS, FRAME_PERIOD)
    f0, _, frames = pitch.dio(y, lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pitch.stonemask(y, lens, f0.float(), frames, FS, FRAME_PERIOD)
    fn = pitch.pitch_fn(dev)
    out = fn(tone(200), FS, 256)
    assert out.dtype == np.float64 and len(out) == pitch.frame_count(FS, FS, FRAME_PERIOD)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_preprocessor_gpu_pitch_end_to_end(dev, tmp_path, monkeypatch):
    """raw corpus -> Preprocessor(pitch="gpu") -> files byte-identical to pitch_fn=pitch.pitch_fn(dev) -> Dataset -> one step"""
    import copy
    from fastspeech2_amd.data import Dataset
    from fastspeech2_amd.model import FastSpeech2, FastSpeech2Loss, ScheduledOptim
    from fastspeech2_amd.utils import to_device
    from tests.golden import configs
    from tests.helpers import make_raw_corpus

    real = os.listdir
    monkeypatch.setattr(os, "listdir", lambda p: sorted(real(p)))
    trees, outs = [], []
    for tag, kw in (("gpu", dict(pitch="gpu", batch_seconds=2.5)), ("fn", dict(pitch_fn=pitch.pitch_fn(dev)))):
        cfg, _ = make_raw_corpus(str(tmp_path / tag))
        outs.append(P.Preprocessor(cfg, device=dev, seed=3, **kw).build_from_path())
        pre = cfg["path"]["preprocessed_path"]
        trees.append({k: v for k, v in _tree(pre).items() if not k.startswith("TextGrid")})
    assert outs[0] == outs[1]
    assert trees[0].keys() == trees[1].keys() and all(trees[0][k] == trees[1][k] for k in trees[0]), \
        [k for k in trees[0] if trees[0][k] != trees[1].get(k)]
    assert len(outs[0]) >= 3 and any(k.startswith("pitch") for k in trees[0])
    import json
    stats = json.loads(trees[0]["stats.json"])
    assert 60.0 < stats["pitch"][2] < 800.0                               # phoneme-level mean of real F0 values

    cfg, _ = make_raw_corpus(str(tmp_path / "gpu2"))
    cfg["preprocessing"]["val_size"] = 1
    P.Preprocessor(cfg, device=dev, seed=3, pitch="gpu").build_from_path()
    pcfg, mcfg = configs.make(dec_layers=1, enc_layers=1)
    pcfg = copy.deepcopy(pcfg)
    pcfg["path"] = dict(pcfg["path"], preprocessed_path=cfg["path"]["preprocessed_path"])
    pcfg["dataset"] = cfg["dataset"]
    tcfg = copy.deepcopy(configs.TRAIN)
    tcfg["optimizer"]["batch_size"] = 2
    ds = Dataset("train.txt", pcfg, tcfg, sort=True, drop_last=True)
    assert len(ds) >= 2
    batch = ds.collate_fn([ds[i] for i in range(2)])[0]
    model = FastSpeech2(pcfg, mcfg, compute_dtype="fp32").to(dev).train()
    opt = ScheduledOptim(model, tcfg, mcfg, 0)
    b = to_device(batch, dev)
    losses = FastSpeech2Loss(pcfg, mcfg)(b, model(*b[2:]))
    losses[0].backward()
    opt.step_and_update_lr()
    assert all(torch.isfinite(l).item() for l in losses)


def test_pyworld_cross_check(gpu_result):
    """reported, not gated: agreement with pyworld where it is installed"""
    pw = pytest.importorskip("pyworld")
    xs, _, f0, _, frames = gpu_result
    for b, x in enumerate(xs):
        xd = x.astype(np.float64)
        d, tt = pw.dio(xd, FS, frame_period=FRAME_PERIOD)
        ref = pw.stonemask(xd, d, tt, FS)
        n = min(len(ref), frames[b])
        both = (ref[:n] > 0) & (f0[b, :n] > 0)
        print("pyworld row %d: frames %d/%d, voicing agreement %.3f, median |rel| on both-voiced %.2e" % (
            b, frames[b], len(ref), np.mean((ref[:n] > 0) == (f0[b, :n] > 0)),
            np.median(np.abs(f0[b, :n][both] / ref[:n][both] - 1)) if both.any() else float("nan")))
