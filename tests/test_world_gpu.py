"""Spectral-envelope mel-cepstra on the GPU (fastspeech2_amd.envelope, csrc/fs2_world.hip) against the numpy oracle
tests/world_ref.py: the envelope and the mel-cepstra elementwise on ragged batches whose padding is NaN in every input and output,
at both transform sizes and on F0 rows that reach every branch; known answers through the whole device path; run-to-run
determinism; refusals before a launch; score.py --cepstra end to end.  The bars come from tests/golden/world_bars.json: 16 x the
distance between two summation orders of the oracle on these same inputs, measured on the CPU (tests/golden/make_world_bars.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import envelope as E
from fastspeech2_amd import metrics as M
from tests import f0_signals as S
from tests import world_cases as C
from tests import world_ref as W
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def padded(arrays, dtype, dev, extra=0):
    """[(n_b,)] -> (B, max n + extra) device tensor, NaN outside the arrays"""
    out = np.full((len(arrays), max(len(a) for a in arrays) + extra), NAN, dtype)
    for b, a in enumerate(arrays):
        out[b, :len(a)] = a
    return torch.from_numpy(out).to(dev)


class Case:
    def __init__(self, name, fs, frame_period, rows, f0, dev):
        self.name, self.fs, self.frame_period, self.rows, self.f0 = name, fs, frame_period, rows, f0
        self.lens, self.frames = [len(r) for r in rows], [len(v) for v in f0]
        self.y, self.f0_d = padded(rows, np.float32, dev, extra=5), padded(f0, np.float64, dev, extra=3)
        self.env = [W.envelope(x, v, fs, frame_period) for x, v in zip(rows, f0)]       # the oracle, once
        self.bins = W.fft_size(fs) // 2 + 1


@pytest.fixture(scope="module")
def cases(dev):
    rows, f0 = C.ragged_case()
    fs, fp, wrows, wf0 = C.wide_case()
    return {"22050": Case("22050", C.FS, C.FRAME_PERIOD, rows, f0, dev), "48000": Case("48000", fs, fp, wrows, wf0, dev)}


@pytest.mark.parametrize("name", ["22050", "48000"])
def test_envelope_against_oracle(dev, cases, name):
    c = cases[name]
    bar = C.bars()["ln_envelope_bar"][name]
    buf = torch.full((len(c.rows), max(c.frames) + 2, c.bins + 3), NAN, dtype=torch.float64, device=dev)
    out = E.envelope(c.y, c.lens, c.f0_d, c.frames, c.fs, c.frame_period, out=buf[:, :, :c.bins])
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    worst = 0.0
    for b, want in enumerate(c.env):
        F = c.frames[b]
        assert np.isnan(got[b, F:]).all() and np.isnan(got[b, :, c.bins:]).all()    # the padding of `out` is left alone
        assert (got[b, :F, :c.bins] > 0).all()
        worst = max(worst, float(np.abs(np.log(got[b, :F, :c.bins]) - np.log(want)).max()))
    print(name, "max |ln envelope - oracle|", worst, "bar", bar)
    assert worst <= bar
    fresh = E.envelope(c.y, c.lens, c.f0_d, c.frames, c.fs, c.frame_period)
    assert fresh.shape == (len(c.rows), max(c.frames), c.bins)
    for b, F in enumerate(c.frames):
        assert torch.equal(fresh[b, :F], out[b, :F])


@pytest.mark.parametrize("name,K,a", [("22050", 24, 0.455), ("22050", 40, 0.455), ("22050", 24, 0.0), ("22050", 40, 0.0),
                                      ("48000", 40, 0.455), ("48000", 24, 0.0)])
def test_mel_cepstra_against_oracle(dev, cases, name, K, a):
    c = cases[name]
    bar = C.bars()["mcep_bar"][name][f"{K},{a}"]
    buf = torch.full((len(c.rows), max(c.frames) + 1, K + 2), NAN, dtype=torch.float64, device=dev)
    E.world_cepstra(c.y, c.lens, c.f0_d, c.frames, c.fs, c.frame_period, n_mcep=K, alpha=a, out=buf[:, :, :K])
    got = buf.cpu().numpy()
    env = E.envelope(c.y, c.lens, c.f0_d, c.frames, c.fs, c.frame_period).cpu().numpy() if a == 0.0 else None
    worst = own = 0.0
    for b, e in enumerate(c.env):
        F = c.frames[b]
        assert np.isnan(got[b, F:]).all() and np.isnan(got[b, :, K:]).all()
        worst = max(worst, float(np.abs(got[b, :F, :K] - W.mel_cepstra(e, K, a)).max()))
        if env is not None:                                                 # no warping: the plain cepstrum of the device's own envelope
            own = max(own, float(np.abs(got[b, :F, :K] - W.plain_cepstrum(env[b, :F])[:, 1:K + 1]).max()))
    print(name, K, a, "max |c~ - oracle|", worst, "against the device's own plain cepstrum", own, "bar", bar)
    assert worst <= bar and own <= bar


# ------------------------------------------------------------------------------------------------ known answers
def stft_of(cfg):
    from fastspeech2_amd import audio as Audio
    pp = cfg["preprocessing"]
    return Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"],
                              pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])


def test_known_answers_through_the_device_path(dev):
    """An identical pair scores exactly 0.  The 120 / 220 Hz renderings of one filter: `score_pairs` extracts its own F0, so the
    comparison with the oracle's recorded score feeds the device the F0 the record was made with (envelope -> mel-cepstra -> DTW,
    all on the device).  Its distance from the record is bounded by the envelope bar e carried through: |dc_q| <= e for the
    one-sided cepstrum of 0.5 ln envelope, |dc~_m| <= e max_m sum_q |table[m][q]|, a local cost moves by at most 2 sqrt(K) that
    (both sides), and so does the mean along a path of the same length."""
    rec = C.bars()
    xs = [C.pulse_train(f) for f in C.PITCHES]
    F, K = rec["pair_frames"], E.DEFAULT_MCEP
    y = torch.from_numpy(np.stack(xs)).to(dev)
    f0 = torch.tensor([[f] * F for f in C.PITCHES], dtype=torch.float64, device=dev)
    c = E.world_cepstra(y, [len(x) for x in xs], f0, [F, F], C.FS, C.FRAME_PERIOD)
    total, plen, _, _ = M.dtw(c[:1], [F], c[1:], [F])
    got = M.scores_from_sums(total.cpu().numpy()[0], plen.cpu().numpy()[0], F, F)
    e = rec["ln_envelope_bar"]["22050"]
    tol = M.MCD_SCALE * 2.0 * np.sqrt(K) * e * np.abs(E.freqt_table(1024, K, E.ALPHA[C.FS])).sum(axis=1).max()
    print("device", got["mcd_db"], "recorded", rec["mcd_world_db"], "tolerance", tol)
    assert got["path_len"] == rec["pair_path_len"]
    assert abs(got["mcd_db"] - rec["mcd_world_db"]) <= tol

    stft = stft_of(config("/nowhere"))
    refs, syns = [xs[0], xs[0]], [xs[1], xs[0].copy()]
    world = M.score_pairs(refs, syns, None, C.FS, C.HOP, device=dev, cepstra="world")
    mel = M.score_pairs(refs, syns, stft, C.FS, C.HOP, device=dev)
    print("score_pairs world", world[0]["mcd_db"], "mel", mel[0]["mcd_db"])
    assert world[1]["mcd_db"] == 0.0 and world[1]["path_len"] == world[1]["frames_ref"] == world[1]["frames_syn"]
    assert 0.0 < world[0]["mcd_db"] < mel[0]["mcd_db"]
    assert all(r["cepstra"] == "world" and r["alpha"] == 0.455 and r["fft_size"] == 1024 for r in world)
    assert all("cepstra" not in r for r in mel)
    quiet = M.score_pairs(refs, syns, None, C.FS, C.HOP, device=dev, cepstra="world", f0=False)     # F0 still drives the envelope
    assert [r["mcd_db"] for r in quiet] == [r["mcd_db"] for r in world] and all("vuv_error" not in r for r in quiet)


def test_two_runs_are_byte_identical(dev):
    refs = [S.tone(200.0, 0.3), S.tone(150.0, 0.25), C.pulse_train(120.0, dur=0.2)]
    syns = [S.tone(220.0, 0.28), S.tone(150.0, 0.3), C.pulse_train(220.0, dur=0.2)]
    first = M.score_pairs(refs, syns, None, S.FS, S.HOP, device=dev, cepstra="world")
    second = M.score_pairs(refs, syns, None, S.FS, S.HOP, device=dev, cepstra="world")
    small = M.score_pairs(refs, syns, None, S.FS, S.HOP, device=dev, cepstra="world", budget=1)     # one pair per batch
    assert json.dumps(first) == json.dumps(second) == json.dumps(small)
    assert all(r["mcd_db"] > 0 and "f0_rmse_cents" in r for r in first)


def test_bad_arguments_are_refused_before_a_launch(dev):
    y = torch.zeros(2, 3000, dtype=torch.float32, device=dev)
    f0 = torch.zeros(2, 12, dtype=torch.float64, device=dev)
    lens, frames, fp = [3000, 2000], [12, 8], S.FRAME_PERIOD
    E.world_cepstra(y, lens, f0, frames, S.FS, fp)                          # the good call
    for bad in (lambda: E.envelope(y.double(), lens, f0, frames, S.FS, fp),
                lambda: E.envelope(y, lens, f0.float(), frames, S.FS, fp),
                lambda: E.envelope(y.cpu(), lens, f0, frames, S.FS, fp),
                lambda: E.envelope(y, lens, f0.cpu(), frames, S.FS, fp),
                lambda: E.envelope(y, lens, f0, [12, 9], S.FS, fp),         # 2000 samples hold 8 frames
                lambda: E.envelope(y, lens, f0, [13, 8], S.FS, fp),         # more frames than f0 has columns
                lambda: E.envelope(y, [3001, 2000], f0, frames, S.FS, fp),
                lambda: E.envelope(y, lens, f0, [12], S.FS, fp),
                lambda: E.envelope(y, lens, f0, frames, S.FS, fp, out=torch.zeros(2, 12, 512, dtype=torch.float64, device=dev)),
                lambda: E.world_cepstra(y, lens, f0, frames, S.FS, fp, n_mcep=0),
                lambda: E.world_cepstra(y, lens, f0, frames, S.FS, fp, n_mcep=41),
                lambda: E.world_cepstra(y, lens, f0, frames, 96000, fp),    # N = 4096
                lambda: E.world_cepstra(y, lens, f0, frames, 32000, fp),    # no tabulated alpha
                lambda: M.score_pairs([np.zeros(3000, np.float32)], [np.zeros(3000, np.float32)], None, 32000, 256, device=dev,
                                      cepstra="world"),
                lambda: M.score_pairs([np.zeros(3000, np.float32)], [np.zeros(3000, np.float32)], None, S.FS, 256, device=dev,
                                      cepstra="sptk")):
        with pytest.raises(ValueError):
            bad()
    assert E.world_cepstra(y, lens, f0, frames, 32000, 8.0, alpha=0.5).shape == (2, 12, 24)


# ------------------------------------------------------------------------------------------------ score.py
def test_score_command_line_with_both_cepstra(dev, tmp_path):
    """score.py as a fresh child process per run, on three 16-bit wav pairs: --cepstra world rows carry cepstra / alpha / fft_size
    and equal `score_pairs` on the same files; --cepstra mel writes, byte for byte, what no flag writes."""
    from scipy.io import wavfile
    root = str(tmp_path)
    cfg = config(root)
    pairs = {"a": (S.tone(200.0, 0.3), S.tone(220.0, 0.28)), "b": (S.tone(150.0, 0.25), S.tone(150.0, 0.25)),
             "c": (C.pulse_train(120.0, dur=0.2), C.pulse_train(220.0, dur=0.2))}
    os.makedirs(os.path.join(root, "raw", "spk"))
    os.makedirs(os.path.join(root, "result"))
    for name, (ref, syn) in pairs.items():
        wavfile.write(os.path.join(root, "raw", "spk", name + ".wav"), S.FS, np.round(ref * 32767).astype(np.int16))
        wavfile.write(os.path.join(root, "result", name + ".wav"), S.FS, np.round(syn * 32767).astype(np.int16))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"{name}|spk|{{AA}}|text\n" for name in pairs))
    for name, doc in (("preprocess.yaml", cfg), ("train.yaml", {"path": {"result_path": os.path.join(root, "result")}})):
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)

    def cli(tag, *extra):
        out = os.path.join(root, tag + ".jsonl")
        run = subprocess.run([sys.executable, os.path.join(ROOT, "score.py"), "-p", os.path.join(root, "preprocess.yaml"), "-t",
                              os.path.join(root, "train.yaml"), "--source", os.path.join(root, "val.txt"), "--out", out, *extra],
                             capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        return open(out).read(), run.stdout.strip().splitlines()[-1]

    plain, plain_summary = cli("plain")
    mel, mel_summary = cli("mel", "--cepstra", "mel")
    assert mel == plain and mel_summary == plain_summary
    assert "cepstra" not in plain and "alpha" not in plain_summary
    text, summary = cli("world", "--cepstra", "world")
    rows = [json.loads(ln) for ln in text.splitlines()]
    summary = json.loads(summary)
    assert [r["basename"] for r in rows] == list(pairs)
    assert all(r["cepstra"] == "world" and r["alpha"] == 0.455 and r["fft_size"] == 1024 for r in rows + [summary])
    assert summary["utterances"] == 3 and rows[1]["mcd_db"] == 0.0
    files = [[M.load_audio(os.path.join(root, d, name + ".wav"), S.FS) for name in pairs] for d in (os.path.join("raw", "spk"), "result")]
    want = M.score_pairs(files[0], files[1], None, S.FS, S.HOP, device=dev, cepstra="world")
    for r, w in zip(rows, want):
        assert json.dumps({k: r[k] for k in w}) == json.dumps(w)
