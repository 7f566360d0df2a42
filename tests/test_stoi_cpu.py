"""STOI / ESTOI without a GPU: the host helpers of fastspeech2_amd/stoi.py against closed forms, the known answers of the
specification through the numpy restatement tests/stoi_ref.py, `metrics.run` with and without `aligned` through its `score_fn` /
`aligned_fn` seams, and copysynth.py with the vocoder stubbed.  The bars are those of tests/golden/stoi_bars.json (16 times the
distance between the fp64 and the longdouble restatement, tests/golden/make_stoi_bars.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml
from scipy.io import wavfile

from fastspeech2_amd import metrics as M
from fastspeech2_amd import stoi as S
from tests import stoi_ref as ref
from tests.test_align_cpu import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "stoi_bars.json")))
BAR = BARS["factor"] * BARS["distance"]["final"]
SR, HOP = 22050, 256


# ------------------------------------------------------------------------------------------------ host helpers
def test_window_is_matlabs_hanning():
    w = S.window()
    n = np.arange(256)
    assert w.shape == (256,) and w.dtype == np.float64
    assert np.abs(w - np.sin(np.pi * (n + 1) / 257) ** 2).max() < 1e-15     # 0.5 (1 - cos 2a) = sin^2 a
    assert w.min() > 0 and np.abs(w - w[::-1]).max() < 1e-15                # no zero end points, symmetric
    assert abs(w[0] - 0.5 * (1 - math.cos(2 * math.pi / 257))) < 1e-18 and np.abs(w - ref.window()).max() == 0


def test_bands_are_contiguous_third_octaves():
    lo, hi = S.band_edges()
    assert len(lo) == len(hi) == 15 and lo[0] == 7 and hi[-1] == 219
    assert np.all(hi > lo) and np.array_equal(lo[1:], hi[:-1])              # non-empty, no gap, no overlap
    assert [(int(a), int(b)) for a, b in zip(lo, hi)] == ref.bands()[0]
    c = S.band_centres()
    assert np.allclose(c, 150.0 * 2.0 ** (np.arange(15) / 3.0), rtol=1e-15) and np.allclose(c, ref.bands()[1], rtol=1e-15)
    f = np.arange(257) * 10000 / 512
    assert np.all(f[lo] < c) and np.all(c < f[hi])                          # each centre lies inside its band
    tw = S.twiddle()
    assert tw.shape == (512, 2) and np.abs(tw[:, 0] ** 2 + tw[:, 1] ** 2 - 1).max() < 1e-15 and tw[128].tolist() == pytest.approx([0, 1])


def test_frame_counts():
    assert [S.n_frames(n) for n in (0, 255, 256, 257, 384, 385, 512, 513)] == [0, 0, 0, 1, 1, 2, 2, 3]
    assert [ref.n_frames(n) for n in (256, 257, 384, 385)] == [0, 1, 1, 2]
    for n in (256, 257, 384, 385, 4097):
        assert len(ref.frames_of(np.zeros(n))) == S.n_frames(n)
    assert S.CLIP == 1 + 10 ** 0.75 and S.EPS == np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ known answers
def _loud(n, seed=3):
    return ref.signal(n, np.random.default_rng(seed), silences=False).astype(np.float64)


def test_a_signal_against_itself_its_negative_and_its_double():
    x = _loud(12000)
    for y in (x, -x, 2 * x):
        st, es = ref.scores(x, y)
        assert abs(st - 1) <= BAR and abs(es - 1) <= BAR, (st, es)


def test_added_noise_lowers_both_scores_strictly():
    x = _loud(20000)
    noise = np.random.default_rng(5).standard_normal(len(x))
    noise *= np.sqrt((x ** 2).mean() / (noise ** 2).mean())
    got = [ref.scores(x, x + noise * 10 ** (-snr / 20)) for snr in (20, 10, 0, -10)]
    print(got)
    for k in (0, 1):
        v = [g[k] for g in got]
        assert 1 > v[0] > v[1] > v[2] > v[3] > -0.2, v
    assert got[0][0] > 0.9 and got[3][0] < 0.6


def test_silence_at_a_pause_changes_nothing():
    """Zeros (more than 60 dB down) spliced into both signals at the same place, at the start, inside and at the end, leave both
    scores where they were and keep exactly the frames that hold a loud sample.  The place is a pause of the signal, on the hop
    grid: a splice into a loud passage cuts two frames in half, which then stay (their loud half is within 40 dB), so the
    compacted signal gains a half-silent frame and the score moves a little; that is the algorithm, pystoi's too, not rounding."""
    H = 128
    rng = np.random.default_rng(11)
    a, b = _loud(40 * H, 1), _loud(45 * H, 2)
    z = np.zeros
    x = np.concatenate([z(H), a, z(2 * H), b, z(2 * H)])
    y = x + 0.03 * rng.standard_normal(len(x)) * (x != 0)
    base = ref.chain(x, y)
    assert base["segments"] > 30 and 0.5 < base["stoi"] < 0.999
    loud = lambda s: sum(1 for k in range(0, max(len(s) - 256, 0), H) if np.any(s[k:k + 256] != 0))    # noqa: E731
    assert base["frames_kept"] == loud(x) < base["frames"]
    for at, n in ((0, 5 * H), (H + len(a) + H, 7 * H), (len(x), 4 * H)):
        x2, y2 = np.insert(x, at, z(n)), np.insert(y, at, z(n))
        c = ref.chain(x2, y2)
        assert c["frames"] == base["frames"] + n // H and c["frames_kept"] == base["frames_kept"] == loud(x2), at
        assert abs(c["stoi"] - base["stoi"]) <= BAR and abs(c["estoi"] - base["estoi"]) <= BAR, at


def test_too_short_is_nan_and_flagged():
    x, y = _loud(3969), _loud(3969, 4)
    c = ref.chain(x, y)
    assert c["X"].shape == (15, 29) and c["segments"] == 0 and c["too_short"] and np.isnan(c["stoi"]) and np.isnan(c["estoi"])
    x, y = _loud(4097), _loud(4097, 4)
    c = ref.chain(x, y)
    assert c["X"].shape == (15, 30) and c["segments"] == 1 and not c["too_short"] and c["seg"].shape == (2, 1)
    assert c["stoi"] == c["seg"][0, 0] and c["estoi"] == c["seg"][1, 0] and -1 <= c["stoi"] <= 1
    assert S.summarize([{"stoi": float("nan"), "estoi": float("nan"), "stoi_segments": 0}, {"stoi": 0.5, "estoi": 0.25, "stoi_segments": 3}]) \
        == {"stoi_mean": 0.5, "estoi_mean": 0.25, "stoi_too_short_utterances": 1}
    assert np.isnan(S.summarize([])["stoi_mean"])


def test_the_device_entry_points_refuse_host_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.measure(torch.zeros(1, 300), [300], torch.zeros(1, 300), [300], 10000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.score_pairs([np.zeros(300, np.float32)], [np.zeros(300, np.float32)], 22050, device="cpu")
    with pytest.raises(ValueError):
        S.score_pairs([np.zeros(300, np.float32)], [], 22050)


# ------------------------------------------------------------------------------------------------ metrics.run / score.py
def _write(path, x, sr=SR):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, (np.clip(x, -1, 1) * 32767).astype(np.int16))


@pytest.fixture()
def corpus(tmp_path):
    """u0 and u1 are copies of their recordings up to a few samples; u2's synthesized file is three hops short"""
    root = str(tmp_path)
    rng = np.random.RandomState(0)
    for name, n, m in (("u0", 20000, 20000), ("u1", 15000, 15000 - 2 * HOP), ("u2", 18000, 18000 - 3 * HOP)):
        x = rng.uniform(-0.5, 0.5, n)
        _write(os.path.join(root, "raw", "spk", name + ".wav"), x)
        _write(os.path.join(root, "result", name + ".wav"), x[:m])
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"u{k}|spk|{{AA B}}|text {k}\n" for k in range(3)))
    for name, doc in (("preprocess.yaml", config(root)), ("train.yaml", {"path": {"result_path": os.path.join(root, "result")}})):
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    return root


def _fake(refs, syns):
    return [{"mcd_db": len(r) / 1000, "path_len": len(s), "frames_ref": len(r) // HOP + 1, "frames_syn": len(s) // HOP + 1}
            for r, s in zip(refs, syns)]


def _aligned(seen):
    def fn(refs, syns):
        seen.append([(len(r), len(s)) for r, s in zip(refs, syns)])
        return [{"stoi": 0.5 + 0.1 * k, "estoi": 0.25, "stoi_frames_kept": 40, "stoi_segments": 10 * k, "aligned_samples": len(r)}
                for k, r in enumerate(refs)]
    return fn


def test_the_default_run_is_what_it_was(corpus):
    """rows and summary of a run without `aligned`, written out by hand: what the parent commit gives for this corpus"""
    rows, skipped, summary = M.run(config(corpus), os.path.join(corpus, "result"), os.path.join(corpus, "val.txt"), score_fn=_fake)
    lens = [(20000, 20000), (15000, 15000 - 2 * HOP), (18000, 18000 - 3 * HOP)]
    assert rows == [{"basename": f"u{k}", "speaker": "spk", "reference_window": "whole", "mcd_db": r / 1000, "path_len": s,
                     "frames_ref": r // HOP + 1, "frames_syn": s // HOP + 1} for k, (r, s) in enumerate(lens)]
    w = np.array([s for _, s in lens], np.float64)
    mcd = np.array([r / 1000 for r, _ in lens])
    assert skipped == [] and summary == {"utterances": 3, "mcd_db_mean": float(mcd.mean()), "mcd_db_weighted": float((mcd * w).sum() / w.sum()),
                                         "skipped": 0, "reference_window": {"textgrid": 0, "whole": 3}}
    again = M.run(config(corpus), os.path.join(corpus, "result"), os.path.join(corpus, "val.txt"), score_fn=_fake, aligned=False,
                  aligned_fn=lambda r, s: 1 / 0)
    assert again == (rows, skipped, summary)


def test_aligned_adds_keys_and_skips_what_is_not_aligned(corpus, capsys):
    import score
    seen = []
    out = os.path.join(corpus, "scores.jsonl")
    argv = ["-p", os.path.join(corpus, "preprocess.yaml"), "-t", os.path.join(corpus, "train.yaml"), "--source",
            os.path.join(corpus, "val.txt"), "--out", out, "--aligned"]
    rows, skipped, summary = score.main(argv, score_fn=_fake, aligned_fn=_aligned(seen))
    assert [r["basename"] for r in rows] == ["u0", "u1"] and seen == [[(20000, 20000), (15000 - 2 * HOP,) * 2]]      # cut to the shorter
    assert [s[0] for s in skipped] == ["u2"] and skipped[0][1].startswith("not time-aligned") and str(3 * HOP) in skipped[0][1]
    for r in rows:
        assert {"stoi", "estoi", "stoi_frames_kept", "stoi_segments", "aligned_samples", "mcd_db", "path_len"} <= set(r)
    assert rows[1]["aligned_samples"] == 15000 - 2 * HOP and rows[1]["mcd_db"] == 15.0              # the DTW side saw the whole pair
    assert summary["stoi_mean"] == 0.6 and summary["estoi_mean"] == 0.25 and summary["stoi_too_short_utterances"] == 1
    assert summary["utterances"] == 2 and summary["skipped"] == 1
    assert [json.loads(line) for line in open(out)] == rows
    assert "skipped u2: not time-aligned" in capsys.readouterr().out
    # --max_len_diff: a wider window takes u2 in, a narrower one drops u1 too
    rows, skipped, _ = score.main(argv + ["--max_len_diff", str(3 * HOP)], score_fn=_fake, aligned_fn=_aligned([]))
    assert len(rows) == 3 and not skipped
    rows, skipped, _ = score.main(argv + ["--max_len_diff", "0"], score_fn=_fake, aligned_fn=_aligned([]))
    assert [r["basename"] for r in rows] == ["u0"] and len(skipped) == 2
    with pytest.raises(SystemExit):
        score.main(argv + ["--max_len_diff", "-1"], score_fn=_fake, aligned_fn=_aligned([]))


# ------------------------------------------------------------------------------------------------ copysynth.py
class _Vocoder:
    def __init__(self):
        self.calls = []

    def infer_pcm(self, mels, max_wav_value):
        self.calls.append((tuple(mels.shape), max_wav_value))
        return torch.ones(mels.shape[0], mels.shape[2] * HOP, dtype=torch.int16)


def test_copysynth_arguments_and_the_missing_file_listing(tmp_path, capsys):
    import copysynth
    root = str(tmp_path)
    cfg = config(root)
    frames = {"a": 12, "b": 30, "c": 7}
    os.makedirs(os.path.join(root, "pre", "mel"))
    for name, T in frames.items():
        np.save(os.path.join(root, "pre", "mel", f"spk-mel-{name}.npy"), np.full((T, 80), -3.0, np.float32))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("a|spk|{AA}|x\nnone|spk|{AA}|x\nb|spk|{AA}|x\nbroken\nc|spk|{AA}|x\n")
    docs = {"p.yaml": cfg, "m.yaml": {"vocoder": {"model": "HiFi-GAN", "speaker": "universal"}},
            "t.yaml": {"path": {"result_path": os.path.join(root, "result")}}}
    for name, doc in docs.items():
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    argv = ["-p", os.path.join(root, "p.yaml"), "-m", os.path.join(root, "m.yaml"), "-t", os.path.join(root, "t.yaml"), "--source",
            os.path.join(root, "val.txt"), "--device", "cpu", "--batch_size", "2"]
    voc = _Vocoder()
    written, missing = copysynth.main(argv, vocoder=voc)
    assert written == [("a", 12 * HOP), ("b", 30 * HOP), ("c", 7 * HOP)]
    assert [m[0] for m in missing] == ["none", "broken"] and "spk-mel-none.npy" in missing[0][1] and missing[1][1] == "no speaker field"
    assert voc.calls == [((2, 80, 30), 32768.0), ((1, 80, 7), 32768.0)]      # longest first, two to a batch
    for name, T in frames.items():                                           # the default folder: {result_path}/copy
        rate, pcm = wavfile.read(os.path.join(root, "result", "copy", name + ".wav"))
        assert rate == SR and pcm.dtype == np.int16 and len(pcm) == T * HOP
    said = capsys.readouterr().out
    assert "skipped none: missing" in said and "skipped broken" in said and "3 utterances" in said
    written, _ = copysynth.main(argv + ["--out_dir", os.path.join(root, "elsewhere")], vocoder=_Vocoder())
    assert os.path.exists(os.path.join(root, "elsewhere", "b.wav")) and len(written) == 3
    for bad in (["--batch_size", "0"], ["--griffin_iters", "-1"], ["--vocoder_dtype", "fp16"]):
        with pytest.raises(SystemExit):
            copysynth.parse_args(argv + bad)
    with pytest.raises(SystemExit):
        copysynth.parse_args(argv[2:])                                       # -p is required
    with pytest.raises(ValueError, match="needs a vocoder"):
        copysynth.copy_synthesize((cfg, docs["m.yaml"], docs["t.yaml"]), os.path.join(root, "val.txt"), device="cpu")
    np.save(os.path.join(root, "pre", "mel", "spk-mel-c.npy"), np.zeros((7, 40), np.float32))
    with pytest.raises(ValueError, match="expected a"):
        copysynth.main(argv, vocoder=_Vocoder())
