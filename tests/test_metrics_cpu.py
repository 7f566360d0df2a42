"""Objective scoring without a GPU: the numpy oracle tests/dtw_ref.py against brute-force enumeration of every monotone path, the
known answers of the specification (fastspeech2_amd/metrics.py), the host pieces of the module (DCT table, summary, refusals) and
score.py's pairing, trimming, skipping and output through its `score_fn` seam."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import align as A
from fastspeech2_amd import metrics as M
from tests import dtw_ref as R
from tests.test_align_cpu import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_dtw_against_every_monotone_path():
    rng = np.random.RandomState(0)
    shapes = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 6), (6, 3), (6, 6), (4, 5)]
    n_tied = 0
    for T1, T2 in shapes:
        for kind in ("random", "ties", "zeros"):
            for _ in range(4):
                d = {"random": lambda: rng.rand(T1, T2), "ties": lambda: rng.randint(0, 3, (T1, T2)).astype(np.float64),
                     "zeros": lambda: np.zeros((T1, T2))}[kind]()
                want_cost, want_path = R.brute_force(d)
                for fn in (R.dtw_on_cost, R.dtw_fast):
                    total, pi, pj, _ = fn(d)
                    assert total == want_cost, (T1, T2, kind)                  # the optimum, bit for bit (the same adds in path order)
                    assert list(zip(pi.tolist(), pj.tolist())) == want_path, (T1, T2, kind)   # and the path the tie rule picks
                    assert R.path_cost(d, pi, pj) == total
                n_tied += kind != "random"
    assert n_tied == 2 * 4 * len(shapes)


def test_oracle_forms_agree_on_larger_matrices():
    rng = np.random.RandomState(1)
    for T1, T2 in ((17, 40), (40, 17), (33, 33)):
        for d in (rng.rand(T1, T2), rng.randint(0, 2, (T1, T2)).astype(np.float64)):
            a, b = R.dtw_on_cost(d), R.dtw_fast(d)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_dct_rows_are_orthonormal():
    for n_mel, K in ((80, 13), (80, 40), (128, 40), (20, 5)):
        C = M.dct_table(n_mel, K)
        assert C.dtype == np.float64 and C.shape == (K, n_mel)
        assert np.abs(C @ C.T - np.eye(K)).max() < 1e-14
        assert np.abs(C.sum(axis=1)).max() < 1e-13                             # every row k >= 1 is orthogonal to the level (c0)
        assert np.abs(C - R.dct_table(n_mel, K)).max() < 1e-15
    for bad in ((80, 0), (80, 41), (129, 13), (10, 10)):
        with pytest.raises(ValueError):
            M.dct_table(*bad)


def test_an_utterance_against_itself():
    rng = np.random.RandomState(2)
    mel = rng.randn(80, 50) * 2 - 5
    c = R.cepstra(mel)
    total, pi, pj = R.dtw(c, c)
    assert total == 0.0 and np.array_equal(pi, np.arange(50)) and np.array_equal(pj, np.arange(50))
    row = R.score_pair(mel, mel)
    assert row["mcd_db"] == 0.0 and row["path_len"] == 50 and row["frames_ref"] == row["frames_syn"] == 50


def test_repeated_frames_cost_nothing_and_the_path_is_the_repeat_map():
    rng = np.random.RandomState(3)
    a = rng.randn(23, 13)
    a[1:] += 10.0 * np.arange(1, 23)[:, None]                                  # no two frames alike
    reps = rng.randint(1, 5, 23)
    idx = np.repeat(np.arange(23), reps)
    total, pi, pj = R.dtw(a, a[idx])
    assert total == 0.0
    assert np.array_equal(pi, idx) and np.array_equal(pj, np.arange(len(idx)))
    total, pi, pj = R.dtw(a[idx], a)                                           # and with the sides exchanged
    assert total == 0.0 and np.array_equal(pi, np.arange(len(idx))) and np.array_equal(pj, idx)


def test_mcd_of_two_constant_cepstra():
    """a_k = u_k, b_k = v_k in every frame: d = |u - v| in every cell, the tie rule takes the diagonal first, so the path has max(T1, T2)
    cells, D = P |u - v| and MCD = (10 / ln 10) sqrt(2) |u - v| whatever the lengths."""
    u, v = np.arange(13.0), np.arange(13.0) + np.array([3.0, 4.0] + [0.0] * 11)  # |u - v| = 5
    for T1, T2 in ((7, 7), (9, 4), (3, 11)):
        total, pi, pj = R.dtw(np.tile(u, (T1, 1)), np.tile(v, (T2, 1)))
        assert len(pi) == max(T1, T2) and total == 5.0 * max(T1, T2)
        row = R.scores(total, pi, pj, T1, T2)
        assert row["mcd_db"] == pytest.approx(10.0 / math.log(10.0) * math.sqrt(2.0) * 5.0, rel=1e-15)
        assert M.scores_from_sums(total, len(pi), T1, T2) == row
    assert M.MCD_SCALE == R.MCD_SCALE


def test_f0_scores_on_hand_made_tracks():
    pi, pj = np.array([0, 1, 2, 3, 3, 4]), np.array([0, 1, 1, 2, 3, 4])
    ref = np.array([0.0, 100.0, 100.0, 200.0, 0.0])
    syn = np.array([0.0, 200.0, 0.0, 100.0, 50.0])
    # cells: (0,0) both unvoiced; (1,1) +1200; (2,1) +1200; (3,2) mismatch; (3,3) -1200; (4,4) mismatch
    assert R.f0_sums(pi, pj, ref, syn) == (2, 3, 3 * 1200.0 ** 2)
    row = R.scores(1.0, pi, pj, 5, 5, ref, syn)
    assert row["vuv_error"] == 2 / 6 and row["f0_rmse_cents"] == 1200.0 and row["n_voiced_pairs"] == 3
    assert M.scores_from_sums(1.0, 6, 5, 5, np.array([2.0, 3.0, 3 * 1200.0 ** 2])) == row
    # a semitone up everywhere
    r = np.full(8, 220.0)
    row = R.scores(0.0, np.arange(8), np.arange(8), 8, 8, r, r * 2 ** (1 / 12))
    assert row["f0_rmse_cents"] == pytest.approx(100.0, rel=1e-12) and row["vuv_error"] == 0.0
    # nothing voiced on both sides at once: NaN, and the V/UV error still counts
    row = R.scores(0.0, np.arange(4), np.arange(4), 4, 4, np.array([0.0, 0.0, 100.0, 0.0]), np.array([0.0, 90.0, 0.0, 0.0]))
    assert math.isnan(row["f0_rmse_cents"]) and row["n_voiced_pairs"] == 0 and row["vuv_error"] == 0.5
    got = M.scores_from_sums(0.0, 4, 4, 4, np.array([2.0, 0.0, 0.0]))
    assert math.isnan(got["f0_rmse_cents"]) and got["n_voiced_pairs"] == 0 and got["vuv_error"] == 0.5
    row = R.scores(0.0, np.arange(3), np.arange(3), 3, 3, np.zeros(3), np.zeros(3))                   # all unvoiced
    assert math.isnan(row["f0_rmse_cents"]) and row["vuv_error"] == 0.0


def test_summary_matches_the_oracle():
    rows = [{"mcd_db": 4.0, "path_len": 100, "vuv_error": 0.1, "f0_rmse_cents": 50.0, "n_voiced_pairs": 60},
            {"mcd_db": 6.0, "path_len": 300, "vuv_error": 0.3, "f0_rmse_cents": float("nan"), "n_voiced_pairs": 0},
            {"mcd_db": 5.0, "path_len": 200, "vuv_error": 0.2, "f0_rmse_cents": 150.0, "n_voiced_pairs": 20}]
    got = M.summarize(rows)
    assert got == R.summarize(rows)
    assert got["mcd_db_mean"] == 5.0 and got["mcd_db_weighted"] == pytest.approx((400 + 1800 + 1000) / 600)
    assert got["f0_nan_utterances"] == 1 and got["f0_rmse_cents_mean"] == 100.0
    assert got["f0_rmse_cents_weighted"] == pytest.approx((50 * 60 + 150 * 20) / 80)
    assert M.summarize([{"mcd_db": 1.0, "path_len": 3}]) == {"utterances": 1, "mcd_db_mean": 1.0, "mcd_db_weighted": 1.0}
    assert M.summarize([]) == {"utterances": 0}


def test_long_sequences_and_host_tensors_are_refused_before_any_launch():
    a = torch.zeros(1, M.MAX_FRAMES + 1, 13, dtype=torch.float64)
    b = torch.zeros(1, 8, 13, dtype=torch.float64)
    for fn in (M.dtw, M.local_cost):
        with pytest.raises(ValueError, match="2049 frames"):                   # the length is refused first, on any device
            fn(a, [M.MAX_FRAMES + 1], b, [8])
        with pytest.raises(ValueError, match="2049 frames"):
            fn(b, [8], a, [M.MAX_FRAMES + 1])
        with pytest.raises(ValueError, match="0 frames"):
            fn(b, [0], b, [8])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(b, [8], b, [8])
    with pytest.raises(ValueError, match="2049 frames"):
        M.scan(torch.zeros(1, 8, M.MAX_FRAMES + 1, dtype=torch.float64), [M.MAX_FRAMES + 1], [8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.scan(torch.zeros(1, 8, 8, dtype=torch.float64), [8], [8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.cepstra(torch.zeros(1, 80, 8), [8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.f0_on_path(torch.zeros(1, 15, dtype=torch.int32), torch.zeros(1, 15, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                     torch.zeros(1, 8, dtype=torch.float64), [8], torch.zeros(1, 8, dtype=torch.float64), [8])

    class Stft:                                                                # what score_pairs reads before the device stage
        hop_length, filter_length, n_mel_channels = 256, 1024, 80
    long = np.zeros(M.MAX_FRAMES * 256, np.float32)                            # 2049 frames
    ok = np.zeros(4000, np.float32)
    with pytest.raises(ValueError, match="2049 frames"):
        M.score_pairs([long], [ok], Stft, 22050, 256, f0=False)
    with pytest.raises(ValueError, match="too short"):
        M.score_pairs([ok], [ok[:512]], Stft, 22050, 256, f0=False)
    with pytest.raises(ValueError):
        M.score_pairs([ok], [ok], Stft, 22050, 256, n_mcep=41)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.score_pairs([ok], [ok], Stft, 22050, 256, device="cpu")
    assert M.frame_counts(2047 * 256, 22050, 256, f0=False) == 2048


def test_the_abi_refuses_long_sequences_before_launch():
    from fastspeech2_amd import _lib
    assert M.max_frames() == M.MAX_FRAMES == 2048
    one = torch.zeros(16, dtype=torch.float64)                                 # never dereferenced: the shape is refused first
    p = one.data_ptr()
    with pytest.raises(ValueError, match="supported maximum"):
        _lib.call("fs2_dtw_scan", p, 2049 * 8, 2049, p, p, p, 2049 * 8, 2049, p, 1, 2049, 8, None)
    with pytest.raises(ValueError, match="supported maximum"):
        _lib.call("fs2_dtw_cost", p, 8 * 13, 13, p, p, 2049 * 13, 13, p, 13, p, 2049 * 8, 8, 1, 8, 2049, None)
    with pytest.raises(ValueError, match="supported maximum"):
        _lib.call("fs2_dtw_backtrack", p, 2049 * 8, 2049, p, p, p, p + 8, 5000, p, 1, 2049, 8, None)
    with pytest.raises(ValueError):
        _lib.call("fs2_mcep", p, 80 * 8, 8, p, p, 41, p, 8 * 41, 41, 1, 80, 8, None)      # K above 40
    with pytest.raises(ValueError):
        _lib.call("fs2_dtw_f0", p, p, 15, p, p, 4, p, 8, p, p, p, 3, 1, 8, 8, None)       # reference row shorter than T1max
    with pytest.raises(ValueError):
        _lib.call("fs2_dtw_scan", None, 64, 8, p, p, p, 64, 8, p, 1, 8, 8, None)          # null pointer


# ------------------------------------------------------------------------------------------------ score.py through score_fn
SR, HOP = 22050, 256


def write_wav(path, n, sr=SR, seed=0):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, (np.random.RandomState(seed).uniform(-0.5, 0.5, n) * 32767).astype(np.int16))


@pytest.fixture()
def corpus(tmp_path):
    """Five metadata lines: u0 has a TextGrid (speech from 0.5 s to 1.25 s), u1 has none, u2 has no synthesized file, u3 has no
    recording, u4's synthesized file is too short for the STFT."""
    root = str(tmp_path)
    cfg = config(root)
    train = {"path": {"result_path": os.path.join(root, "result")}}
    for name, n in (("u0", 2 * SR), ("u1", SR), ("u2", SR), ("u4", SR)):
        write_wav(os.path.join(root, "raw", "spk", name + ".wav"), n, seed=len(name) + n)
    for name, n in (("u0", 17000), ("u1", 23000), ("u3", 9000), ("u4", 300)):
        write_wav(os.path.join(root, "result", name + ".wav"), n, seed=n)
    os.makedirs(os.path.join(root, "pre", "TextGrid", "spk"))
    A.write_textgrid(os.path.join(root, "pre", "TextGrid", "spk", "u0.TextGrid"), [(0.5, 1.25, "word")],
                     [(0.0, 0.5, "sil"), (0.5, 1.0, "AA"), (1.0, 1.25, "B"), (1.25, 2.0, "sp")], 2.0)
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"u{k}|spk|{{AA B}}|text {k}\n" for k in range(5)))
    for name, doc in (("preprocess.yaml", cfg), ("train.yaml", train)):
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    return root


def fake_scores(seen):
    def fn(refs, syns):
        seen.append(([len(r) for r in refs], [len(s) for s in syns], [r.dtype for r in refs]))
        return [{"mcd_db": float(len(r)) / 1000, "path_len": len(s), "frames_ref": len(r) // HOP + 1, "frames_syn": len(s) // HOP + 1}
                for r, s in zip(refs, syns)]
    return fn


def run_cli(root, extra, seen):
    import score
    out = os.path.join(root, "scores.jsonl")
    argv = ["-p", os.path.join(root, "preprocess.yaml"), "-t", os.path.join(root, "train.yaml"), "--source",
            os.path.join(root, "val.txt"), "--out", out] + extra
    rows, skipped, summary = score.main(argv, score_fn=fake_scores(seen))
    with open(out) as f:
        written = [json.loads(line) for line in f]
    assert written == rows
    return rows, skipped, summary


def test_cli_pairs_trims_skips_and_writes(corpus, capsys):
    seen = []
    rows, skipped, summary = run_cli(corpus, [], seen)
    assert [r["basename"] for r in rows] == ["u0", "u1"]
    window = int(SR * 1.25) - int(SR * 0.5)                                    # the preprocessor's own slice of the recording
    assert seen == [([window, SR], [17000, 23000], [np.dtype(np.float32)] * 2)]
    assert [r["reference_window"] for r in rows] == ["textgrid", "whole"]
    assert rows[0]["speaker"] == "spk" and rows[0]["mcd_db"] == window / 1000 and rows[1]["path_len"] == 23000
    assert [s[0] for s in skipped] == ["u2", "u3", "u4"]
    assert "result" in skipped[0][1] and "u2.wav" in skipped[0][1] and "missing" in skipped[0][1]
    assert os.path.join("raw", "spk", "u3.wav") in skipped[1][1]
    assert "300 samples" in skipped[2][1]
    assert summary["utterances"] == 2 and summary["skipped"] == 3 and summary["reference_window"] == {"textgrid": 1, "whole": 1}
    assert summary["mcd_db_weighted"] == pytest.approx((window / 1000 * 17000 + SR / 1000 * 23000) / 40000)
    out = capsys.readouterr().out.strip().splitlines()
    assert [ln.split(":")[0] for ln in out[:3]] == ["skipped u2", "skipped u3", "skipped u4"]       # never silently
    assert json.loads(out[-1]) == summary


def test_cli_no_trim_and_other_folders(corpus):
    seen = []
    rows, skipped, _ = run_cli(corpus, ["--no_trim"], seen)
    assert seen[0][0] == [2 * SR, SR] and [r["reference_window"] for r in rows] == ["whole", "whole"]
    # --ref_dir / --syn_dir: {dir}/{basename}.wav on both sides
    alt = os.path.join(corpus, "alt")
    write_wav(os.path.join(alt, "ref", "u1.wav"), 12345)
    write_wav(os.path.join(alt, "syn", "u1.wav"), 6789)
    seen = []
    rows, skipped, _ = run_cli(corpus, ["--ref_dir", os.path.join(alt, "ref"), "--syn_dir", os.path.join(alt, "syn")], seen)
    assert [r["basename"] for r in rows] == ["u1"] and seen[0][:2] == ([12345], [6789])
    assert len(skipped) == 4 and all("missing" in s[1] for s in skipped)
    # a recording longer than the scan supports is listed, not passed on
    write_wav(os.path.join(alt, "ref", "u0.wav"), 2048 * HOP)
    write_wav(os.path.join(alt, "syn", "u0.wav"), 5000)
    seen = []
    rows, skipped, _ = run_cli(corpus, ["--no_trim", "--ref_dir", os.path.join(alt, "ref"), "--syn_dir", os.path.join(alt, "syn")], seen)
    assert [r["basename"] for r in rows] == ["u1"] and ("u0", "reference has 2049 frames, more than the supported 2048") in skipped


def test_audio_at_another_rate_is_refused(corpus):
    write_wav(os.path.join(corpus, "result", "u1.wav"), 16000, sr=16000)
    with pytest.raises(ValueError, match=r"16000 Hz.*prepare_align\.py.*--resample gpu"):
        M.load_audio(os.path.join(corpus, "result", "u1.wav"), SR)
    with pytest.raises(SystemExit, match="prepare_align.py"):
        run_cli(corpus, [], [])
