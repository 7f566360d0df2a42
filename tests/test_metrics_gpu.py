"""Objective scoring on the GPU (fastspeech2_amd.metrics, csrc/fs2_dtw.hip) against the numpy oracle tests/dtw_ref.py: every kernel
on ragged batches whose padding is NaN (a sentinel in the integer buffers) in every input and every output, outputs as strided
views, exact agreement on integer-valued cepstra at every workgroup size, the project's fp64 bar on real-valued ones,
run-to-run determinism, and score.py end to end on tone sequences with time-stretched and pitch-shifted variants."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import audio as Audio
from fastspeech2_amd import metrics as M
from fastspeech2_amd import pitch as Pitch
from tests import dtw_ref as R
from tests import f0_signals as S
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu
RTOL = 1e-6                                                                # the project's bar for fp64 kernels (tests/test_align_gpu.py:20)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
K = 13
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (300, 57), (1024, 1025), (2048, 1500), (2048, 2048)]


def padded(arrays, fill, dtype, dev, extra=0):
    """[(T_b, W)] -> (B, Tmax + extra, W) device tensor, everything outside the arrays = fill"""
    T = max(a.shape[0] for a in arrays) + extra
    out = np.full((len(arrays), T) + arrays[0].shape[1:], fill, dtype)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return torch.from_numpy(out).to(dev)


def integer_pair(rng, T1, T2):
    """Small-integer cepstra drawn from a pool of 6 frames, in runs of 1-4 equal frames: zero-cost cells and exact ties everywhere."""
    pool = rng.randint(-3, 4, (6, K)).astype(np.float64)

    def seq(T):
        idx = np.repeat(rng.randint(0, 6, T), rng.randint(1, 5, T))[:T]
        return pool[idx]
    return seq(T1), seq(T2)


@pytest.fixture(scope="module")
def integer_cases():
    rng = np.random.RandomState(11)
    cases = []
    for T1, T2 in SIZES:
        a, b = integer_pair(rng, T1, T2)
        d = R.local_cost(a, b)
        total, pi, pj, bp = R.dtw_fast(d)
        cases.append({"a": a, "b": b, "d": d, "total": total, "pi": pi, "pj": pj, "bp": bp})
    return cases


def run_dtw_checked(dev, cases, exact):
    """The four stages on one ragged batch with poisoned padding and strided outputs; everything outside a pair must be untouched.
    Returns the per-pair (total, pi, pj)."""
    al, bl = [len(c["a"]) for c in cases], [len(c["b"]) for c in cases]
    B, T1, T2 = len(cases), max(al), max(bl)
    a = padded([c["a"] for c in cases], NAN, np.float64, dev, extra=2)
    b = padded([c["b"] for c in cases], NAN, np.float64, dev)
    cost = torch.full((B, T2 + 1, T1 + 3), NAN, dtype=torch.float64, device=dev)[:, :T2, :T1]        # strided views
    bp = torch.full((B, T2, T1 + 5), 77, dtype=torch.uint8, device=dev)[:, :, :T1]
    L = T1 + T2 - 1
    pi = torch.full((B, L + 4), -77, dtype=torch.int32, device=dev)[:, :L]
    pj = torch.full((B, L + 4), -77, dtype=torch.int32, device=dev)[:, :L]
    assert M.local_cost(a, al, b, bl, out=cost).data_ptr() == cost.data_ptr()
    _, total = M.scan(cost, al, bl, out=bp)
    plen, _, _ = M.backtrack(bp, al, bl, out=(pi, pj))
    total, plen = total.cpu().numpy(), plen.cpu().numpy()
    pi, pj = pi.cpu().numpy(), pj.cpu().numpy()
    out = []
    for p, c in enumerate(cases):
        t1, t2 = al[p], bl[p]
        skew_d, skew_bp = cost[p].cpu().numpy(), bp[p].cpu().numpy()
        i, j = np.meshgrid(np.arange(t1), np.arange(t2), indexing="ij")
        got_d, got_bp = skew_d[(i + j) % t2, i], skew_bp[(i + j) % t2, i]
        rest_d, rest_bp = skew_d.copy(), skew_bp.copy()
        rest_d[:t2, :t1], rest_bp[:t2, :t1] = NAN, 77
        assert np.isnan(rest_d).all() and (rest_bp == 77).all(), p                # padding is never written
        P = int(plen[p])
        assert (pi[p, P:t1 + t2 - 1] == -1).all() and (pj[p, P:t1 + t2 - 1] == -1).all(), p
        assert (pi[p, t1 + t2 - 1:] == -77).all() and (pj[p, t1 + t2 - 1:] == -77).all(), p
        if exact:
            assert np.array_equal(got_d, c["d"]), p                               # squares, sums and the rounded root, bit for bit
            assert np.array_equal(got_bp, c["bp"]), p
            assert total[p] == c["total"], (p, total[p], c["total"])
            assert P == len(c["pi"]) and np.array_equal(pi[p, :P], c["pi"]) and np.array_equal(pj[p, :P], c["pj"]), p
        out.append((total[p], pi[p, :P].copy(), pj[p, :P].copy()))
    return out


def test_cepstra_against_oracle(dev):
    rng = np.random.RandomState(3)
    mels = [(rng.randn(80, T) * 2.5 - 5).astype(np.float32) for T in (57, 1, 300, 2, 513)]
    lens = [m.shape[1] for m in mels]
    mel = padded([m.T for m in mels], NAN, np.float32, dev, extra=3).transpose(1, 2).contiguous()
    for n_mcep in (13, 40, 1):
        out = torch.full((len(mels), max(lens) + 2, n_mcep + 3), NAN, dtype=torch.float64, device=dev)[:, :max(lens), :n_mcep]
        c = M.cepstra(mel, lens, n_mcep, out=out).cpu().numpy()
        for b, m in enumerate(mels):
            want, bound = R.cepstra(m, n_mcep), R.cepstra_bound(m, n_mcep)
            err = np.abs(c[b, :lens[b]] - want)
            print("cepstra n_mcep", n_mcep, "T", lens[b], "max err / bound", float((err / bound).max()))
            assert (err <= bound).all(), (n_mcep, b, float((err / bound).max()))
            assert np.isnan(c[b, lens[b]:]).all()
    whole = M.cepstra(mel, lens).cpu().numpy()                             # its own buffer: the same values
    assert np.array_equal(whole[2, :300], M.cepstra(mel, lens, out=torch.empty(5, 520, 13, dtype=torch.float64, device=dev))
                          .cpu().numpy()[2, :300])
    with pytest.raises(ValueError):
        M.cepstra(mel, lens, 41)
    with pytest.raises(ValueError):
        M.cepstra(mel, [600, 1, 1, 1, 1])                                  # longer than the buffer
    with pytest.raises(ValueError):
        M.cepstra(mel.double(), lens)


@pytest.mark.parametrize("n", range(len(SIZES)))
def test_dtw_is_exact_on_integer_cepstra(dev, integer_cases, n):
    run_dtw_checked(dev, [integer_cases[n]], exact=True)


def test_dtw_is_exact_on_a_mixed_batch(dev, integer_cases):
    order = [4, 7, 0, 5, 2, 6, 1, 3]                                        # not sorted: a pair's result must not depend on its row
    got = run_dtw_checked(dev, [integer_cases[n] for n in order], exact=True)
    ties = sum(1 for n in order if (integer_cases[n]["d"] == 0).sum() > 1)
    assert ties >= 5 and len(got) == 8
    c = integer_cases[4]                                                    # and the one-call form on plain buffers
    total, plen, pi, pj = M.dtw(padded([c["a"]], NAN, np.float64, dev), [300], padded([c["b"]], NAN, np.float64, dev), [57])
    P = int(plen[0])
    assert float(total[0]) == c["total"] and np.array_equal(pi[0, :P].cpu().numpy(), c["pi"]) \
        and np.array_equal(pj[0, :P].cpu().numpy(), c["pj"])


def test_dtw_on_real_valued_cepstra(dev):
    rng = np.random.RandomState(5)
    cases = []
    for T1, T2 in ((300, 57), (57, 300), (1, 1), (1, 9), (1024, 1025), (700, 911), (1500, 640), (2, 2)):
        # a slowly varying trajectory, the second a warped noisy copy: the kind of pair the scores are for
        base = np.cumsum(rng.randn(max(T1, T2) + 8, K), axis=0) * 0.3
        a = base[np.sort(rng.randint(0, len(base), T1))] + 0.05 * rng.randn(T1, K)
        b = base[np.sort(rng.randint(0, len(base), T2))] + 0.05 * rng.randn(T2, K)
        cases.append({"a": a, "b": b})
    got = run_dtw_checked(dev, cases, exact=False)
    for p, (c, (total, pi, pj)) in enumerate(zip(cases, got)):
        d = R.local_cost(c["a"], c["b"])
        want, _, _, _ = R.dtw_fast(d)
        T1, T2 = d.shape
        print("pair", p, (T1, T2), "total", total, "oracle", want, "rel", abs(total - want) / max(want, 1e-300))
        assert abs(total - want) <= RTOL * abs(want), (p, total, want)
        assert (pi[0], pj[0]) == (0, 0) and (pi[-1], pj[-1]) == (T1 - 1, T2 - 1), p
        steps = set(zip(np.diff(pi).tolist(), np.diff(pj).tolist()))
        assert steps <= {(1, 1), (1, 0), (0, 1)}, (p, steps)
        again = R.path_cost(d, pi, pj)                                     # the GPU's path, priced by the oracle's own costs
        assert abs(again - want) <= 1e-9 * abs(want), (p, again, want)


def f0_track(rng, T, voiced_share):
    f = 120.0 * 2.0 ** rng.uniform(-0.5, 1.0, T)
    seg = np.repeat(rng.rand(T // 5 + 1) < voiced_share, 5)[:T]
    return np.where(seg, f, 0.0)


def test_f0_sums_against_oracle_on_the_oracles_path(dev, integer_cases):
    rng = np.random.RandomState(8)
    picks = [integer_cases[n] for n in (4, 5, 3, 0, 1, 6)]
    al, bl = [len(c["a"]) for c in picks], [len(c["b"]) for c in picks]
    share = [(0.7, 0.7), (0.6, 0.8), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0), (0.5, 0.5)]            # pair 3 and 4: nothing voiced on both sides
    fr = [f0_track(rng, t, s[0]) for t, s in zip(al, share)]
    fs = [f0_track(rng, t, s[1]) for t, s in zip(bl, share)]
    L = max(al) + max(bl) - 1
    pi = np.full((len(picks), L + 2), -77, np.int32)
    pj = np.full((len(picks), L + 2), -77, np.int32)
    for p, c in enumerate(picks):
        pi[p, :len(c["pi"])], pj[p, :len(c["pj"])] = c["pi"], c["pj"]
    plen = torch.tensor([len(c["pi"]) for c in picks], dtype=torch.int32, device=dev)
    f0r = padded([f[:, None] for f in fr], NAN, np.float64, dev)[:, :, 0].contiguous()
    f0s = padded([f[:, None] for f in fs], NAN, np.float64, dev)[:, :, 0].contiguous()
    buf = torch.full((len(picks), 5), NAN, dtype=torch.float64, device=dev)
    out = buf[:, 1:4]                                                                              # a strided view
    sums = M.f0_on_path(torch.from_numpy(pi).to(dev)[:, :L], torch.from_numpy(pj).to(dev)[:, :L], plen, f0r, al, f0s, bl, out=out)
    assert sums.data_ptr() == out.data_ptr()
    whole = sums.cpu().numpy()
    n_nan = 0
    for p, c in enumerate(picks):
        mism, voiced, sq = R.f0_sums(c["pi"], c["pj"], fr[p], fs[p])
        assert whole[p, 0] == mism and whole[p, 1] == voiced, p                                    # counts exact
        assert abs(whole[p, 2] - sq) <= RTOL * abs(sq), p
        got = M.scores_from_sums(c["total"], len(c["pi"]), al[p], bl[p], whole[p])
        want = R.scores(c["total"], c["pi"], c["pj"], al[p], bl[p], fr[p], fs[p])
        if math.isnan(want["f0_rmse_cents"]):
            assert math.isnan(got["f0_rmse_cents"]) and got["n_voiced_pairs"] == 0
            n_nan += 1
        else:
            assert abs(got["f0_rmse_cents"] - want["f0_rmse_cents"]) <= RTOL * want["f0_rmse_cents"]
        assert got["vuv_error"] == want["vuv_error"] and got["mcd_db"] == want["mcd_db"]
    assert n_nan == 2
    assert torch.isnan(buf[:, [0, 4]]).all()


def test_bad_arguments(dev):
    a = torch.zeros(2, 8, K, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        M.dtw(a, [8, 8], a[:1], [8])                                       # one side has fewer pairs
    with pytest.raises(ValueError):
        M.dtw(a, [8], a, [8, 8])                                           # lens does not match the batch
    with pytest.raises(ValueError):
        M.dtw(a, [9, 8], a, [8, 8])                                        # longer than the buffer
    with pytest.raises(ValueError):
        M.dtw(a.float(), [8, 8], a, [8, 8])
    with pytest.raises(ValueError):
        M.local_cost(a, [8, 8], a, [8, 8], out=torch.zeros(2, 8, 7, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        M.scan(torch.zeros(2, 8, 8, dtype=torch.float64, device=dev), [8, 9], [8, 8])


# ------------------------------------------------------------------------------------------------ audio
def tones(f0s, durs, gap=0.12):
    parts = []
    for k, (f, d) in enumerate(zip(f0s, durs)):
        if k:
            parts.append(np.zeros(int(gap * S.FS), np.float32))
        parts.append(S.tone(f, d))
    return np.concatenate(parts)


SHIFT_CENTS = 100.0
BASE_F0, BASE_DUR = (200.0, 260.0, 150.0, 330.0), (0.45, 0.3, 0.5, 0.35)


def make_pairs():
    """name -> (recorded, synthesized): identical, time-stretched, pitch-shifted by SHIFT_CENTS, both, and another melody."""
    up = 2.0 ** (SHIFT_CENTS / 1200.0)
    base = tones(BASE_F0, BASE_DUR)
    return {"same": (base, base.copy()),
            "stretch": (base, tones(BASE_F0, [d * s for d, s in zip(BASE_DUR, (1.3, 0.8, 1.2, 1.4))])),
            "shift": (base, tones([f * up for f in BASE_F0], BASE_DUR)),
            "both": (base, tones([f * up for f in BASE_F0], [d * 1.25 for d in BASE_DUR])),
            "other": (base, tones((110.0, 450.0, 240.0), (0.5, 0.4, 0.6)))}


def stft_of(cfg):
    pp = cfg["preprocessing"]
    return Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"],
                              pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])


def test_two_runs_of_score_pairs_are_byte_identical(dev):
    pairs = make_pairs()
    stft = stft_of(config("/nowhere"))
    refs, syns = [p[0] for p in pairs.values()], [p[1] for p in pairs.values()]
    first = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev)
    second = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev)
    small = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, budget=1)        # one pair per batch: the same scores
    assert json.dumps(first) == json.dumps(second) == json.dumps(small)
    assert all(r["frames_ref"] in (len(w) // S.HOP, len(w) // S.HOP + 1) for r, w in zip(first, refs))      # cut to DIO's count
    no_f0 = M.score_pairs(refs, syns, stft, S.FS, S.HOP, f0=False, device=dev)
    assert all("vuv_error" not in r and r["mcd_db"] >= 0 for r in no_f0)


def test_score_command_line_end_to_end(dev, tmp_path):
    """score.py in a subprocess on 16-bit wav files; its JSON must equal the oracle applied to the GPU's own mels and F0 tracks of
    the same files.  Floats are compared at the fp64 bar (the oracle's cepstra differ from the kernel's in the last bits); path
    lengths and counts are compared exactly."""
    from scipy.io import wavfile
    root = str(tmp_path)
    cfg = config(root)
    pairs = make_pairs()
    os.makedirs(os.path.join(root, "raw", "spk"))
    os.makedirs(os.path.join(root, "result"))
    for name, (ref, syn) in pairs.items():
        wavfile.write(os.path.join(root, "raw", "spk", name + ".wav"), S.FS, np.round(ref * 32767).astype(np.int16))
        wavfile.write(os.path.join(root, "result", name + ".wav"), S.FS, np.round(syn * 32767).astype(np.int16))
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("".join(f"{name}|spk|{{AA}}|text\n" for name in list(pairs) + ["absent"]))
    for name, doc in (("preprocess.yaml", cfg), ("train.yaml", {"path": {"result_path": os.path.join(root, "result")}})):
        with open(os.path.join(root, name), "w") as f:
            yaml.safe_dump(doc, f)
    out = os.path.join(root, "scores.jsonl")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "score.py"), "-p", os.path.join(root, "preprocess.yaml"), "-t",
                          os.path.join(root, "train.yaml"), "--source", os.path.join(root, "val.txt"), "--out", out],
                         capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "skipped absent: missing" in run.stdout
    rows = {r["basename"]: r for r in map(json.loads, open(out))}
    assert list(rows) == list(pairs) and all(r["reference_window"] == "whole" for r in rows.values())
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["utterances"] == 5 and summary["skipped"] == 1

    # the oracle on the GPU's own features of the very files
    stft = stft_of(cfg)
    want = {}
    for name in pairs:
        feats = []
        for path in (os.path.join(root, "raw", "spk", name + ".wav"), os.path.join(root, "result", name + ".wav")):
            w = torch.from_numpy(M.load_audio(path, S.FS)).to(dev).unsqueeze(0)
            mel, _, fr = stft.mel_spectrogram_ragged(w.clamp(-1.0, 1.0), [w.shape[1]])
            f0, _, f0_frames = Pitch.dio_stonemask(w, [w.shape[1]], S.FS, S.FRAME_PERIOD)
            feats += [mel[0, :, :int(fr[0])].cpu().numpy(), f0[0, :int(f0_frames[0])]]
        want[name] = R.score_pair(feats[0], feats[2], feats[1], feats[3])
    for name, w in want.items():
        got = rows[name]
        print(name, "got", {k: got[k] for k in w}, "oracle", w)
        for key in ("path_len", "frames_ref", "frames_syn", "n_voiced_pairs"):
            assert got[key] == w[key], (name, key)
        for key in ("mcd_db", "vuv_error", "f0_rmse_cents"):
            assert abs(got[key] - w[key]) <= RTOL * abs(w[key]), (name, key, got[key], w[key])
    for key in ("mcd_db_mean", "mcd_db_weighted", "vuv_error_mean", "f0_rmse_cents_weighted"):
        assert abs(summary[key] - R.summarize(list(want.values()))[key]) <= RTOL * abs(R.summarize(list(want.values()))[key])

    same = rows["same"]
    assert same["mcd_db"] == 0.0 and same["vuv_error"] == 0.0 and same["f0_rmse_cents"] == 0.0
    assert same["path_len"] == same["frames_ref"] == same["frames_syn"] and same["n_voiced_pairs"] > 50
    assert rows["stretch"]["mcd_db"] < rows["other"]["mcd_db"] and rows["shift"]["mcd_db"] > 0.0
    # the known shift: the oracle's own distance from it on these tracks is the tolerance (plus the fp64 bar on the GPU's figure)
    for name in ("shift", "both"):
        slack = abs(want[name]["f0_rmse_cents"] - SHIFT_CENTS)
        print(name, "cents", rows[name]["f0_rmse_cents"], "oracle", want[name]["f0_rmse_cents"], "oracle's distance from the shift", slack)
        assert abs(rows[name]["f0_rmse_cents"] - SHIFT_CENTS) <= slack + RTOL * SHIFT_CENTS, (name, rows[name], slack)
