"""Prosody scores on the GPU (fastspeech2_amd.metrics: voiced_contours, prosody_on_path, contour_dtw; csrc/fs2_prosody.hip and
fs2_dtw_prosody in csrc/fs2_dtw.hip) against the numpy oracle tests/prosody_ref.py: ragged batches whose padding is NaN in every
input and a sentinel in every output, outputs as strided views, counts and paths exact, float sums at the project's fp64 bar, and
`score_pairs(..., prosody=True)` / `score.py --prosody` end to end on tone sequences with known answers."""
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
from tests import prosody_ref as PR
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu
RTOL = 1e-6                                                                # the project's bar for fp64 kernels (tests/test_metrics_gpu.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
K = 13
SENTINEL = -77.0
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048)        # either side of a wave, the workgroup, the chunk carry
PATTERNS = ("none", "all", "first", "last", "alternating", "runs")
PATH_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (300, 57), (1024, 1025), (2048, 2048)]
PATH_SHARES = [(1.0, 1.0), (0.0, 1.0), (0.0, 0.0), (1.0, 1.0), (0.7, 0.7), (0.6, 0.8), (0.5, 0.5)]    # n = 1, 0, 0, then many


def close(got, want, scale=None):
    return abs(got - want) <= RTOL * abs(want if scale is None else scale)


def track(rng, T, pattern):
    f = np.round(120.0 * 2.0 ** rng.uniform(-0.5, 1.0, T), 2)
    v = np.zeros(T, bool)
    if pattern == "all":
        v[:] = True
    elif pattern == "first":
        v[0] = True
    elif pattern == "last":
        v[T - 1] = True
    elif pattern == "alternating":
        v[::2] = True
    elif pattern == "runs":
        v = np.repeat(rng.rand(T) < 0.6, rng.randint(1, 9, T))[:T]
    return np.where(v, f, 0.0)


def rows_to_device(rows, dev, extra=2, dtype=np.float64):
    """[(T_b,)] -> (B, Tmax + extra) device tensor, NaN outside the rows"""
    out = np.full((len(rows), max(len(r) for r in rows) + extra), NAN, dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return torch.from_numpy(out).to(dev)


def check_contours(dev, rows):
    lens = [len(r) for r in rows]
    B, Tmax = len(rows), max(lens)
    buf = torch.full((B, Tmax + 3), SENTINEL, dtype=torch.float64, device=dev)
    contour, n_v, stats = M.voiced_contours(rows_to_device(rows, dev), lens, out=buf[:, :Tmax])    # a strided view
    assert contour.data_ptr() == buf.data_ptr()
    got, n_v, stats = buf.cpu().numpy(), n_v.cpu().numpy(), stats.cpu().numpy()
    assert not np.isnan(got).any() and not np.isnan(stats).any()               # the NaN padding of the input was never read
    for b, r in enumerate(rows):
        u = PR.voiced(r)
        n, mean, m2, m3, m4 = PR.moments(u)
        assert n_v[b] == n and stats[b, 0] == n, (b, lens[b])
        assert np.array_equal(got[b, :n], u), (b, lens[b])                     # the same values in the same order, bit for bit
        assert (got[b, n:] == SENTINEL).all(), (b, lens[b])                    # nothing written beyond n_v
        assert close(stats[b, 1], mean) and close(stats[b, 2], m2) and close(stats[b, 4], m4), (b, lens[b], stats[b], (mean, m2, m4))
        assert close(stats[b, 3], m3, PR.m3_scale(u)), (b, lens[b], stats[b, 3], m3)
        if n == 0:
            assert (stats[b] == 0.0).all()


def test_compaction_and_moments(dev):
    rng = np.random.RandomState(21)
    rows = [track(rng, T, p) for T in LENGTHS for p in PATTERNS]
    order = rng.permutation(len(rows))                                         # a row's result must not depend on its place
    check_contours(dev, [rows[k] for k in order])
    for T, p in ((1, "all"), (1, "none"), (257, "runs"), (2048, "alternating"), (2048, "all")):
        check_contours(dev, [track(rng, T, p)])
    contour, n_v, _ = M.voiced_contours(rows_to_device(rows[:6], dev), [1] * 6)                    # its own buffer
    assert contour.shape == (6, 1) and n_v.tolist() == [0, 1, 1, 1, 1, int(rows[5][0] > 0)]


@pytest.fixture(scope="module")
def path_cases():
    """The oracle's own paths of integer-valued cepstral pairs, and F0 / energy tracks on them: integer reference F0, the synthesized
    F0 of a frame 1.2, 0.8 or a random multiple of the reference frame the path first pairs it with."""
    rng = np.random.RandomState(31)
    cases = []
    for (T1, T2), share in zip(PATH_SIZES, PATH_SHARES):
        pool = rng.randint(-3, 4, (6, K)).astype(np.float64)
        a = pool[np.repeat(rng.randint(0, 6, T1), rng.randint(1, 5, T1))[:T1]]
        b = pool[np.repeat(rng.randint(0, 6, T2), rng.randint(1, 5, T2))[:T2]]
        total, pi, pj = R.dtw(a, b)
        r = rng.randint(80, 301, T1).astype(np.float64)
        partner = np.zeros(T2, np.int64)
        partner[pj[::-1]] = pi[::-1]                                           # the first cell of the path in column j
        kind = rng.randint(0, 3, T2)
        s = np.where(kind == 0, 1.2 * r[partner], np.where(kind == 1, 0.8 * r[partner], r[partner] * rng.uniform(0.7, 1.4, T2)))
        vr = np.repeat(rng.rand(T1 // 5 + 1) < share[0], 5)[:T1]
        vs = np.repeat(rng.rand(T2 // 5 + 1) < share[1], 5)[:T2]
        cases.append({"pi": pi, "pj": pj, "T1": T1, "T2": T2, "fr": np.where(vr, r, 0.0), "fs": np.where(vs, s, 0.0),
                      "er": (rng.rand(T1) * 40).astype(np.float32), "es": (rng.rand(T2) * 40).astype(np.float32)})
    return cases


def test_path_sums_against_oracle_on_the_oracles_path(dev, path_cases):
    cs = path_cases
    al, bl = [c["T1"] for c in cs], [c["T2"] for c in cs]
    L = max(al) + max(bl) - 1
    pi = np.full((len(cs), L + 2), -77, np.int32)
    pj = np.full((len(cs), L + 2), -77, np.int32)
    for p, c in enumerate(cs):
        pi[p, :len(c["pi"])], pj[p, :len(c["pj"])] = c["pi"], c["pj"]
    assert [len(c["pi"]) for c in cs][:4] == [1, 7, 7, 2] and 256 < len(cs[4]["pi"]) < 1024 < len(cs[5]["pi"]) and len(cs[6]["pi"]) > 2048
    plen = torch.tensor([len(c["pi"]) for c in cs], dtype=torch.int32, device=dev)
    buf = torch.full((len(cs), 10), NAN, dtype=torch.float64, device=dev)
    out = buf[:, 1:9]                                                          # a strided view
    sums = M.prosody_on_path(torch.from_numpy(pi).to(dev)[:, :L], torch.from_numpy(pj).to(dev)[:, :L], plen,
                             rows_to_device([c["fr"] for c in cs], dev), al, rows_to_device([c["fs"] for c in cs], dev), bl,
                             rows_to_device([c["er"] for c in cs], dev, dtype=np.float32),
                             rows_to_device([c["es"] for c in cs], dev, dtype=np.float32), out=out)
    assert sums.data_ptr() == out.data_ptr()
    whole = sums.cpu().numpy()
    assert torch.isnan(buf[:, [0, 9]]).all() and not np.isnan(whole).any()
    n_zero = n_one = n_boundary = 0
    for p, c in enumerate(cs):
        q = PR.path_sums(c["pi"], c["pj"], c["fr"], c["fs"], c["er"], c["es"])
        P = len(c["pi"])
        got = whole[p]
        print("pair", p, (c["T1"], c["T2"]), "P", P, "gpu", got.tolist(), "oracle", q)
        assert (got[0], got[1], got[2]) == (q["gross"], q["n"], q["mism"]), p                      # counts exact
        assert close(got[3], q["sxx"]) and close(got[4], q["syy"]) and close(got[6], q["de"]) and close(got[7], q["se"]), p
        assert close(got[5], q["sxy"], math.sqrt(q["sxx"] * q["syy"])), p
        want = PR.path_scores(q, P)
        row = M.prosody_scores(got, P, [0] * 5, [0] * 5, NAN, 0)
        for key in ("gpe", "ffe", "f0_corr", "energy_mae", "energy_mae_rel"):
            if math.isnan(want[key]):
                assert math.isnan(row[key]), (p, key)
            elif key in ("gpe", "ffe"):
                assert row[key] == want[key], (p, key)
            else:
                assert close(row[key], want[key]), (p, key, row[key], want[key])
        n_zero += q["n"] == 0
        n_one += q["n"] == 1
        r, s = c["fr"][c["pi"]], c["fs"][c["pj"]]
        n_boundary += int(np.sum((r > 0) & (s > 0) & (np.abs(s - r) == 0.2 * r)))
    assert n_zero == 2 and n_one == 1 and n_boundary > 100                     # cells exactly on the 20 % boundary were there


def test_contour_dtw_is_exact_on_integer_contours(dev):
    rng = np.random.RandomState(41)
    counts = [(1, 1), (1, 7), (2, 2), (257, 64), (0, 9), (1025, 1024)]

    def with_gaps(n):
        u = np.repeat(rng.randint(100, 112, n), rng.randint(1, 4, n))[:n].astype(np.float64) if n else np.zeros(0)
        T = n + rng.randint(1, 40)
        f = np.zeros(T)
        f[np.sort(rng.permutation(T)[:n])] = u
        return f
    fr, fs = [with_gaps(n) for n, _ in counts], [with_gaps(n) for _, n in counts]
    u, nu, _ = M.voiced_contours(rows_to_device(fr, dev), [len(f) for f in fr])
    w, nw, _ = M.voiced_contours(rows_to_device(fs, dev), [len(f) for f in fs])
    assert list(zip(nu.tolist(), nw.tolist())) == counts
    total, plen, pi, pj, launched = M.contour_dtw(u, nu.cpu(), w, nw.cpu())
    assert launched == [0, 1, 2, 3, 5]                                         # the pair with an empty side reaches no kernel
    total, plen, pi, pj = total.cpu().numpy(), plen.cpu().numpy(), pi.cpu().numpy(), pj.cpu().numpy()
    for p in range(len(counts)):
        want_total, want_pi, want_pj = PR.contour_dtw(PR.voiced(fr[p]), PR.voiced(fs[p]))
        P = len(want_pi)
        assert plen[p] == P, p
        if P == 0:
            assert math.isnan(total[p]) and (pi[p] == -1).all() and (pj[p] == -1).all()
            continue
        assert total[p] == want_total, (p, total[p], want_total)               # integer Hz: bit for bit
        assert np.array_equal(pi[p, :P], want_pi) and np.array_equal(pj[p, :P], want_pj), p
        assert (pi[p, P:] == -1).all() and (pj[p, P:] == -1).all(), p
    row = M.prosody_scores([0] * 8, 1, [0] * 5, [0] * 5, total[4], plen[4])
    assert math.isnan(row["f0_dtw_hz"]) and row["f0_dtw_path_len"] == 0
    total, plen, _, _, launched = M.contour_dtw(u[4:5], [0], w[4:5], [9])       # nothing to launch at all
    assert launched == [] and math.isnan(float(total[0])) and int(plen[0]) == 0


def test_bad_arguments(dev):
    f = torch.zeros(2, 8, dtype=torch.float64, device=dev)
    e = torch.zeros(2, 8, dtype=torch.float32, device=dev)
    p = torch.zeros(2, 15, dtype=torch.int32, device=dev)
    n = torch.ones(2, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        M.voiced_contours(f.cpu(), [8, 8])                                     # host tensor
    with pytest.raises(ValueError):
        M.voiced_contours(f.float(), [8, 8])                                   # float32 F0
    with pytest.raises(ValueError):
        M.voiced_contours(f, [9, 8])                                           # longer than the buffer
    with pytest.raises(ValueError):
        M.voiced_contours(f, [8])                                              # lens does not match the batch
    with pytest.raises(ValueError):
        M.voiced_contours(torch.zeros(1, M.max_frames() + 1, dtype=torch.float64, device=dev), [M.max_frames() + 1])
    with pytest.raises(ValueError):
        M.voiced_contours(f, [8, 8], out=torch.zeros(2, 7, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        M.prosody_on_path(p, p.clone(), n, f.cpu(), [8, 8], f, [8, 8], e, e)
    with pytest.raises(ValueError):
        M.prosody_on_path(p, p.clone(), n, f.float(), [8, 8], f, [8, 8], e, e)
    with pytest.raises(ValueError):
        M.prosody_on_path(p, p.clone(), n, f, [8, 8], f, [8, 8], e.double(), e)                    # float64 energy
    with pytest.raises(ValueError):
        M.prosody_on_path(p, p.clone(), n, f, [9, 8], f, [8, 8], e, e)
    with pytest.raises(ValueError):
        M.prosody_on_path(p, p.clone(), n, f, [M.max_frames() + 1, 8], f, [8, 8], e, e)
    with pytest.raises(ValueError):
        M.contour_dtw(f.cpu(), [8, 8], f, [8, 8])
    with pytest.raises(ValueError):
        M.contour_dtw(f.float(), [8, 8], f, [8, 8])
    with pytest.raises(ValueError):
        M.contour_dtw(f, [9, 8], f, [8, 8])
    wav = S.tone(200.0, 0.3)
    with pytest.raises(ValueError, match="stft=None"):
        M.score_pairs([wav], [wav], None, S.FS, S.HOP, device=dev, cepstra="world", prosody=True)
    with pytest.raises(ValueError, match="f0=False"):
        M.score_pairs([wav], [wav], stft_of(config("/nowhere")), S.FS, S.HOP, device=dev, f0=False, prosody=True)


# ------------------------------------------------------------------------------------------------ audio
def stft_of(cfg):
    pp = cfg["preprocessing"]
    return Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"],
                              pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])


def gpu_features(stft, wav, dev):
    """(log-mel, F0, energy) of one waveform as score_pairs takes them: the GPU's own mel and energy of the clamped audio and its
    DIO + StoneMask track, so that the oracle is held against the scoring kernels and not against the front end's float32."""
    w = torch.from_numpy(wav).to(dev).unsqueeze(0)
    mel, energy, fr = stft.mel_spectrogram_ragged(w.clamp(-1.0, 1.0), [w.shape[1]])
    f0, _, f0_frames = Pitch.dio_stonemask(w, [w.shape[1]], S.FS, S.FRAME_PERIOD)
    n = int(fr[0])
    return mel[0, :, :n].cpu().numpy().astype(np.float64), f0[0, :int(f0_frames[0])], energy[0, :n].cpu().numpy()


def compare_row(name, got, want, m3_scales):
    """`got` against the oracle's row: counts exact, NaN where the oracle has NaN, floats at RTOL; the signed M3 at RTOL of
    sum |u - mean|^3 (`m3_scales` per side), because it may cancel."""
    print(name, "got", got, "oracle", want)
    assert got.keys() == want.keys(), sorted(set(got) ^ set(want))
    for key, w in want.items():
        g = got[key]
        if isinstance(w, dict):
            assert g["n"] == w["n"] and close(g["mean"], w["mean"]) and close(g["m2"], w["m2"]) and close(g["m4"], w["m4"]), (name, key)
            assert abs(g["m3"] - w["m3"]) <= RTOL * m3_scales[key], (name, key, g["m3"], w["m3"])
        elif isinstance(w, (int, np.integer)):
            assert g == w, (name, key, g, w)
        elif math.isnan(w):
            assert math.isnan(g), (name, key, g)
        else:
            assert close(g, float(w)), (name, key, g, w)


def test_score_pairs_with_prosody_on_tone_sequences(dev):
    pairs = PR.tone_pairs()
    stft = stft_of(config("/nowhere"))
    refs, syns = [p[0] for p in pairs.values()], [p[1] for p in pairs.values()]
    rows = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, prosody=True)
    again = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, prosody=True)
    small = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev, prosody=True, budget=1)      # one pair per batch: the same scores
    assert json.dumps(rows) == json.dumps(again) == json.dumps(small)
    plain = M.score_pairs(refs, syns, stft, S.FS, S.HOP, device=dev)
    today = {"mcd_db", "path_len", "frames_ref", "frames_syn", "vuv_error", "f0_rmse_cents", "n_voiced_pairs"}
    assert all(set(r) == today for r in plain)
    assert json.dumps([{k: r[k] for k in p} for r, p in zip(rows, plain)]) == json.dumps(plain)    # and the same values
    for (name, (ref, syn)), row in zip(pairs.items(), rows):
        (mr, fr, er), (ms, fs, es) = gpu_features(stft, ref, dev), gpu_features(stft, syn, dev)
        scales = {"f0_stats_ref": PR.m3_scale(PR.voiced(fr[:row["frames_ref"]])), "f0_stats_syn": PR.m3_scale(PR.voiced(fs[:row["frames_syn"]]))}
        compare_row(name, row, PR.score_pair(mr, ms, fr, fs, er, es), scales)
    same, up10, up30 = rows
    assert same["gpe"] == 0.0 and same["ffe"] == 0.0 and same["f0_dtw_hz"] == 0.0 and same["energy_mae"] == 0.0
    assert abs(same["f0_corr"] - 1.0) < 1e-9 and same["f0_stats_ref"] == same["f0_stats_syn"] and same["f0_stats_ref"]["n"] > 50
    assert up10["gpe"] < 0.1 and up30["gpe"] > 0.9
    # spectral-envelope cepstra: another path, the same tracks; the STFT then runs for the energy alone
    world = M.score_pairs(refs[:1], syns[:1], stft, S.FS, S.HOP, device=dev, cepstra="world", prosody=True)[0]
    assert world["cepstra"] == "world" and world["f0_stats_ref"] == same["f0_stats_ref"] and world["f0_dtw_hz"] == 0.0
    assert world["gpe"] == 0.0 and world["energy_mae"] == 0.0 and abs(world["f0_corr"] - 1.0) < 1e-9


def test_score_command_line_with_prosody(dev, tmp_path):
    """score.py --prosody in a subprocess on a three-utterance corpus: the keys land in the rows, and the corpus pitch moments of the
    summary equal the oracle's merge of the oracle's per-utterance moments of the GPU's own F0 tracks of the very files."""
    from scipy.io import wavfile
    root = str(tmp_path)
    cfg = config(root)
    pairs = PR.tone_pairs()
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
    out = os.path.join(root, "scores.jsonl")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "score.py"), "-p", os.path.join(root, "preprocess.yaml"), "-t",
                          os.path.join(root, "train.yaml"), "--source", os.path.join(root, "val.txt"), "--out", out, "--prosody"],
                         capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rows = [json.loads(line) for line in open(out)]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert [r["basename"] for r in rows] == list(pairs) and summary["utterances"] == 3
    assert all(key in r for r in rows for key in PR.SCORES + ("f0_dtw_path_len", "f0_stats_ref", "f0_stats_syn"))
    for side, folder in (("ref", os.path.join(root, "raw", "spk")), ("syn", os.path.join(root, "result"))):
        parts, tracks = [], []
        for name in pairs:
            w = torch.from_numpy(M.load_audio(os.path.join(folder, name + ".wav"), S.FS)).to(dev).unsqueeze(0)
            f0, _, frames = Pitch.dio_stonemask(w, [w.shape[1]], S.FS, S.FRAME_PERIOD)
            tracks.append(PR.voiced(f0[0, :min(int(frames[0]), w.shape[1] // S.HOP + 1)]))
            parts.append(PR.moments(tracks[-1]))
        mom = PR.merge_all(parts)
        sigma, skew, kurt = PR.shape(mom)
        print(side, "summary", {k: v for k, v in summary.items() if k.endswith(side)}, "oracle", mom[0], sigma, skew, kurt)
        assert summary["f0_voiced_frames_" + side] == mom[0]
        # sigma^2 = M2 / N is a sum of squares: RTOL.  gamma = (M3 / N) / sigma^3: M3 to RTOL of sum |d|^3, sigma^3 to 1.5 RTOL.
        # K + 3 = (M4 / N) / sigma^4: M4 to RTOL, sigma^4 to 2 RTOL.
        x = np.concatenate(tracks)
        abs3 = np.mean(np.abs(x - x.mean()) ** 3) / sigma ** 3
        assert close(summary["f0_std_hz_" + side], sigma)
        assert close(summary["f0_skew_" + side], skew, abs3 + 1.5 * abs(skew))
        assert close(summary["f0_kurt_" + side], kurt, 3.0 * (kurt + 3.0))
    want = PR.summarize(rows)                                                  # and the whole summary from the rows themselves
    for key, v in want.items():
        assert (math.isnan(v) and math.isnan(summary[key])) or summary[key] == pytest.approx(v, rel=1e-12), key
