"""Prosody scores without a GPU: the numpy oracle tests/prosody_ref.py against independent forms (extended-precision moments of the
concatenated data, numpy's correlation, hand-made tracks), the host pieces of fastspeech2_amd.metrics (scores from the sums, the
merge of the moments, the summary, the refusals), score.py's `--prosody` through its `score_fn` seam, and the known answers of the
GPU end-to-end test on the CPU chain (oracle mel, tests/f0_ref.py, tests/dtw_ref.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import metrics as M
from tests import dtw_ref as R
from tests import prosody_ref as PR
from tests.test_metrics_cpu import HOP, corpus  # noqa: F401  (the fixture)

NAN = float("nan")


def same(a, b, rel=1e-12):
    """two summaries / rows: the same keys, NaN where the other has NaN, numbers within `rel`, everything else equal"""
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k], rel)
        elif isinstance(a[k], float) and isinstance(b[k], float):
            assert (math.isnan(a[k]) and math.isnan(b[k])) or a[k] == pytest.approx(b[k], rel=rel, abs=0.0), (k, a[k], b[k])
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    return True


def direct_moments(u):
    """(n, mean, M2, M3, M4) in numpy's extended precision, straight from the definitions"""
    x = np.asarray(u, np.longdouble)
    n = len(x)
    mean = x.sum() / n
    d = x - mean
    return n, float(mean), float((d ** 2).sum()), float((d ** 3).sum()), float((d ** 4).sum())


def utterances(rng, sizes):
    return [np.round(rng.gamma(6.0, 30.0, n) + 60.0, 3) for n in sizes]       # skewed, like F0 in Hz


def test_oracle_moments_against_extended_precision():
    rng = np.random.RandomState(0)
    for u in utterances(rng, (1, 2, 3, 64, 257, 2048)):
        got, want = PR.moments(u), direct_moments(u)
        assert got[0] == want[0] and got[1] == pytest.approx(want[1], rel=1e-14)
        assert got[2] == pytest.approx(want[2], rel=1e-12, abs=0.0) and got[4] == pytest.approx(want[4], rel=1e-12, abs=0.0)
        assert abs(got[3] - want[3]) <= 1e-12 * PR.m3_scale(u)
    assert PR.moments([]) == (0, 0.0, 0.0, 0.0, 0.0)
    assert PR.moments([123.0]) == (1, 123.0, 0.0, 0.0, 0.0)
    assert np.array_equal(PR.voiced([0.0, 100.0, 0.0, 50.0, -1.0]), [100.0, 50.0])


@pytest.mark.parametrize("sizes", [(40,), (40, 77), (40, 0, 77, 1, 300, 2, 13)])
def test_merge_of_utterances_against_the_concatenation(sizes):
    rng = np.random.RandomState(len(sizes))
    parts = utterances(rng, sizes)
    want = direct_moments(np.concatenate(parts))
    scale = PR.m3_scale(np.concatenate(parts))
    for merge_all in (PR.merge_all, lambda ps: __import__("functools").reduce(M.merge_moments, ps, (0, 0.0, 0.0, 0.0, 0.0))):
        got = merge_all([PR.moments(u) for u in parts])
        assert got[0] == want[0] and got[1] == pytest.approx(want[1], rel=1e-13)
        assert got[2] == pytest.approx(want[2], rel=1e-11) and got[4] == pytest.approx(want[4], rel=1e-11)
        assert abs(got[3] - want[3]) <= 1e-11 * scale
    # the corpus figures against numpy's own population moments of the concatenation
    x = np.concatenate(parts)
    d = x - x.mean()
    sigma = math.sqrt((d ** 2).mean())
    N, got_sigma, skew, kurt = M.corpus_moments([PR.stats_dict(PR.moments(u)) for u in parts])
    assert N == len(x) and got_sigma == pytest.approx(sigma, rel=1e-11)
    assert skew == pytest.approx((d ** 3).mean() / sigma ** 3, rel=1e-9) and kurt == pytest.approx((d ** 4).mean() / sigma ** 4 - 3.0, rel=1e-9)
    assert PR.shape(PR.merge_all([PR.moments(u) for u in parts])) == pytest.approx((got_sigma, skew, kurt), rel=1e-12)


def test_corpus_moments_without_voiced_frames_or_spread():
    N, sigma, skew, kurt = M.corpus_moments([PR.stats_dict(PR.moments([]))] * 2)
    assert N == 0 and math.isnan(sigma) and math.isnan(skew) and math.isnan(kurt)
    N, sigma, skew, kurt = M.corpus_moments([PR.stats_dict(PR.moments([200.0, 200.0])), PR.stats_dict(PR.moments([200.0]))])
    assert N == 3 and sigma == 0.0 and math.isnan(skew) and math.isnan(kurt)
    assert all(math.isnan(v) for v in PR.shape((0, 0.0, 0.0, 0.0, 0.0)))
    # a normal sample: skewness and EXCESS kurtosis near 0
    x = np.random.RandomState(5).randn(200000) * 30 + 200
    _, sigma, skew, kurt = M.corpus_moments([PR.stats_dict(PR.moments(x[:70000])), PR.stats_dict(PR.moments(x[70000:]))])
    assert sigma == pytest.approx(30.0, rel=0.01) and abs(skew) < 0.03 and abs(kurt) < 0.06


def test_correlation_against_numpy():
    rng = np.random.RandomState(1)
    T = 400
    r = np.where(rng.rand(T) < 0.7, 120.0 * 2.0 ** rng.uniform(-0.5, 1.0, T), 0.0)
    s = np.where(rng.rand(T) < 0.7, r * 2.0 ** (0.2 * rng.randn(T)) + (r == 0) * 150.0, 0.0)
    e = rng.rand(T).astype(np.float32)
    idx = np.arange(T)
    q = PR.path_sums(idx, idx, r, s, e, e)
    both = (r > 0) & (s > 0)
    assert q["n"] == both.sum() > 100
    want = np.corrcoef(np.log(r[both]), np.log(s[both]))[0, 1]
    assert PR.path_scores(q, T)["f0_corr"] == pytest.approx(want, rel=1e-12)
    got = M.prosody_scores([q[k] for k in ("gross", "n", "mism", "sxx", "syy", "sxy", "de", "se")], T, PR.moments(PR.voiced(r)),
                           PR.moments(PR.voiced(s)), 0.0, 0)
    assert got["f0_corr"] == pytest.approx(want, rel=1e-12)
    # a constant track, one both-voiced cell: no correlation
    for rr, ss in ((np.full(9, 200.0), 100.0 + np.arange(9.0)), (np.array([100.0, 0.0]), np.array([90.0, 80.0]))):
        k = np.arange(len(rr))
        z = np.zeros(len(rr), np.float32)
        assert math.isnan(PR.path_scores(PR.path_sums(k, k, rr, ss, z, z), len(rr))["f0_corr"])


def test_gross_pitch_error_on_hand_made_tracks():
    z = np.zeros(8, np.float32)
    ref = np.array([100.0, 100.0, 100.0, 100.0, 100.0, 0.0, 100.0, 0.0])
    syn = np.array([120.0, 80.0, 121.0, 79.0, 100.0, 50.0, 0.0, 0.0])
    k = np.arange(8)
    q = PR.path_sums(k, k, ref, syn, z, z)
    # 120 and 80 are exactly on the 20 % boundary and do not count; 121 and 79 do; two V/UV mismatches; one cell unvoiced on both
    assert (q["gross"], q["n"], q["mism"]) == (2, 5, 2)
    row = PR.path_scores(q, 8)
    assert row["gpe"] == 2 / 5 and row["ffe"] == 4 / 8
    assert math.isnan(row["energy_mae_rel"]) and row["energy_mae"] == 0.0
    for r, s, want in ((100.0, 120.0, 0), (100.0, 80.0, 0), (100.0, 121.0, 1), (5.0, 6.0, 0), (5.0, 4.0, 0), (35.0, 42.0, 0),
                       (35.0, 28.0, 0), (35.0, 42.00000000000001, 1)):
        assert PR.path_sums([0], [0], [r], [s], z, z)["gross"] == want, (r, s)
    # nothing voiced on both sides at once
    q = PR.path_sums(np.arange(4), np.arange(4), [0.0, 0.0, 100.0, 0.0], [0.0, 90.0, 0.0, 0.0], z, z)
    row = PR.path_scores(q, 4)
    assert q["n"] == 0 and math.isnan(row["gpe"]) and math.isnan(row["f0_corr"]) and row["ffe"] == 0.5
    got = M.prosody_scores([0, 0, 2, 0.0, 0.0, 0.0, 0.0, 0.0], 4, (1, 100.0, 0, 0, 0), (1, 90.0, 0, 0, 0), NAN, 0)
    assert math.isnan(got["gpe"]) and math.isnan(got["f0_corr"]) and got["ffe"] == 0.5 and math.isnan(got["f0_dtw_hz"])
    assert got["f0_dtw_path_len"] == 0 and got["f0_stats_ref"] == {"n": 1, "mean": 100.0, "m2": 0.0, "m3": 0.0, "m4": 0.0}
    # a path that repeats cells: energy over the cells, not the frames
    e_ref, e_syn = np.array([1.0, 3.0], np.float32), np.array([2.0, 2.0, 7.0], np.float32)
    q = PR.path_sums([0, 0, 1], [0, 1, 2], [100.0, 0.0], [100.0, 100.0, 0.0], e_ref, e_syn)
    row = PR.path_scores(q, 3)
    assert row["energy_mae"] == (1 + 1 + 4) / 3 and row["energy_mae_rel"] == 6 / 5


def test_contour_dtw_of_a_contour_against_itself_with_repeats():
    rng = np.random.RandomState(3)
    u = 100.0 + 10.0 * np.arange(19) + rng.randint(0, 5, 19)                   # no two values alike
    idx = np.repeat(np.arange(19), rng.randint(1, 5, 19))
    total, pi, pj = PR.contour_dtw(u, u[idx])
    assert total == 0.0 and np.array_equal(pi, idx) and np.array_equal(pj, np.arange(len(idx)))
    total, pi, pj = PR.contour_dtw(u, u + 2.0)                                 # |u - w| = 2 on the diagonal, at least 4 off it
    assert total == 2.0 * 19 and np.array_equal(pi, np.arange(19)) and np.array_equal(pj, np.arange(19))
    total, pi, pj = PR.contour_dtw(u, [])
    assert math.isnan(total) and len(pi) == 0
    f0 = np.concatenate([[0.0], u, [0.0, 0.0]])
    row = PR.prosody(np.arange(22), np.arange(22), f0, f0, np.ones(22, np.float32), np.ones(22, np.float32))
    assert row["f0_dtw_hz"] == 0.0 and row["f0_dtw_path_len"] == 19 and row["gpe"] == 0.0 and row["f0_corr"] == pytest.approx(1.0, abs=1e-12)


def prosody_rows():
    st = lambda u: PR.stats_dict(PR.moments(u))                                # noqa: E731
    rng = np.random.RandomState(4)
    a, b, c = utterances(rng, (50, 80, 1))
    base = [{"mcd_db": 4.0, "path_len": 100, "vuv_error": 0.1, "f0_rmse_cents": 50.0, "n_voiced_pairs": 60},
            {"mcd_db": 6.0, "path_len": 300, "vuv_error": 0.3, "f0_rmse_cents": NAN, "n_voiced_pairs": 0},
            {"mcd_db": 5.0, "path_len": 200, "vuv_error": 0.2, "f0_rmse_cents": 150.0, "n_voiced_pairs": 20}]
    extra = [{"gpe": 0.25, "ffe": 0.2, "f0_corr": 0.9, "f0_dtw_hz": 12.0, "f0_dtw_path_len": 70, "energy_mae": 1.5, "energy_mae_rel": 0.1,
              "f0_stats_ref": st(a), "f0_stats_syn": st(a * 1.1)},
             {"gpe": NAN, "ffe": 0.3, "f0_corr": NAN, "f0_dtw_hz": NAN, "f0_dtw_path_len": 0, "energy_mae": 2.5, "energy_mae_rel": NAN,
              "f0_stats_ref": st(b), "f0_stats_syn": st([])},
             {"gpe": 0.5, "ffe": 0.4, "f0_corr": NAN, "f0_dtw_hz": 30.0, "f0_dtw_path_len": 30, "energy_mae": 0.5, "energy_mae_rel": 0.3,
              "f0_stats_ref": st(c), "f0_stats_syn": st(b + 5.0)}]
    return base, [dict(x, **y) for x, y in zip(base, extra)], (a, b, c)


def test_summary_with_and_without_the_prosody_keys():
    base, rows, (a, b, c) = prosody_rows()
    plain = M.summarize(base)
    assert same(plain, R.summarize(base)) and not any("gpe" in k or "f0_std" in k for k in plain)     # today's summary, exactly
    got = M.summarize(rows)
    assert same(got, PR.summarize(rows))
    assert {k: v for k, v in got.items() if k in plain}.keys() == plain.keys() and same({k: got[k] for k in plain}, plain)
    assert got["gpe_mean"] == 0.375 and got["gpe_weighted"] == pytest.approx((0.25 * 60 + 0.5 * 20) / 80) and got["gpe_nan_utterances"] == 1
    assert got["ffe_weighted"] == pytest.approx((0.2 * 100 + 0.3 * 300 + 0.4 * 200) / 600) and got["ffe_nan_utterances"] == 0
    assert got["f0_corr_mean"] == 0.9 and got["f0_corr_nan_utterances"] == 2
    assert got["f0_dtw_hz_weighted"] == pytest.approx((12.0 * 70 + 30.0 * 30) / 100) and got["f0_dtw_hz_nan_utterances"] == 1
    assert got["energy_mae_weighted"] == pytest.approx((1.5 * 100 + 2.5 * 300 + 0.5 * 200) / 600)
    ref = np.concatenate([a, b, c])
    assert got["f0_voiced_frames_ref"] == 131 and got["f0_std_hz_ref"] == pytest.approx(ref.std(), rel=1e-11)
    d = ref - ref.mean()
    assert got["f0_skew_ref"] == pytest.approx((d ** 3).mean() / ref.std() ** 3, rel=1e-9)
    assert got["f0_kurt_ref"] == pytest.approx((d ** 4).mean() / ref.std() ** 4 - 3.0, rel=1e-9)
    assert got["f0_std_hz_syn"] == pytest.approx(np.concatenate([a * 1.1, b + 5.0]).std(), rel=1e-11)
    nothing = [dict(r, gpe=NAN, f0_corr=NAN, f0_dtw_hz=NAN, f0_stats_ref=PR.stats_dict(PR.moments([]))) for r in rows]
    got = M.summarize(nothing)
    assert same(got, PR.summarize(nothing)) and math.isnan(got["gpe_mean"]) and math.isnan(got["f0_std_hz_ref"]) and got["gpe_nan_utterances"] == 3


def test_batch_bytes_adds_nothing_when_off():
    for args in ((7, 300, 280), (1, 2048, 2048, 24, 256, 1024)):
        assert M.batch_bytes(*args) == M.batch_bytes(*args, prosody=False)
        assert M.batch_bytes(*args, prosody=True) == M.batch_bytes(*args) + args[0] * (args[1] + args[2]) * 24
    assert M.batch_bytes(3, 100, 90) == 3 * (100 * 90 * 9 + 190 * (256 * 40 + 13 * 8 + 64))              # the figure before this switch


def test_refusals_before_any_launch():
    f = torch.zeros(2, 8, dtype=torch.float64)
    with pytest.raises(ValueError, match="on the GPU"):
        M.voiced_contours(f, [8, 8])
    with pytest.raises(ValueError, match="2049 frames"):
        M.voiced_contours(torch.zeros(1, 2049, dtype=torch.float64), [2049])
    p = torch.zeros(2, 15, dtype=torch.int32)
    with pytest.raises(ValueError, match="on the GPU"):
        M.prosody_on_path(p, p, torch.zeros(2, dtype=torch.int32), f, [8, 8], f, [8, 8], f.float(), f.float())
    with pytest.raises(ValueError, match="2049 frames"):
        M.prosody_on_path(p, p, torch.zeros(2, dtype=torch.int32), f, [2049, 8], f, [8, 8], f.float(), f.float())
    with pytest.raises(ValueError, match="on the GPU"):
        M.contour_dtw(f, [8, 8], f, [8, 8])
    with pytest.raises(ValueError, match="2049 frames"):
        M.contour_dtw(f, [2049, 8], f, [8, 8])

    class Stft:
        hop_length, filter_length, n_mel_channels = 256, 1024, 80
    ok = np.zeros(4000, np.float32)
    with pytest.raises(ValueError, match="f0=False"):
        M.score_pairs([ok], [ok], Stft, 22050, 256, f0=False, prosody=True)
    with pytest.raises(ValueError, match="stft=None"):
        M.score_pairs([ok], [ok], None, 22050, 256, cepstra="world", prosody=True)
    with pytest.raises(ValueError, match="too short"):                         # the energy needs the STFT with world cepstra too
        M.score_pairs([ok], [ok[:512]], Stft, 22050, 256, cepstra="world", prosody=True)


def test_the_abi_refuses_bad_arguments_before_launch():
    from fastspeech2_amd import _lib
    one = torch.zeros(16, dtype=torch.float64)                                 # never dereferenced: the arguments are refused first
    p = one.data_ptr()
    with pytest.raises(ValueError, match="supported maximum"):
        _lib.call("fs2_prosody_voiced", p, 2049, p, p + 8, 2049, p, p, 5, 1, 2049, None)
    with pytest.raises(ValueError, match="strides"):
        _lib.call("fs2_prosody_voiced", p, -8, p, p + 8, 8, p, p, 5, 1, 8, None)                  # negative stride
    with pytest.raises(ValueError, match="strides"):
        _lib.call("fs2_prosody_voiced", p, 8, p, p + 8, 8, p, p, 4, 1, 8, None)                   # statistics row too short
    with pytest.raises(ValueError, match="null"):
        _lib.call("fs2_prosody_voiced", p, 8, p, None, 8, p, p, 5, 1, 8, None)
    with pytest.raises(ValueError, match="in place"):
        _lib.call("fs2_prosody_voiced", p, 8, p, p, 8, p, p, 5, 1, 8, None)
    with pytest.raises(ValueError, match="supported maximum"):
        _lib.call("fs2_dtw_prosody", p, p, 5000, p, p, 2049, p, 8, p, 2049, p, 8, p, p, p, 8, 1, 2049, 8, None)
    with pytest.raises(ValueError, match="strides"):
        _lib.call("fs2_dtw_prosody", p, p, 15, p, p, 8, p, 8, p, 8, p, -8, p, p, p, 8, 1, 8, 8, None)      # negative stride
    with pytest.raises(ValueError, match="strides"):
        _lib.call("fs2_dtw_prosody", p, p, 15, p, p, 8, p, 8, p, 8, p, 8, p, p, p, 7, 1, 8, 8, None)       # sums row too short
    with pytest.raises(ValueError, match="null"):
        _lib.call("fs2_dtw_prosody", p, p, 15, p, p, 8, p, 8, None, 8, p, 8, p, p, p, 8, 1, 8, 8, None)


# ------------------------------------------------------------------------------------------------ score.py through score_fn
def fake_scores(seen):
    st = PR.stats_dict(PR.moments([100.0, 200.0, 300.0]))

    def fn(refs, syns, **kw):
        seen.append(kw)
        rows = [{"mcd_db": 1.0, "path_len": len(s), "frames_ref": len(r) // HOP + 1, "frames_syn": len(s) // HOP + 1, "vuv_error": 0.0,
                 "f0_rmse_cents": 10.0, "n_voiced_pairs": 5} for r, s in zip(refs, syns)]
        if kw.get("prosody"):
            for k, row in enumerate(rows):
                row.update({"gpe": 0.1 * (k + 1), "ffe": 0.2, "f0_corr": NAN if k else 0.5, "f0_dtw_hz": 3.0, "f0_dtw_path_len": 9,
                            "energy_mae": 1.0, "energy_mae_rel": 0.5, "f0_stats_ref": st, "f0_stats_syn": st})
        return rows
    return fn


def run_cli(root, extra, seen):
    import score
    out = os.path.join(root, "scores.jsonl")
    argv = ["-p", os.path.join(root, "preprocess.yaml"), "-t", os.path.join(root, "train.yaml"), "--source",
            os.path.join(root, "val.txt"), "--out", out] + extra
    rows, skipped, summary = score.main(argv, score_fn=fake_scores(seen))
    with open(out) as f:
        written = [json.loads(line) for line in f]
    return rows, written, summary


def test_cli_prosody_switch(corpus, capsys):  # noqa: F811
    seen = []
    with pytest.raises(SystemExit, match="--no_f0"):
        run_cli(corpus, ["--prosody", "--no_f0"], seen)
    assert seen == [] and not os.path.exists(os.path.join(corpus, "scores.jsonl"))       # refused before any work
    rows, written, summary = run_cli(corpus, [], seen)
    assert seen == [{}] and "gpe" not in written[0] and not any(k.startswith(("gpe", "f0_std")) for k in summary)
    capsys.readouterr()
    rows, written, summary = run_cli(corpus, ["--prosody"], seen)
    assert seen[-1] == {"prosody": True}
    assert len(written) == 2 and all(same(w, r) for w, r in zip(written, rows))
    for key in ("gpe", "ffe", "f0_corr", "f0_dtw_hz", "f0_dtw_path_len", "energy_mae", "energy_mae_rel", "f0_stats_ref", "f0_stats_syn"):
        assert key in written[0], key
    assert written[1]["gpe"] == 0.2 and math.isnan(written[1]["f0_corr"]) and written[0]["f0_stats_ref"]["n"] == 3
    assert summary["gpe_mean"] == pytest.approx(0.15) and summary["f0_corr_nan_utterances"] == 1
    assert summary["f0_voiced_frames_ref"] == 6 and summary["f0_std_hz_syn"] == pytest.approx(np.std([100.0, 200.0, 300.0] * 2))
    assert same(json.loads(capsys.readouterr().out.strip().splitlines()[-1]), summary)


# ------------------------------------------------------------------------------------------------ the known answers, on the CPU chain
def test_the_cpu_chain_meets_the_known_answers_of_the_end_to_end_test():
    """The conditions tests/test_prosody_gpu.py sets for its three pairs (identical, every tone at 1.10 and at 1.30 times the
    frequency) are conditions, not measurements: the whole chain in numpy (the oracle's STFT mel and energy, tests/f0_ref.py for
    DIO + StoneMask, tests/dtw_ref.py for the path) has to meet them on these signals."""
    pairs = PR.tone_pairs()
    feats = {}

    def features(w):
        key = w.tobytes()
        if key not in feats:
            feats[key] = PR.chain_features(w)
        return feats[key]
    rows = {}
    for name, (ref, syn) in pairs.items():
        (mr, fr, er), (ms, fs, es) = features(ref), features(syn)
        rows[name] = PR.score_pair(mr, ms, fr, fs, er, es)
        print(name, {k: rows[name][k] for k in PR.SCORES + ("n_voiced_pairs", "path_len", "f0_dtw_path_len")})
    assert list(rows) == ["same"] + ["x%.2f" % f for f in PR.FACTORS]
    same_row = rows["same"]
    assert same_row["gpe"] == 0.0 and same_row["ffe"] == 0.0 and same_row["f0_dtw_hz"] == 0.0 and same_row["energy_mae"] == 0.0
    assert abs(same_row["f0_corr"] - 1.0) < 1e-9 and same_row["f0_stats_ref"] == same_row["f0_stats_syn"]
    assert same_row["n_voiced_pairs"] > 50
    assert rows["x1.10"]["gpe"] < 0.1 and rows["x1.10"]["n_voiced_pairs"] > 50
    assert rows["x1.30"]["gpe"] > 0.9 and rows["x1.30"]["n_voiced_pairs"] > 50
