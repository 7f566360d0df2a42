"""The modulation-spectrum postfilter without a GPU: the known answers of the specification (fastspeech2_amd/postfilter.py) through
the numpy restatement tests/postfilter_ref.py, so that the conditions the GPU tests rely on hold before a kernel runs; the host code
(the npz round trip, the config check, the refusals that need no device, the command lines) and the ABI.  The bars are those of
tests/golden/postfilter_bars.json: 16 times the distance between the fp64 and the longdouble restatement on the same input
(tests/golden/make_postfilter_bars.py)."""
import json
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib
from fastspeech2_amd import modspec as MS
from fastspeech2_amd import postfilter as PF
from tests import modspec_ref as mref
from tests import postfilter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "postfilter_bars.json")))


def bar(case, key="y"):
    return BARS["factor"] * BARS["distance"][case][key]


def closed_form_bar(case):
    """against a closed form: the bar, and what the closed form itself is off by (the tables and the input are rounded to fp64)"""
    return bar(case) + BARS["distance"][case]["to_expected"]


def _tables(tab, K=None, n=2):
    K = K or tab["mu_n"].shape[0]
    return PF.Tables(tab["mu_n"], tab["sd_n"], tab["mu_g"], tab["sd_g"], n, n, 0, 0, K, 22050, 256, 7)


def test_the_bars_belong_to_these_inputs():
    cases = lambda d: {k: {"seed": v[0], "K": v[1], "frames": list(v[2])} for k, v in d.items()}    # noqa: E731
    assert BARS["factor"] == 16 and BARS["stats_cases"] == cases(ref.STATS_CASES) and BARS["filter_cases"] == cases(ref.FILTER_CASES)
    assert BARS["filter_k"] == ref.FILTER_K
    assert BARS["known"] == [ref.KNOWN_SEED, ref.KNOWN_T, ref.KNOWN_COEF, list(ref.GAINS), list(ref.KNOWN_K), ref.CLAMP_BIN, ref.CLAMP_DB]
    assert set(BARS["distance"]) == set(ref.STATS_CASES) | set(ref.FILTER_CASES) | set(ref.known_cases())
    assert (ref.N, ref.FLOOR, ref.MIN_FRAMES, ref.MAX_FRAMES) == (PF.NFFT, PF.FLOOR, PF.MIN_FRAMES, PF.MAX_FRAMES)
    assert (ref.MAX_GAIN_DB, ref.K_DEFAULT) == (PF.MAX_GAIN_DB, PF.K_DEFAULT) == (20, 0.85)
    assert (PF.NFFT, PF.MAX_FRAMES, PF.MAX_COEF, PF.FLOOR, PF.MIN_FRAMES) == (MS.NFFT, MS.MAX_FRAMES, MS.MAX_COEF, MS.FLOOR, MS.MIN_FRAMES)
    # every length of interest at K = 1 and 13; the coefficient bound at T <= 257 only; the statistics cases mix the asked lengths
    assert set(ref.FILTER_CASES["f13"][2]) == set(ref.FILTER_CASES["f1"][2]) == set(ref.EVERY_T)
    assert ref.FILTER_CASES["f128"][1] == 128 and max(ref.FILTER_CASES["f128"][2]) <= 257 and ref.FILTER_CASES["f80"][1] == 80
    for name, (_, K, frames) in ref.STATS_CASES.items():
        assert set(frames) == {1, 31, 32, 33, 257, 2048} and K in (1, 13, 80)
        assert [len(s) for s in ref.STATS_SPLITS[name]] == [3, 4]
    # the closed forms hold far inside what a test allows them
    for name, d in BARS["distance"].items():
        if "to_expected" in d:
            assert d["to_expected"] <= 1e-14 and d["y"] <= 1e-14, name


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("k", ref.KNOWN_K)
def test_equal_statistics_leave_the_trajectory_alone(k):
    c, tab, kk, expected = ref.known_cases()[f"equal_k{k}"]
    assert kk == k and np.abs(ref.apply(c, tab, k) - expected).max() <= closed_form_bar(f"equal_k{k}")
    assert np.abs(ref.gains(ref.logms(c), tab, k) - 1).max() <= 1e-14


@pytest.mark.parametrize("k", ref.KNOWN_K)
@pytest.mark.parametrize("a", ref.GAINS)
def test_a_shift_of_the_mean_by_2_ln_a_is_a_gain_of_a_to_the_k(a, k):
    name = f"gain{a}_k{k}"
    c, tab, _, expected = ref.known_cases()[name]
    y = ref.apply(c, tab, k)
    assert np.abs(y - expected).max() <= closed_form_bar(name)
    assert np.abs(y - c).max() > 0.1                                        # and it is a gain: the trajectory did move
    assert np.allclose(y.mean(axis=0), c.mean(axis=0), atol=1e-13)          # the mean is untouched


def test_a_constant_comes_back_unchanged():
    c, tab, k, expected = ref.known_cases()["constant"]
    assert np.abs(ref.apply(c, tab, k) - expected).max() <= closed_form_bar("constant")


def test_the_clamp_gives_exactly_20_db():
    c, tab, k, expected = ref.known_cases()["clamp"]
    g = ref.gains(ref.logms(c), tab, k)
    assert abs(g[0, ref.CLAMP_BIN] - 10.0) <= 1e-14 and np.abs(np.delete(g[0], ref.CLAMP_BIN) - 1).max() <= 1e-14
    tab60 = dict(tab)
    assert abs(20 * np.log10(np.exp(0.5 * (tab60["mu_n"] - tab60["mu_g"])[0, ref.CLAMP_BIN])) - 60) <= 1e-12      # unclamped: 60 dB
    assert ref.clamp_factor() == 3.25
    assert np.abs(ref.apply(c, tab, k) - expected).max() <= closed_form_bar("clamp")


def test_pass_through_rows_and_k_0():
    rows, tab = ref.filter_input("f1")
    for c in rows:
        y = ref.apply(c, tab, 1.0)
        assert (y.tobytes() == c.tobytes()) == (len(c) < ref.MIN_FRAMES)
        assert ref.apply(c, tab, 0).tobytes() == c.tobytes()
    assert PF.pass_through([1, 31, 32, 2048, 2049]) == 3
    with pytest.raises(ValueError):
        PF.pass_through([0])


def test_the_longdouble_restatement_agrees_with_the_fft():
    rows, tab = ref.filter_input("f13")
    c = rows[0][:, :2]
    tab = {n: v[:2] for n, v in tab.items()}
    a, b = ref.apply(c, tab, 0.85), ref.apply(c, tab, 0.85, np.longdouble)
    assert b.dtype == np.longdouble and np.abs(a - b).max() < 1e-13 and np.abs(a - c).max() > 1e-3
    s = ref.stats_input("s13")
    few = [r[:, :2] for r in s if len(r) <= 257]
    u, v = ref.statistics(few), ref.statistics(few, np.longdouble)
    assert u[2:] == v[2:] == (5, 3) and np.abs(u[0] - v[0]).max() < 1e-9 and np.abs(u[1] - v[1]).max() < 1e-9


def test_the_corpus_satisfies_both_inequalities_on_the_restatement_alone():
    """known answer 4: AR(1) rows against their 5-tap moving average; statistics trained on them, the generated rows filtered at
    k = 1: every band above 4 Hz lies strictly closer to the natural one, and so does the global variance"""
    natural, generated = ref.corpus()
    assert len(natural) >= 24 and all(200 <= len(c) <= 600 and c.shape[1] == 4 for c in natural)
    tab = ref.tables(natural, generated)
    filtered = [ref.apply(c, tab, 1.0) for c in generated]
    bins, hz = mref.band_bins(*ref.RATE)
    assert (bins, hz) == MS.band_bins(*ref.RATE)
    before, gv_before = ref.corpus_summary(natural, generated, bins)
    after, gv_after = ref.corpus_summary(natural, filtered, bins)
    high = [j for j, (lo, _) in enumerate(hz) if lo >= 4]
    assert len(high) == 4
    print(before.tolist(), after.tolist(), gv_before, gv_after)
    for j in high:
        assert abs(after[j]) < abs(before[j]), j
    assert abs(gv_after) < abs(gv_before) and gv_before < 0


# ------------------------------------------------------------------------------------------------ host code
def test_npz_round_trip_and_the_config_check(tmp_path):
    from tests.test_align_cpu import config
    _, tab = ref.filter_input("f13")
    t = PF.Tables(tab["mu_n"], tab["sd_n"], tab["mu_g"], tab["sd_g"], 6, 5, 1, 2, 13, 22050, 256, restore_step=900000)
    path = os.path.join(str(tmp_path), "stats.npz")
    t.save(path)
    with np.load(path) as z:
        assert set(z.files) == {"mu_n", "sd_n", "mu_g", "sd_g", "n_natural", "n_generated", "left_out_natural", "left_out_generated", "n_mel",
                                "sampling_rate", "hop_length", "nfft", "floor", "restore_step"}
        assert int(z["nfft"]) == 4096 and float(z["floor"]) == 1e-12 and z["mu_n"].shape == (13, 2049) and z["mu_n"].dtype == np.float64
    back = PF.load(path)
    for name in ("mu_n", "sd_n", "mu_g", "sd_g"):
        assert getattr(back, name).tobytes() == tab[name].tobytes()
    assert (back.n_natural, back.n_generated, back.left_out_natural, back.left_out_generated) == (6, 5, 1, 2)
    assert (back.n_mel, back.sampling_rate, back.hop_length, back.restore_step) == (13, 22050, 256, 900000)
    cfg = config("/nowhere")
    cfg["preprocessing"]["mel"]["n_mel_channels"] = 13
    assert cfg["preprocessing"]["audio"]["sampling_rate"] == 22050 and cfg["preprocessing"]["stft"]["hop_length"] == 256
    PF.load(path, cfg)
    for section, key, value in (("mel", "n_mel_channels", 80), ("audio", "sampling_rate", 16000), ("stft", "hop_length", 200)):
        bad = json.loads(json.dumps(cfg))
        bad["preprocessing"][section][key] = value
        with pytest.raises(ValueError, match="preprocess config"):
            PF.load(path, bad)
    with open(path, "wb") as f:                                              # another transform length: not this module's file
        np.savez(f, **{**{n: getattr(t, n) for n in ("mu_n", "sd_n", "mu_g", "sd_g")}, "n_natural": 6, "n_generated": 5, "left_out_natural": 0,
                       "left_out_generated": 0, "n_mel": 13, "sampling_rate": 22050, "hop_length": 256, "nfft": 2048, "floor": 1e-12,
                       "restore_step": 1})
    with pytest.raises(ValueError, match="4096"):
        PF.load(path)


def test_refusals_that_need_no_device():
    _, tab = ref.filter_input("f13")
    with pytest.raises(ValueError, match="at least 2"):                     # fewer than 2 utterances on a side
        PF.Tables(tab["mu_n"], tab["sd_n"], tab["mu_g"], tab["sd_g"], 2, 1, 0, 0, 13, 22050, 256)
    with pytest.raises(ValueError, match="at least 2"):
        PF.Stats(13, 22050, 256).finalize()
    with pytest.raises(ValueError, match="at least 2"):
        ref.statistics(ref.stats_input("s1")[1:3])                          # 2048 frames and 1 frame: one utterance is kept
    with pytest.raises(ValueError):
        PF.Tables(tab["mu_n"][:, :2048], tab["sd_n"], tab["mu_g"], tab["sd_g"], 2, 2, 0, 0, 13, 22050, 256)
    with pytest.raises(ValueError):
        PF.Stats(129, 22050, 256)
    t = _tables(tab)
    mel = torch.zeros(2, 40, 13)
    for k in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="emphasis"):
            PF.apply(mel, [40, 40], t, k)
    with pytest.raises(ValueError, match="no CPU fallback"):
        PF.apply(mel, [40, 40], t)
    with pytest.raises(ValueError, match="no CPU fallback"):
        PF.Stats(13, 22050, 256).add_natural(mel, [40, 40])
    with pytest.raises(ValueError, match="frame"):
        PF.apply(mel, [0, 40], t)
    with pytest.raises(ValueError, match="Tables"):
        PF.apply(mel, [40, 40], tab)


def test_the_command_lines_parse():
    import postfilter as cli
    import synthesize
    a = cli.parse_args(["train", "-p", "p.yaml", "-m", "m.yaml", "-t", "t.yaml", "--restore_step", "9", "out.npz"])
    assert (a.command, a.source, a.batch_size, a.max_utts, a.restore_step, a.out) == ("train", None, 8, 0, 9, "out.npz")
    with pytest.raises(SystemExit):
        cli.parse_args(["train", "-p", "p.yaml", "-m", "m.yaml", "-t", "t.yaml", "out.npz"])       # no --restore_step
    base = ["--restore_step", "1", "--mode", "batch", "--source", "v.txt", "-p", "p", "-m", "m", "-t", "t"]
    s = synthesize.parse_args(base)
    assert s.postfilter is None and s.postfilter_k == 0.85
    s = synthesize.parse_args(base + ["--postfilter", "s.npz", "--postfilter_k", "0.5", "--griffin_iters", "3"])
    assert (s.postfilter, s.postfilter_k, s.griffin_iters) == ("s.npz", 0.5, 3)
    with pytest.raises(SystemExit):
        synthesize.parse_args(base + ["--postfilter_k", "1.5"])


def test_the_new_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    assert len(protos["fs2_ms_stats_update"][1]) == 10 and len(protos["fs2_ms_filter"][1]) == 25
    lib = _lib.load()
    assert hasattr(lib, "fs2_ms_stats_update") and hasattr(lib, "fs2_ms_filter")
    # argument checks return before any launch, without a device
    with pytest.raises(ValueError, match="coefficients"):
        _lib.call("fs2_ms_filter", None, 80, 80, None, None, 80, 1, None, None, None, None, None, 2049, 0.85, 1e-12, 20.0, 32, None, 80, 80, 0, 1, 1,
                  129, None)
    with pytest.raises(ValueError, match="emphasis"):
        _lib.call("fs2_ms_filter", None, 80, 80, None, None, 80, 1, None, None, None, None, None, 2049, 1.5, 1e-12, 20.0, 32, None, 80, 80, 0, 1, 1,
                  80, None)
    with pytest.raises(ValueError, match="null"):
        _lib.call("fs2_ms_filter", None, 80, 80, None, None, 80, 1, None, None, None, None, None, 2049, 0.85, 1e-12, 20.0, 32, None, 80, 80, 0, 1, 1,
                  80, None)
    with pytest.raises(ValueError, match="strides"):
        _lib.call("fs2_ms_stats_update", None, 2049, 2049, None, None, 4098, 0, 1, 2, None)
