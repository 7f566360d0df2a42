"""CPU: the numpy oracle of the spectral-envelope mel-cepstra (tests/world_ref.py) held against analytic answers: `freqt` against
the integral that defines it, the envelope against the known filter behind a pulse train, and the reason the feature exists, a
distortion that does not follow the pitch.  Also the host-side pieces of fastspeech2_amd/envelope.py that need no device."""
import json
import math

import numpy as np
import pytest

from fastspeech2_amd import envelope as E
from fastspeech2_amd import metrics as M
from tests import world_cases as C
from tests import world_ref as W

K = 24


def quadrature(order, a, n_pts, rule):
    """c~_0 = (1 / pi) int_0^pi L dw~, c~_m = (2 / pi) int_0^pi L cos(m w~) dw~ on n_pts equal steps of the WARPED axis, L = ln |H|
    evaluated from the poles at w = the inverse map of w~ (the all-pass map with -a).  rule "left": the rectangle rule, whose error
    is first order in the step, (step / 2) (g(0) - g(pi)) to leading order; "trapezoid": exact to rounding for this even, periodic,
    analytic integrand."""
    wt = np.pi * np.arange(n_pts + 1) / n_pts
    L = np.log(np.abs(C.response(order, W.warped(wt, -a))))
    wgt = np.ones(n_pts + 1)
    wgt[-1] = 0.0
    if rule == "trapezoid":
        wgt[0] = wgt[-1] = 0.5
    m = np.arange(K + 1)[:, None]
    out = (2.0 / n_pts) * np.sum(wgt[None, :] * L[None, :] * np.cos(m * wt[None, :]), axis=1)
    out[0] /= 2.0
    return out


@pytest.mark.parametrize("order", [2, 8])
@pytest.mark.parametrize("a", [0.455, 0.554])
def test_freqt_against_the_integral_that_defines_it(order, a):
    """The acceptance distance is measured: 4 x the distance between the rectangle rule at 2^16 and at 2^18 points (its own
    truncation error, which is what limits this comparison).  The trapezoid rule has no truncation error here, so against it the
    bar is rounding alone: the worst case n u max |L| of a sum of n = 2^16 terms, doubled for the cosine factors' own rounding,
    plus what the 4096-term input cepstrum leaves out (r^M / M per pole, r the largest pole radius)."""
    M_in = 4096
    c = C.exact_cepstrum(order, M_in)
    got = W.freqt(c, K, a)[0]
    q16, q18 = quadrature(order, a, 1 << 16, "left"), quadrature(order, a, 1 << 18, "left")
    bar = 4.0 * np.abs(q16 - q18).max()
    print("rectangle rule: oracle - q18", np.abs(got - q18).max(), "bar", bar)
    assert np.abs(got - q18).max() <= bar
    n = 1 << 16
    wt = np.pi * np.arange(n + 1) / n
    peak = np.abs(np.log(np.abs(C.response(order, W.warped(wt, -a))))).max()
    r = np.abs(C.poles(order)).max()
    tight = 2.0 * n * 2.0 ** -53 * peak + len(C.poles(order)) * r ** M_in / M_in
    trap = quadrature(order, a, n, "trapezoid")
    print("trapezoid rule: oracle - quadrature", np.abs(got - trap).max(), "bar", tight)
    assert np.abs(got - trap).max() <= tight


def test_freqt_without_warping_is_the_plain_cepstrum():
    c = C.exact_cepstrum(8, 513)
    assert np.array_equal(W.freqt(c, 40, 0.0)[0], c[:41])
    assert np.array_equal(E.freqt_table(1024, 40, 0.0), np.eye(513)[1:41])


def test_the_products_freqt_table_is_the_recursion():
    """table @ c against the recursion on c: a dot product of M + 1 rounded products, (M + 1) 2^-52 sum |t_q c_q| per element (twice
    the standard bound), once more for the rounding the table's own entries carry"""
    rng = np.random.RandomState(3)
    for n, Kc, a in ((1024, 24, 0.455), (2048, 40, 0.554), (256, 7, -0.3)):
        c = rng.randn(4, n // 2 + 1) * np.exp(-np.arange(n // 2 + 1) / 30.0)
        T = E.freqt_table(n, Kc, a)
        bound = 2.0 * (n // 2 + 1) * 2.0 ** -52 * (np.abs(c) @ np.abs(T).T)
        assert (np.abs(c @ T.T - W.freqt(c, Kc, a)[:, 1:]) <= bound).all()


def test_envelope_recovers_the_filter_behind_a_pulse_train():
    """a regression pin on the restatement (1.5 x the recorded RMS dB), not a quality claim"""
    rec = C.bars()["envelope_rms_db"]
    for f0 in C.PITCHES:
        got = C.envelope_error_db(f0)
        print(f0, "Hz: rms dB", got, "recorded", rec[str(int(f0))])
        assert got <= 1.5 * rec[str(int(f0))]
        assert got < 1.0                                                    # and the envelope is the filter, to under a dB


def test_the_distortion_does_not_follow_the_pitch():
    """the same filter at 120 and at 220 Hz: the spectral-envelope MCD is far below the mel-DCT's, which resolves the harmonics"""
    rec = C.bars()
    world, mel, F, P = C.pair_mcds()
    print("world", world, "mel", mel, "recorded", rec["mcd_world_db"], rec["mcd_mel_db"])
    assert world < mel
    assert (F, P) == (rec["pair_frames"], rec["pair_path_len"])
    assert abs(world - rec["mcd_world_db"]) <= 1e-9 * rec["mcd_world_db"] and abs(mel - rec["mcd_mel_db"]) <= 1e-9 * rec["mcd_mel_db"]


def test_the_two_transform_forms_of_the_oracle_agree():
    x = C.pulse_train(150.0, dur=0.05)
    f0 = np.array([150.0, 0.0])
    a, b = W.envelope(x, f0, C.FS, C.FRAME_PERIOD), W.envelope(x, f0, C.FS, C.FRAME_PERIOD, W.MatrixFft())
    assert np.abs(np.log(a) - np.log(b)).max() < 1e-8 and (a > 0).all()


def test_sizes_constants_and_refusals_need_no_device():
    assert [E.fft_size(fs) for fs in (16000, 22050, 24000, 44100, 48000)] == [1024, 1024, 1024, 2048, 2048]
    assert [W.fft_size(fs) for fs in (16000, 22050, 48000)] == [1024, 1024, 2048]
    assert E.ALPHA == {16000: 0.410, 22050: 0.455, 24000: 0.466, 44100: 0.544, 48000: 0.554}
    assert E.alpha_for(22050) == 0.455 and E.alpha_for(32000, 0.5) == 0.5
    with pytest.raises(ValueError, match="2048"):
        E.fft_size(96000)
    with pytest.raises(ValueError, match="--alpha"):
        E.alpha_for(32000)
    for bad in (0, 41):
        with pytest.raises(ValueError):
            E.check_mcep(bad)
    tw = E.twiddle_table(1024)
    assert tw.shape == (512, 2) and tw[0].tolist() == [1.0, -0.0] and abs(tw[256, 0]) < 1e-16 and tw[256, 1] == -1.0
    # the envelope buffers are part of a batch's cost: (N / 2 + 1) float64 per frame and side
    assert M.batch_bytes(3, 100, 80, 24, 256, 1024) - M.batch_bytes(3, 100, 80, 24, 256) == 3 * 180 * 513 * 8
    assert M.batch_bytes(3, 100, 80, 13, 256) == 3 * (100 * 80 * 9 + 180 * (256 * 40 + 13 * 8 + 64))


def test_score_cli_arguments_and_refusals_before_any_file_is_read():
    import score
    base = ["-p", "p.yaml", "-t", "t.yaml", "--source", "val.txt"]
    args = score.parse_args(base)
    assert (args.cepstra, args.alpha, args.n_mcep) == ("mel", None, None)
    args = score.parse_args(base + ["--cepstra", "world", "--alpha", "0.42", "--n_mcep", "30"])
    assert (args.cepstra, args.alpha, args.n_mcep) == ("world", 0.42, 30)
    cfg = {"preprocessing": {"audio": {"sampling_rate": 32000}, "stft": {"hop_length": 256}}}
    with pytest.raises(ValueError, match="--alpha"):
        M.run(cfg, "/nowhere", "/nowhere/val.txt", cepstra="world")
    cfg["preprocessing"]["audio"]["sampling_rate"] = 22050
    with pytest.raises(ValueError):
        M.run(cfg, "/nowhere", "/nowhere/val.txt", cepstra="world", n_mcep=41)
    with pytest.raises(ValueError):
        M.run(cfg, "/nowhere", "/nowhere/val.txt", cepstra="mel", alpha=0.4)


def test_the_recorded_bars_are_what_the_generator_writes():
    rec = C.bars()
    assert rec["factor"] == 16
    for case in ("22050", "48000"):
        assert rec["ln_envelope_bar"][case] == 16 * rec["ln_envelope_distance"][case] > 0
        for key, d in rec["mcep_distance"][case].items():
            assert rec["mcep_bar"][case][key] == 16 * d > 0
    assert math.isfinite(json.loads(json.dumps(rec))["mcd_world_db"])


def test_the_smoothing_is_the_difference_of_running_integrals_without_its_cancellation():
    """The specified short sum and the running-integral form WORLD uses are one quantity.  With u = 2^-53, L mirrored bins and w bins
    in the window: a sequential running integral S carries at most (L - 1) u S (the standard bound of a recursive sum), each of the
    two interpolations and the difference a few u S more, so that form is within 2 (L + 4) u S_total / wd of the truth; the short
    sum of w + 2 non-negative products is within 2 (w + 3) u of its own value.  That holds on a flat spectrum and on one spanning
    70 dB; on the second the first term is what the running-integral form loses, and the measured distance is printed."""
    n, fs, u = 1024, C.FS, 2.0 ** -53
    rng = np.random.RandomState(5)
    flat = 1.0 + 0.5 * rng.rand(n // 2 + 1)
    for g in (65.0, 180.0, 500.0, 2756.25):
        wd, df = 2.0 * g / 3.0, fs / n
        w, b = wd / df, int(wd * n / fs) + 1
        L = n // 2 + 2 * b + 1
        for name, P in (("flat", flat), ("70 dB", flat * 10.0 ** (-7.0 * np.arange(n // 2 + 1) / (n // 2)))):
            short, running = W.linear_smoothing(P, wd, fs, n), W.linear_smoothing_by_running_integral(P, wd, fs, n)
            total = (P.sum() + 2.0 * P[:b + 1].sum() + 2.0 * P[-b - 1:].sum()) * df          # at least the mirrored spectrum's integral
            bound = 2.0 * (L + 4) * u * total / wd + 2.0 * (w + 3.0) * u * short
            print(g, "Hz,", name, ": running-integral form against the short sum, relative", (np.abs(short - running) / short).max())
            assert (short > 0).all() and (np.abs(short - running) <= bound).all()
