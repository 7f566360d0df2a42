"""pYIN specification (fastspeech2_amd/pyin.py) without a GPU: the numpy oracle tests/pyin_ref.py on the known-answer signals against
the recorded bars, the host-side constants, and the surfaces that take the new estimator (Preprocessor, preprocess.py --pitch,
score.py --f0, the ABI header)."""
import numpy as np
import pytest

from fastspeech2_amd import _lib
from fastspeech2_amd import preprocess as P
from tests import pyin_ref as R
from tests.f0_signals import FRAME_PERIOD, FS, HOP, far_from_signal
from tests.golden import make_pyin_bars as G
from tests.helpers import make_raw_corpus
from tests.test_metrics_cpu import corpus, run_cli                          # noqa: F401  (the score.py corpus fixture and its driver)

BARS = G.load_bars()
CASES = {name: (x, truth) for name, x, truth in G.known_answers()}


@pytest.fixture(scope="module")
def oracle_tracks():
    return {name: R.pyin(x, FS, FRAME_PERIOD) for name, (x, _) in CASES.items()}


def test_bars_are_what_the_generator_derives():
    assert BARS["bin_width"] == 2.0 ** (1.0 / 240.0) - 1.0
    assert set(BARS["bar"]) == set(CASES) == set(BARS["oracle_error"])
    for name, err in BARS["oracle_error"].items():
        assert BARS["bar"][name] == (BARS["bin_width"] if err <= BARS["bin_width"] else err + BARS["bin_width"])


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_known_answers(oracle_tracks, name):
    f0, pv, t = oracle_tracks[name]
    voiced, err = G.worst_error(f0, CASES[name][1](t))
    print(name, "worst relative error", err, "bar", BARS["bar"][name])
    assert voiced and err <= BARS["bar"][name]
    assert abs(err - BARS["oracle_error"][name]) <= 1e-9                       # the recorded figure is this oracle's
    assert np.all((pv >= 0) & (pv <= 1))


@pytest.mark.parametrize("name", G.SILENT)
def test_oracle_silence_is_unvoiced(oracle_tracks, name):
    """digital silence of any length (a 0.3 s gap, a 1 s gap, 1.5 s of trailing zeros) stays unvoiced: a flat d' has no candidate"""
    x = CASES[name][0]
    f0, pv, t = oracle_tracks[name]
    far = far_from_signal(x, t)
    assert far.sum() >= 10 and np.all(f0[far] == 0) and np.all(pv[far] == 0)
    assert "".join(str(int(v > 0)) for v in f0) == BARS["silence_voiced"][name]


def test_oracle_all_zeros_has_no_candidate():
    f0, pv, _ = R.pyin(np.zeros(5000, np.float32), FS, FRAME_PERIOD)           # d' = 1 everywhere: flat, no mass on any voiced bin
    assert np.all(f0 == 0) and np.all(pv == 0)
    d = R.cmnd(np.full(5000, 0.25, np.float32), FS, FRAME_PERIOD)[10:12]       # a constant signal inside the row: flat as well
    obs, pv, _ = R.observe(d, FS)
    assert np.all(pv == 0) and np.all(obs[:, :839] == 0) and np.all(obs[:, 839:] == 1.0 / 839)


def test_constants_of_the_docstring():
    from fastspeech2_amd import pyin
    g = R.geometry(FS, FRAME_PERIOD)
    assert (g["hop"], g["tmin"], g["tmax"], g["nb"], g["h"]) == (HOP, 27, 311, 839, 50)
    assert pyin.hop_samples(FS, FRAME_PERIOD) == HOP and pyin.lag_range(FS) == (27, 311) and pyin.n_bins() == 839
    assert pyin.half_width(FS, HOP) == 50
    w = pyin.threshold_weights()
    assert len(w) == 100 and abs(w.sum() - 1) < 1e-12 and np.all(w >= 0) and np.abs(w - R.beta_weights()).max() < 1e-14
    x = np.arange(1, 101) / 100.0
    assert np.abs(np.cumsum(w) - (1 - (1 - x) ** 18 * (1 + 18 * x))).max() < 1e-12
    logw, logz = pyin.transition_band(839, 50)
    rw, rz = R.log_transition(839, 50)
    assert np.array_equal(logw, rw) and np.abs(logz - rz).max() < 1e-13
    assert abs(np.exp(logz[400]) - 51.0 ** 2) < 1e-9 and np.exp(logz[0]) < np.exp(logz[400])      # renormalised at the edge
    assert list(pyin.row_chunks([900, 800, 10, 5], 1800)) == [(0, 2), (2, 4)]
    assert list(pyin.row_chunks([5000, 1], 1000)) == [(0, 1), (1, 2)]
    with pytest.raises(ValueError):
        pyin._params(FS, FRAME_PERIOD, 71.0, 800.0, 32, 100, (2, 18), 0.01, 20, 35.92, 0.01)     # no lag range in 32 samples


def test_preprocessor_and_cli_take_pyin(tmp_path):
    assert P.resolve_pitch("pyin") == "pyin"
    cfg, _ = make_raw_corpus(str(tmp_path))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.Preprocessor(cfg, device="cpu", pitch="pyin")
    with pytest.raises(ValueError):
        P.Preprocessor(cfg, pitch="pyin", pitch_fn=lambda w, s, h: None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.Preprocessor(cfg, device="cpu", pitch="pyin", resample="gpu")       # allowed together: the device check is what refuses


def test_score_parser_takes_f0():
    import score
    base = ["-p", "p.yaml", "-t", "t.yaml", "--source", "val.txt"]
    assert score.parse_args(base).f0 == "dio"
    assert score.parse_args(base + ["--f0", "pyin"]).f0 == "pyin"
    with pytest.raises(SystemExit):
        score.parse_args(base + ["--f0", "harvest"])


def test_score_cli_summary_says_the_estimator(corpus):                        # noqa: F811
    _, _, summary = run_cli(corpus, ["--f0", "pyin"], [])
    assert summary["f0_estimator"] == "pyin" and summary["utterances"] == 2
    assert "f0_estimator" not in run_cli(corpus, [], [])[2]                    # DIO: the summary is what it was
    assert "f0_estimator" not in run_cli(corpus, ["--f0", "pyin", "--no_f0"], [])[2]


def test_scoring_budget_counts_the_pyin_workspace():
    from fastspeech2_amd import pyin
    per_frame = 2 * 839 * 8 + 312 * 8 + 2 * 839 + 24                           # observations, d', backpointers, states + f0 + p_v scratch
    assert pyin.workspace_bytes(4, 100) == 400 * per_frame + 400 * 20
    assert pyin.workspace_bytes(1000, 900) == pyin.FRAME_BUDGET * per_frame + 900000 * 20      # one chunk at a time
    assert pyin.workspace_bytes(1, 50000) == 50000 * per_frame + 50000 * 20                    # a chunk holds at least one row


def test_metrics_refuses_an_unknown_estimator():
    from fastspeech2_amd import metrics as M
    with pytest.raises(ValueError, match="f0_estimator"):
        M.score_pairs([], [], None, FS, HOP, f0_estimator="harvest")


def test_abi_declares_the_three_stages():
    protos = _lib.parse_header()
    assert {"fs2_pyin_cmnd", "fs2_pyin_observe", "fs2_pyin_viterbi"} <= set(protos)
    assert protos["fs2_pyin_viterbi"][2][-1] == "stream" and protos["fs2_pyin_cmnd"][2][-1] == "stream"
    lib = _lib.load()
    with pytest.raises(ValueError):                                            # null pointers are refused before any launch
        _lib.call("fs2_pyin_cmnd", None, 0, None, None, 256, 2048, 311, None, 1, 1, 0, None)
    assert lib.fs2_pyin_viterbi(None, None, 839, 64, None, None, 0.01, 71.0, 240, None, None, None, 1, 1, None) == -1
