"""GPU pYIN (fastspeech2_amd.pyin, csrc/fs2_pyin.hip): each of the three stages against the numpy oracle tests/pyin_ref.py on the
oracle's own input, then the whole estimator: known answers within tests/golden/pyin_bars.json, ragged batches with poisoned padding,
amplitude invariance, the API's refusals, the preprocessor and the scores with the estimator swapped in, and real speech.
Every test prints the figure it asserts on before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from fastspeech2_amd import pitch, pyin
from fastspeech2_amd import preprocess as P
from tests import pyin_ref as R
from tests.f0_signals import FRAME_PERIOD, FS, HOP, far_from_signal, speech, tone
from tests.golden import make_pyin_bars as G

pytestmark = pytest.mark.gpu
BARS = G.load_bars()


def _batch(xs, dev, poison=0.0):
    lens = [len(x) for x in xs]
    y = torch.full((len(xs), max(max(lens), 1)), poison, dtype=torch.float32)
    for b, x in enumerate(xs):
        y[b, :len(x)] = torch.from_numpy(np.asarray(x, np.float32))
    return y.to(dev), lens


def _pad(rows, dev, dtype=torch.float64):
    """[(F_b, ...) arrays] -> (B, Fmax, ...) device tensor, zero beyond each row's frames"""
    Fmax = max(len(r) for r in rows)
    out = torch.zeros((len(rows), Fmax) + rows[0].shape[1:], dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.from_numpy(np.ascontiguousarray(r))
    return out.to(dev)


@pytest.fixture(scope="module")
def oracle():
    """the oracle's every stage on the known-answer signals and the speech fixture, computed once"""
    x_sp, sr = speech()
    assert sr == FS
    cases = [(name, x) for name, x, _ in G.known_answers()] + [("speech", x_sp)]
    return {name: (x,) + R.pyin(x, FS, FRAME_PERIOD, full=True) for name, x in cases}


# ------------------------------------------------------------------------------------------------ stage 1
def _check_cmnd(xs, fs, frame_period, L, dev, what, fmin=R.FMIN):
    g = R.geometry(fs, frame_period, fmin=fmin, frame_length=L)
    y, lens = _batch(xs, dev, poison=float("nan"))
    frames = [pitch.frame_count(n, fs, frame_period) for n in lens]
    got = pyin.cmnd(y, lens, frames, g["hop"], L, g["tmax"]).cpu().numpy()
    assert got.shape == (len(xs), max(frames), g["tmax"] + 1)
    worst = 0.0
    for b, x in enumerate(xs):
        want = R.cmnd(x, fs, frame_period, fmin=fmin, frame_length=L)
        assert want.shape[0] == frames[b]
        worst = max(worst, float((np.abs(got[b, :frames[b]] - want) / np.maximum(want, 1.0)).max()))
        assert np.all(got[b, frames[b]:] == 0)
        if not np.any(x):
            assert np.all(got[b, :frames[b]] == 1.0)                           # digital silence: exactly 1
    print(what, "max |d' - oracle| / max(d', 1) =", worst)
    assert worst <= 1e-10
    return got


def test_cmnd_small_ragged_batch(dev):
    """fs 8000, L 512, W 256, hop 64: a 0.25 s tone, a row shorter than L / 2 (every frame mostly padding), a row of exact zeros"""
    fs = 8000
    xs = [tone(200, 0.25, fs=fs), tone(150, 0.25, fs=fs)[:100], np.zeros(700, np.float32)]
    _check_cmnd(xs, fs, 64 / fs * 1000, 512, dev, "L=512")


def test_cmnd_defaults(dev):
    _check_cmnd([tone(110, 0.3)], FS, FRAME_PERIOD, 2048, dev, "L=2048")


def test_cmnd_large_hop_fewer_frames_per_workgroup(dev):
    """hop 2048 with L 2048: the span of 8 frames does not fit the LDS budget, a workgroup takes 2 frames; 7 frames: an odd count"""
    x = tone(150, 0.6)
    assert pitch.frame_count(len(x), FS, 2048 / FS * 1000) == 7
    _check_cmnd([x, x[:3000]], FS, 2048 / FS * 1000, 2048, dev, "hop=2048")


def test_cmnd_long_lag_range_two_passes(dev):
    """fmin 30: tau_max = 735, more than the 512 lags one pass holds in registers: a second pass over the lags 512 .. 735"""
    assert R.geometry(FS, FRAME_PERIOD, fmin=30.0)["tmax"] == 735
    _check_cmnd([tone(80, 0.2), tone(330, 0.2)[:1500]], FS, FRAME_PERIOD, 2048, dev, "tmax=735", fmin=30.0)


# ------------------------------------------------------------------------------------------------ stage 2
def test_observe_on_the_oracles_dprime(dev, oracle):
    names = ["tone80", "tone600", "glide", "tones_with_silence", "trailing_zeros", "speech"]
    rows = [oracle[n][4]["dprime"] for n in names]
    frames = [len(r) for r in rows]
    flagged = np.concatenate([oracle[n][4]["boundary"] for n in names])
    assert flagged.mean() <= 0.01, flagged.mean()                               # a condition on the inputs, met under the oracle alone
    g = R.geometry(FS, FRAME_PERIOD)
    obs, pv = pyin.observe(_pad(rows, dev), frames, g["tmin"], FS)
    obs, pv = obs.cpu().numpy(), pv.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(names):
        info = oracle[n][4]
        ok = ~info["boundary"]
        worst = max(worst, float(np.abs(obs[b, :frames[b]][ok] - info["obs"][ok]).max()))
        assert np.abs(obs[b, :frames[b]].sum(axis=1) - 1).max() <= 1e-12
        assert np.abs(pv[b, :frames[b]][ok] - oracle[n][2][ok]).max() <= 1e-12
        assert np.all(obs[b, frames[b]:] == 0) and np.all(pv[b, frames[b]:] == 0)
    print("observe max |obs - oracle| =", worst, "flagged share", flagged.mean())
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------ stage 3
def _synthetic_obs(rng, nb, targets):
    """rows with 0.8 at the target bin (None: no candidate stands out) over a continuous random floor, so that no two paths tie"""
    rows = []
    for tb in targets:
        voiced = rng.uniform(1e-6, 2e-6, nb)
        if tb is not None:
            voiced[tb] += 0.8
        pv = min(voiced.sum(), 1.0)
        rows.append(np.concatenate([voiced, np.full(nb, (1 - pv) / nb)]))
    return np.stack(rows)


def _check_viterbi(cases, h, dev, what):
    want = []
    for name, obs in cases:
        states, ll, margin = R.viterbi(obs, h)
        assert margin > 1e-9, (name, margin)                                   # the inputs hold no tie: verified under the oracle
        want.append((states, ll))
    frames = [len(o) for _, o in cases]
    st, f0 = pyin.viterbi(_pad([o for _, o in cases], dev), frames, h)
    st, f0 = st.cpu().numpy(), f0.cpu().numpy()
    nb = cases[0][1].shape[1] // 2
    for b, (name, obs) in enumerate(cases):
        states, ll = want[b]
        got_ll = R.log_likelihood(st[b, :frames[b]], obs, h)
        print(what, name, "log-likelihood", got_ll, "oracle", ll, "differing states", int(np.sum(st[b, :frames[b]] != states)))
        assert abs(got_ll - ll) <= 1e-9 * abs(ll), name
        assert np.array_equal(st[b, :frames[b]], states), name
        ref_f0 = R.states_to_f0(states, nb, 240, pyin.F0_FLOOR)
        assert np.all(np.abs(f0[b, :frames[b]] - ref_f0) <= 1e-12 * ref_f0), name
        assert np.all(st[b, frames[b]:] == 0) and np.all(f0[b, frames[b]:] == 0)
    return st


def test_viterbi_on_the_oracles_obs(dev, oracle):
    rng = np.random.RandomState(11)
    nb = 839
    tone_obs = oracle["tone200"][4]["obs"]
    cases = [("F=1", tone_obs[20:21]), ("F=2", tone_obs[20:22]), ("tone200", tone_obs), ("glide", oracle["glide"][4]["obs"]),
             ("bin 0", _synthetic_obs(rng, nb, [0, 0, 3, 0, 0])), ("bin nb-1", _synthetic_obs(rng, nb, [nb - 1, nb - 1, nb - 4, nb - 1])),
             ("voicing flip", _synthetic_obs(rng, nb, [300, 300, 310, None, None, None, 310, 300]))]
    st = _check_viterbi(cases, 50, dev, "nb=839")
    flip = st[6, :8]
    assert np.all(flip[:3] < nb) and np.all(flip[3:6] >= nb) and np.all(flip[6:] < nb)        # the row does flip, both ways
    assert np.all(st[4, :5] % nb <= 3) and np.all(st[5, :4] % nb >= nb - 4)


def test_viterbi_small_state_space(dev):
    """fmin 100, fmax 200: 241 bins, 482 states in a workgroup of 1024 threads; and a narrow band"""
    rng = np.random.RandomState(12)
    nb = 241
    cases = [("walk", _synthetic_obs(rng, nb, [0, 30, 60, 100, 150, 200, 240, 240, None, 120])), ("F=1", _synthetic_obs(rng, nb, [7]))]
    _check_viterbi(cases, 50, dev, "nb=241 h=50")
    _check_viterbi(cases, 10, dev, "nb=241 h=10")


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def gpu_result(dev, oracle):
    names = list(oracle)
    y, lens = _batch([oracle[n][0] for n in names], dev, poison=float("nan"))
    f0, pv, t, frames, states = pyin.pyin(y, lens, FS, FRAME_PERIOD, return_states=True)
    return names, f0.cpu().numpy(), pv.cpu().numpy(), t, frames.numpy(), states.cpu().numpy()


def test_known_answers_within_the_bars(gpu_result, oracle):
    names, f0, pv, t, frames, _ = gpu_result
    for b, (name, _, truth) in enumerate(G.known_answers()):
        assert names[b] == name and frames[b] == len(oracle[name][1])
        voiced, err = G.worst_error(f0[b, :frames[b]], truth(t[:frames[b]]))
        print(name, "worst relative error", err, "bar", BARS["bar"][name])
        assert voiced and err <= BARS["bar"][name], name
        assert np.all(f0[b, frames[b]:] == 0) and np.all(pv[b, frames[b]:] == 0) and np.all(np.isfinite(f0[b]))
    for name in G.SILENT:                                                       # digital silence of any length stays unvoiced
        b = names.index(name)
        far = far_from_signal(oracle[name][0], t[:frames[b]])
        assert far.sum() >= 10 and np.all(f0[b, :frames[b]][far] == 0) and np.all(pv[b, :frames[b]][far] == 0), name
        assert "".join(str(int(v > 0)) for v in f0[b, :frames[b]]) == BARS["silence_voiced"][name], name


def test_real_speech_plausible(gpu_result, oracle, dev):
    names, f0, _, _, frames, _ = gpu_result
    b = names.index("speech")
    v = f0[b, :frames[b]]
    share, want = float(np.mean(v > 0)), float(np.mean(oracle["speech"][1] > 0))
    assert abs(share - want) <= 0.02, (share, want)
    assert np.all((v[v > 0] >= pyin.F0_FLOOR) & (v[v > 0] <= pyin.F0_CEIL))
    y, lens = _batch([oracle["speech"][0]], dev)
    d, _, fr = pitch.dio_stonemask(y, lens, FS, FRAME_PERIOD)
    d = d[0, :fr[0]]
    both = (v > 0) & (d > 0)
    print("speech: voiced share pyin %.3f (oracle %.3f) dio %.3f; both voiced %d frames, of which |pyin / dio - 1| > 0.2 on %.3f" % (
        share, want, float(np.mean(d > 0)), int(both.sum()), float(np.mean(np.abs(v[both] / d[both] - 1) > 0.2)) if both.any() else 0.0))


def test_ragged_rows_bitwise_alone(dev):
    """each row of a mixed batch, walked in several chunks == that row alone, bitwise; NaN / huge padding never reaches an output"""
    x_sp = speech()[0]
    xs = [x_sp[:12000], tone(200)[:256], tone(330)[:1], np.zeros(0, np.float32), tone(110)[:5000], x_sp[7000:13000]]
    for poison in (float("nan"), 3.0e30):
        y, lens = _batch(xs, dev, poison=poison)
        f0, pv, _, frames = pyin.pyin_numpy(y, lens, FS, FRAME_PERIOD, frame_budget=60)
        assert frames.tolist() == [pitch.frame_count(n, FS, FRAME_PERIOD) for n in lens]
        assert np.all(np.isfinite(f0)) and np.all(np.isfinite(pv))
        for b, x in enumerate(xs):
            y1, l1 = _batch([x], dev, poison=-poison)
            g1, p1, _, fr1 = pyin.pyin_numpy(y1, l1, FS, FRAME_PERIOD)
            assert fr1[0] == frames[b]
            assert np.array_equal(f0[b, :frames[b]], g1[0]) and np.array_equal(pv[b, :frames[b]], p1[0]), b
            assert np.all(f0[b, frames[b]:] == 0)
    assert np.any(f0[0] > 0) and np.any(f0[4] > 0)


def test_amplitude_invariance(dev, oracle):
    xs = [oracle["tone150"][0], oracle["glide"][0]]
    assert min(oracle["tone150"][4]["margin"], oracle["glide"][4]["margin"]) > 1e-6      # far from a tie: a 1e-7 change moves no state
    y, lens = _batch(xs, dev)
    a = pyin.pyin(y, lens, FS, FRAME_PERIOD, return_states=True)[4]
    b = pyin.pyin(y * 0.1, lens, FS, FRAME_PERIOD, return_states=True)[4]
    assert torch.equal(a, b)


def test_api_checks(dev):
    y, lens = _batch([tone(200)[:4000]], dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pyin.pyin(y.cpu(), lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pyin.pyin(y.double(), lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pyin.pyin(y[0], lens, FS, FRAME_PERIOD)
    with pytest.raises(ValueError):
        pyin.pyin(y, [y.shape[1] + 1], FS, FRAME_PERIOD)
    with pytest.raises(ValueError, match="one-byte backpointer"):
        pyin.pyin(y, lens, FS, FRAME_PERIOD, max_transition_rate=80.0)          # h = 110: 2 (2 h + 1) > 255
    obs = torch.full((1, 2, 2 * 839), 1.0 / 1678, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="one-byte backpointer"):              # FS2_EINVAL from the entry point itself
        pyin.viterbi(obs, [2], 64)
    with pytest.raises(ValueError):
        pyin.viterbi(obs.float(), [2], 50)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pyin.observe(torch.ones(1, 2, 312, dtype=torch.float64), [2], 27, FS)   # host tensor
    out = pyin.pitch_fn(dev)(tone(200), FS, 256)
    assert out.dtype == np.float64 and len(out) == pitch.frame_count(FS, FS, FRAME_PERIOD)


def test_preprocessor_with_pyin_matches_the_oracle(dev, tmp_path, monkeypatch):
    """raw corpus -> Preprocessor(pitch="pyin") writes what pitch_fn=pyin.pitch_fn(dev) writes, byte for byte, and frame-level pitch
    files that agree with the oracle's on its voiced interior (voiced frames at least two frames from an unvoiced one)."""
    from tests.helpers import make_raw_corpus
    from tests.test_f0_gpu import _tree

    real = os.listdir
    monkeypatch.setattr(os, "listdir", lambda p: sorted(real(p)))
    trees = {}
    for tag, kw in (("pyin", dict(pitch="pyin", batch_seconds=2.5)), ("fn", dict(pitch_fn=pyin.pitch_fn(dev))),
                    ("oracle", dict(pitch_fn=lambda w, sr, hop: R.pyin(w, sr, hop / sr * 1000)[0]))):
        cfg, _ = make_raw_corpus(str(tmp_path / tag))
        cfg["preprocessing"]["pitch"].update(feature="frame_level", normalization=False)
        P.Preprocessor(cfg, device=dev, seed=3, **kw).build_from_path()
        trees[tag] = {k: v for k, v in _tree(cfg["path"]["preprocessed_path"]).items() if not k.startswith("TextGrid")}
    assert trees["pyin"].keys() == trees["fn"].keys() == trees["oracle"].keys()
    assert all(trees["pyin"][k] == trees["fn"][k] for k in trees["pyin"]), [k for k in trees["pyin"] if trees["pyin"][k] != trees["fn"][k]]
    files = [k for k in trees["pyin"] if k.startswith("pitch")]
    assert len(files) >= 3
    checked = 0
    for k in files:
        got, want = (np.load(os.path.join(str(tmp_path / tag), "pre", k)) for tag in ("pyin", "oracle"))
        assert got.shape == want.shape
        v = np.concatenate([[False] * 2, want > 0, [False] * 2])
        inner = v[0:-4] & v[1:-3] & v[2:-2] & v[3:-1] & v[4:]
        assert np.all(np.abs(got[inner] - want[inner]) <= 1e-12 * want[inner]), k
        checked += int(inner.sum())
    assert checked >= 20


def test_metrics_with_pyin(dev):
    from fastspeech2_amd import audio as Audio
    from fastspeech2_amd import metrics as M
    stft = Audio.TacotronSTFT(1024, HOP, 1024, 80, FS, 0, 8000)
    ref, syn = tone(200)[:16000], tone(210)[:15000]
    row = M.score_pairs([ref], [syn], stft, FS, HOP, device=dev, f0_estimator="pyin")[0]
    plain = M.score_pairs([ref], [syn], stft, FS, HOP, device=dev)[0]
    assert row["f0_estimator"] == "pyin" and "f0_estimator" not in plain
    assert np.isfinite(row["f0_rmse_cents"]) and row["n_voiced_pairs"] > 20
    assert abs(row["f0_rmse_cents"] - 1200 * np.log2(210 / 200)) < 15                   # 84 cents apart, bins of 5 cents
    assert row["mcd_db"] == plain["mcd_db"] and set(row) == set(plain) | {"f0_estimator"}
    print(json.dumps(row))
