"""GPU: the speaker-similarity kernels (csrc/fs2_spk.hip through fastspeech2_amd/speaker.py), each alone against the numpy oracle
tests/spk_ref.py with the derived bounds of its docstring and the measured exp / log shares of tests/golden/spk_bars.json; then
the model end to end on the corpus of tests/spk_corpus.py, its known answers, its file and the command line.

Measured on the GPU (error / allowance, the worst over the shapes): printed by every test before it asserts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import _lib
from fastspeech2_amd import speaker as S
from tests import spk_corpus as SC
from tests import spk_ref as R
from tests.golden import make_spk_bars as MB
from tests.test_align_cpu import config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, NINF = float("nan"), -np.inf
BARS = json.load(open(MB.PATH))


def wide(arr, dev, pad, fill=NAN, rows=1):
    """-> (view of arr's shape inside a buffer `pad` columns wider and `rows` rows longer, filled with `fill`; the buffer)"""
    arr = np.asarray(arr, np.float64)
    buf = torch.full((arr.shape[0] + rows, arr.shape[1] + pad), fill, dtype=torch.float64, device=dev)
    view = buf[:arr.shape[0], :arr.shape[1]]
    view.copy_(torch.from_numpy(arr))
    return view, buf


def guard_intact(buf, n_rows, n_cols, fill):
    h = buf.cpu().numpy().copy()
    h[:n_rows, :n_cols] = fill
    return np.array_equal(h, np.full_like(h, fill), equal_nan=True)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ fs2_spk_loglik
def check_loglik(dev, x, a, b, c, G, pad, tag):
    N, D = x.shape
    M = len(c) // G
    xv, _ = wide(x, dev, pad)
    av, _ = wide(a, dev, pad)
    bv, _ = wide(b, dev, pad)
    lv, lbuf = wide(np.full((N, G), 7.0), dev, pad, 7.0)
    want_post = G == 1
    pv, pbuf = wide(np.full((N, M), 7.0), dev, pad, 7.0)
    got = S.loglik(xv, av, bv, up(c, dev), G, post=pv if want_post else False, out=lv)
    again = S.loglik(xv, av, bv, up(c, dev), G, post=True if want_post else False)
    lse = lv.cpu().numpy()
    assert guard_intact(lbuf, N, G, 7.0)
    if want_post:
        assert got[0].data_ptr() == lv.data_ptr() and torch.equal(again[0], lv) and torch.equal(again[1], pv)     # two runs: the same bits
        assert guard_intact(pbuf, N, M, 7.0)
    else:
        assert torch.equal(again, lv)
    worst = 0.0
    for g in range(G):
        sl = slice(g * M, (g + 1) * M)
        want = R.lse(R.comp_scores(x, a[sl], b[sl], c[sl], np.longdouble), np.longdouble)
        P, T = R.lse_bounds(x, a[sl], b[sl], c[sl])
        fin = np.isfinite(want)
        assert np.array_equal(lse[~fin, g], np.asarray(want[~fin], np.float64))                                     # -inf exactly
        tol = 2 * P + 4 * BARS["rho_lse"] * T
        err = np.abs(lse[fin, g] - want[fin])
        if fin.any():
            worst = max(worst, float((err / tol[fin]).max()))
        assert (err <= tol[fin]).all(), (tag, g, float((err / tol[fin]).max()))
    if want_post and N:
        post = pv.cpu().numpy()
        L = R.comp_scores(x, a, b, c, np.longdouble)
        want = R.posteriors(L, R.lse(L, np.longdouble), np.longdouble)
        P, T = R.post_bounds(x, a, b, c)
        tol = 2 * P + 4 * BARS["rho_post"] * T
        err = np.abs(post - want)
        print(tag, "post err / allowance", float((err / tol).max()))
        assert not np.isnan(post).any() and (err <= tol).all()
        fin = np.isfinite(R.lse(L, np.longdouble))
        assert (np.abs(post[fin].sum(1) - 1) <= tol[fin].sum(1) + R.gamma(M)).all() and (post[~fin] == 0).all()
    print(tag, "lse err / allowance", worst)
    return lse


@pytest.mark.parametrize("i", range(len(MB.LOGLIK_SHAPES)))
@pytest.mark.parametrize("pad", [0, 3])
def test_loglik_against_oracle(dev, i, pad):
    x, a, b, c, G = MB.loglik_case(i)
    check_loglik(dev, x, a, b, c, G, pad, f"{MB.LOGLIK_SHAPES[i]} pad {pad}")


def test_loglik_single_component_is_the_component_score(dev):
    """M = 1: lse is L itself, so this is the dot product alone against 2 x gamma_(2D+1) sum |terms|"""
    for i, (N, D, M, G) in enumerate(MB.LOGLIK_SHAPES):
        if M != 1:
            continue
        x, a, b, c, G = MB.loglik_case(i)
        lse = S.loglik(up(x, dev), up(a, dev), up(b, dev), up(c, dev), G).cpu().numpy()
        want, bound = R.comp_scores(x, a, b, c, np.longdouble), R.comp_bound(x, a, b, c)
        print((N, D, M, G), "L err / bound", float((np.abs(lse - want) / bound).max()))
        assert (np.abs(lse - want) <= 2 * bound).all()


@pytest.mark.parametrize("kind", ["one component", "a whole group", "all groups"])
def test_loglik_minus_infinity(dev, kind):
    rng = np.random.RandomState(11)
    for G, M, D, N in ((1, 65, 13, 65), (5, 17, 38, 17)):
        x = rng.randn(N, D)
        a, b, c = MB.draw_mixture(rng, G, M, D)
        if kind == "one component":
            c[M // 2] = NINF
        elif kind == "a whole group":
            c[(G - 1) * M:] = NINF
        else:
            c[:] = NINF
        lse = check_loglik(dev, x, a, b, c, G, 3, f"{kind} G={G}")
        if kind != "one component":
            assert (lse[:, G - 1] == NINF).all()


def test_loglik_refusals(dev):
    assert S.max_dim() == 64 and S.max_components() == 2048
    t = torch.zeros(4, 2049 * 2, dtype=torch.float64, device=dev)
    p = t.data_ptr()
    call = lambda *args: _lib.call("fs2_spk_loglik", *args, None)                                # noqa: E731
    # x, ldx, a, b, ldt, c, lse, ldl, post, ldp, N, D, M, G
    with pytest.raises(ValueError, match="dimensions"):
        call(p, 65, p, p, 65, p, p, 1, None, 0, 4, 65, 2, 1)
    with pytest.raises(ValueError, match="components"):
        call(p, 2, p, p, 2, p, p, 1, None, 0, 4, 2, 2049, 1)
    with pytest.raises(ValueError, match="one group"):
        call(p, 2, p, p, 2, p, p, 2, p, 2, 4, 2, 2, 2)
    for nulls in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        xx, aa, bb, cc, ll = nulls
        with pytest.raises(ValueError, match="null"):
            call(xx, 2, aa, bb, 2, cc, ll, 1, None, 0, 4, 2, 2, 1)
    with pytest.raises(ValueError, match="bad shape"):
        call(p, 1, p, p, 2, p, p, 1, None, 0, 4, 2, 2, 1)
    x = torch.zeros(4, 2, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        S.loglik(x, t[:4, :2], t[:4, :2], t[0, :4], 2, post=True)
    with pytest.raises(ValueError, match="fit together"):
        S.loglik(x, t[:4, :3], t[:4, :3], t[0, :4])
    with pytest.raises(RuntimeError, match="GPU"):
        S.loglik(x.cpu(), t[:4, :2], t[:4, :2], t[0, :4])


# ------------------------------------------------------------------------------------------------ fs2_spk_accum
@pytest.mark.parametrize("i", range(len(MB.ACCUM_SHAPES)))
def test_accum_against_oracle(dev, i):
    N, D, M = MB.ACCUM_SHAPES[i]
    post, x = MB.accum_case(i)
    pv, _ = wide(post, dev, 2)
    xv, _ = wide(x, dev, 3)
    sv, sbuf = wide(np.zeros((M, 1 + 2 * D)), dev, 2, 0.0)
    need = S.accum_ws(N, D, M)
    ws = torch.full((need + 8,), 3.0, dtype=torch.float64, device=dev)
    S.accumulate(pv, xv, sv, ws[:max(need, 1)] if need else ws[:1])
    assert (ws[need:] == 3.0).all()                                        # the workspace guard
    got = sv.cpu().numpy()
    again = S.accumulate(pv, xv)
    assert torch.equal(again, sv)                                          # two runs, own workspace: the same bits
    assert guard_intact(sbuf, M, 1 + 2 * D, 0.0)
    want, bound = R.accumulate(post, x, np.longdouble), R.stats_bound(post, x)
    err = np.abs(got - want)
    print((N, D, M), "stats err / bound", float((err / np.maximum(bound, 1e-300)).max()), "chunks x tiles", need // 4096)
    assert (err <= 2 * bound).all()
    if N:
        S.accumulate(pv, xv, sv)                                           # a second batch adds to the table
        assert (np.abs(sv.cpu().numpy() - 2 * want) <= 4 * bound + R.U * np.abs(2 * want)).all()
        with pytest.raises(ValueError, match="workspace"):
            _lib.call("fs2_spk_accum", pv.data_ptr(), pv.stride(0), xv.data_ptr(), xv.stride(0), sv.data_ptr(), sv.stride(0), ws.data_ptr(),
                      need - 1, N, D, M, None)


def test_accum_plan():
    ws = S.accum_ws
    assert ws(0, 13, 16) == 0 and ws(16, 2, 3) == 4096 and ws(17, 2, 3) == 2 * 4096 and ws(511, 1, 16) == 32 * 4096
    assert ws(513, 38, 65) == 17 * 2 * 2 * 4096 and ws(513, 64, 64) == 17 * 3 * 4096 and ws(5, 65, 1) == 0 and ws(5, 1, 2049) == 0


# ------------------------------------------------------------------------------------------------ fs2_spk_feats
@pytest.mark.parametrize("n_cep", [1, 5, 19, 32])
def test_feats_against_oracle(dev, n_cep):
    rng = np.random.RandomState(n_cep)
    lens = [0, 1, 2, 3, 5, 37, 64, 40, 40, 300]
    floor = 6.0
    ceps = []
    for b, T in enumerate(lens):
        c = rng.randn(T, n_cep + 1) * (0.5 + rng.rand(n_cep + 1)) + rng.randn(n_cep + 1)
        c[:, 0] = rng.uniform(0, 2 * floor, T)                             # some frames pass, some do not
        if b == 5:
            c[:, 0] = [10.0] + [0.0] * (T - 1)                             # exactly one passes
        if b == 6:
            c[:, 0] = rng.uniform(0, floor / 2, T)                         # all pass
        if b == 7:
            c[:, 0] = np.linspace(0, 100 * floor, T)                       # only the last passes
        if b == 8:
            c[:, 1:] = 1.25                                                # constant: zero variance
        ceps.append(c)
    Tm, K, D, Ntot = max(lens), n_cep + 1, 2 * n_cep, sum(lens)
    buf = torch.full((len(lens), Tm + 1, K + 2), NAN, dtype=torch.float64, device=dev)
    cep = buf[:, :Tm, :K]
    for b, c in enumerate(ceps):
        cep[b, :len(c)] = torch.from_numpy(c)
    fv, fbuf = wide(np.full((Ntot, D), 9.0), dev, 2, 9.0)
    feat, offs, n_kept, mean, var = S.features(cep, lens, floor, out=fv)
    feat2, _, n2, mean2, var2 = S.features(cep, lens, floor)
    nk, fh, mh, vh = n_kept.tolist(), fbuf.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
    assert offs == [int(v) for v in np.cumsum([0] + lens[:-1])]
    assert torch.equal(n_kept, n2)
    assert np.array_equal(mh, mean2.cpu().numpy(), equal_nan=True) and np.array_equal(vh, var2.cpu().numpy(), equal_nan=True)
    written = np.zeros((Ntot + 1, D + 2), bool)
    worst = 0.0
    for b, c in enumerate(ceps):
        want = R.features(c, floor, np.longdouble)
        assert nk[b] == want["n_kept"], (b, nk[b], want["n_kept"])
        rows = slice(offs[b], offs[b] + nk[b])
        written[rows, :D] = True
        if nk[b]:
            err = np.abs(fh[rows, :D] - want["x"])
            worst = max(worst, float((err / want["bound"]).max()))
            assert (err <= 2 * want["bound"]).all(), (b, float((err / want["bound"]).max()))
            assert torch.equal(feat2[rows], fv[rows])                      # two runs: the same bits
            assert np.allclose(mh[b], np.asarray(want["mean"], np.float64), rtol=1e-12, atol=1e-13)
            assert np.allclose(vh[b], np.asarray(want["var"], np.float64), rtol=1e-12)
    assert nk[:4] == [0, 0] + nk[2:4] and nk[5] == 0 and nk[6] == 64 and nk[7] == 0 and nk[8] == 0 and nk[9] >= 2
    assert (vh[8] == 0).all() and np.isnan(mh[5]).all()
    assert (fh[~written] == 9.0).all()                                     # rows beyond n_kept and every guard cell untouched
    print("n_cep", n_cep, "n_kept", nk, "feature err / bound", worst)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="cepstra"):
            _lib.call("fs2_spk_feats", cep.data_ptr(), cep.stride(0), cep.stride(1), n_kept.data_ptr(), n_kept.data_ptr(), bad, floor,
                      fv.data_ptr(), 80, n_kept.data_ptr(), mean.data_ptr(), var.data_ptr(), 80, len(lens), Tm, None)


# ------------------------------------------------------------------------------------------------ fs2_spk_mean_rows
@pytest.mark.parametrize("G", [1, 5])
def test_mean_rows_against_oracle(dev, G):
    rng = np.random.RandomState(G)
    n_kept = [0, 1, 2, 65, 3, 4]
    lens = [2, 1, 4, 65, 3, 4]                                             # blocks with rows beyond n_kept
    offs = [int(v) for v in np.cumsum([0] + lens[:-1])]
    N = sum(lens)
    lse, ubm = 5 * rng.randn(N, G), 5 * rng.randn(N)
    lse[offs[4] + 1, 0] = NINF                                             # -inf in lse alone: -inf
    lse[offs[5], G - 1] = NINF
    ubm[offs[5]] = NINF                                                    # in both: NaN (and -inf - finite elsewhere in the row: +inf)
    lv, _ = wide(lse, dev, 2)
    ov, obuf = wide(np.full((len(lens), G), 7.0), dev, 2, 7.0)
    out = S.mean_rows(lv, up(ubm, dev), offs, n_kept, out=ov).cpu().numpy()
    want, bound = R.mean_rows(lse, ubm, offs, n_kept, np.longdouble)
    assert guard_intact(obuf, len(lens), G, 7.0)
    assert np.isnan(out[0]).all() and out[4, 0] == NINF and np.isnan(out[5, G - 1])
    fin = np.isfinite(np.asarray(want, np.float64))
    assert np.array_equal(out[~fin], np.asarray(want, np.float64)[~fin], equal_nan=True)
    print("G", G, "mean err / bound", float((np.abs(out[fin] - want[fin]) / bound[fin]).max()))
    assert (np.abs(out[fin] - want[fin]) <= 2 * bound[fin]).all()
    assert np.array_equal(S.mean_rows(lv, up(ubm, dev), offs, n_kept).cpu().numpy(), out, equal_nan=True)          # two runs: the same bits
    with pytest.raises(ValueError, match="fit together"):
        S.mean_rows(lv, up(ubm, dev), offs, [n + 1 for n in lens])


# ------------------------------------------------------------------------------------------------ end to end
def gpu_features(dev, utts):
    """the corpus utterances through cepstra0 and features on the GPU -> [kept frames (n, D) on the host]"""
    lens = [u["mel"].shape[1] for u in utts]
    mel = torch.zeros(len(utts), SC.N_MEL, max(lens), dtype=torch.float32)
    for b, u in enumerate(utts):
        mel[b, :, :lens[b]] = torch.from_numpy(u["mel"])
    feat, offs, n_kept, _, _ = S.features(S.cepstra0(mel.to(dev), lens, SC.N_CEP), lens, S.default_energy_floor(SC.N_MEL))
    feat, n_kept = feat.cpu(), n_kept.tolist()
    return [feat[o:o + n].clone() for o, n in zip(offs, n_kept)]


@pytest.fixture(scope="module")
def trained(dev):
    """seed -> (model, training features per utterance, held-out features, train, held), GPU-trained"""
    out = {}
    for seed in SC.SEEDS:
        train, held = SC.corpus(seed)
        ft, fh = gpu_features(dev, train), gpu_features(dev, held)
        model = S.SpeakerModel(dev, SC.N_CEP, SC.M, SC.ITERS, feature_config={"n_mel": SC.N_MEL})
        pools = [torch.cat([f for f, u in zip(ft, train) if u["speaker"] == s]) for s in range(SC.N_SPEAKERS)]
        model.fit_ubm(torch.cat(pools))
        model.enrol([(f"s{s}", p) for s, p in enumerate(pools)])
        out[seed] = (model, pools, fh, train, held)
    return out


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_llr_matrix_against_the_oracle_on_the_gpu_tables(trained, seed):
    model, _, fh, _, held = trained[seed]
    llr = model.score(fh)
    X, offs, n = MB.pack([f.numpy() for f in fh])
    ubm = {"w": model.w, "mu": model.mu, "var": model.var}
    want, (P, T) = R.llr_matrix(X, offs, n, ubm, list(model.means), np.longdouble)
    tol = 2 * P + 4 * BARS["rho_lse"] * T
    print("seed", seed, "llr err / allowance", float((np.abs(llr - want) / tol).max()))
    assert (np.abs(llr - want) <= tol).all()
    rep = R.report(llr, [u["speaker"] for u in held])
    print("seed", seed, rep, "oracle", BARS["seeds"][str(seed)])
    assert rep["accuracy"] >= BARS["accuracy_bar"] and rep["eer"] <= BARS["eer_bar"]
    assert np.array_equal(llr, model.score(fh))                            # two runs: the same bits


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_ubm_training_against_the_oracle(trained, seed):
    model, pools, _, _, _ = trained[seed]
    want = R.fit_ubm(np.concatenate([p.numpy() for p in pools]), SC.M, SC.ITERS)
    got, ref = model.history[-1][-1], want["history"][-1][-1]
    print("seed", seed, "loglik per frame", got, ref, "means", MB.nearest(model.mu, want["mu"]))
    assert [len(h) for h in model.history] == [len(h) for h in want["history"]]
    assert abs(got - ref) <= BARS["ll_tol"] and MB.nearest(model.mu, want["mu"]) <= BARS["mean_tol"]
    assert MB.nearest(want["mu"], model.mu) <= BARS["mean_tol"]


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_known_answers(dev, trained, seed):
    """tests/test_spk_cpu.py confirms these for the oracle on every seed.  With r = 1e12, alpha <= n / r < 1e-9 and the adapted means
    leave the UBM's by less than 1e-9 of a spread, so |llr| stays under 1e-8."""
    model, pools, fh, _, held = trained[seed]
    Dm = SC.distortions()
    utt = next(u for u in held if u["speaker"] == 0)
    rows = [model.score(gpu_features(dev, [{"mel": SC.distort(utt["base"], (1 - al) * Dm[0] + al * Dm[1])}]))[0] for al in (0.0, 0.5, 1.0)]
    print("seed", seed, "target llr over alpha", [r[0] for r in rows])
    assert rows[0][0] > rows[1][0] > rows[2][0] and S.rank_and_rival(rows[2], 1)[0] == 1
    flat = S.SpeakerModel(dev, SC.N_CEP, SC.M, SC.ITERS, relevance=1e12)
    flat.w, flat.mu, flat.var = model.w, model.mu, model.var
    flat.enrol([(f"s{s}", p) for s, p in enumerate(pools)])
    assert np.abs(flat.score(fh)).max() < 1e-8


def test_save_load_and_refusals(dev, trained, tmp_path):
    model, pools, fh, _, _ = trained[SC.SEEDS[0]]
    path = str(tmp_path / "spk.npz")
    model.save(path)
    back = S.SpeakerModel.load(path, dev, {"n_mel": SC.N_MEL})
    assert back.names == model.names and back.options() == model.options() and back.history == model.history
    assert np.array_equal(back.score(fh), model.score(fh))
    with pytest.raises(ValueError, match="feature settings"):
        S.SpeakerModel.load(path, dev, {"n_mel": 40})
    with pytest.raises(ValueError, match="power of two"):
        S.SpeakerModel(dev, components=12)
    empty = fh[:1] + [fh[0][:0]]
    assert np.isnan(model.score(empty)[1]).all() and not np.isnan(model.score(empty)[0]).any()


def test_command_line(dev, tmp_path):
    """`speaker.py train` then `speaker.py score` on wavs: rows, the summary, a missing wav and an unknown speaker listed, and the
    refusal of a list of one speaker."""
    root = str(tmp_path)
    train, held = SC.wav_corpus(root, 7)
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(config(root), f)
    lists = {"train.txt": train, "one.txt": [e for e in train if e[1] == "spa"],
             "val.txt": held + [("nowav", "spa"), (held[0][0], "stranger")]}
    for name, entries in lists.items():
        with open(os.path.join(root, name), "w") as f:
            f.writelines(f"{n}|{s}|{{AA}}|text\n" for n, s in entries)
    wavs = os.path.join(root, "wavs")
    os.makedirs(wavs)
    for n, s in held:
        os.symlink(os.path.join(root, "raw", s, n + ".wav"), os.path.join(wavs, n + ".wav"))
    model, out = os.path.join(root, "spk.npz"), os.path.join(root, "rows.jsonl")
    base = [sys.executable, os.path.join(ROOT, "speaker.py")]
    cfg = os.path.join(root, "preprocess.yaml")
    one = subprocess.run(base + ["train", cfg, model, "--source", os.path.join(root, "one.txt"), "--components", "4"], capture_output=True,
                         text=True, cwd=ROOT, timeout=600)
    assert one.returncode != 0 and "at least two" in one.stderr and not os.path.exists(model)
    run = subprocess.run(base + ["train", cfg, model, "--source", os.path.join(root, "train.txt"), "--components", "8", "--iters", "2",
                                 "--n_cep", "12"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "3 speakers enrolled, 8 components of 24 dimensions" in run.stdout
    run = subprocess.run(base + ["score", model, "-p", cfg, "--source", os.path.join(root, "val.txt"), "--wav_dir", wavs, "--out", out],
                         capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    rows = [json.loads(ln) for ln in open(out)]
    assert [r["basename"] for r in rows] == [n for n, _ in held]
    for r in rows:
        assert set(r) == {"basename", "speaker", "llr", "rank", "rival", "margin", "n_kept"}
        assert 1 <= r["rank"] <= 3 and r["rival"] in ("spa", "spb", "spc") and r["rival"] != r["speaker"] and r["n_kept"] >= 2
        assert (r["rank"] == 1) == (r["margin"] > 0 or (r["margin"] == 0 and r["speaker"] < r["rival"]))
    assert "skipped nowav: missing " in run.stdout and "speaker stranger is not in the model" in run.stdout
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["utterances"] == len(held) and summary["missing"] == 2 and summary["speakers_enrolled"] == 3
    assert summary["accuracy"] == np.mean([r["rank"] == 1 for r in rows]) and set(summary["per_speaker"]) == {"spa", "spb", "spc"}
    assert abs(summary["mean_llr"] - np.mean([r["llr"] for r in rows])) < 1e-12 and 0 <= summary["eer"] <= 1
    print("tones:", {k: summary[k] for k in ("mean_llr", "accuracy", "eer")})
