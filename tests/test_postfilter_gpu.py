"""The GPU modulation-spectrum postfilter (fastspeech2_amd/postfilter.py, csrc/fs2_msfilter.hip) against the fp64 restatement
tests/postfilter_ref.py: the statistics kernel on ragged batches fed in unequal parts, the filter kernel on the restatement's own
statistics at every length and width of interest in fp64 and with float32 trajectories, the known answers of the specification, and
utils.SynthPipeline / the two command lines end to end.  Floating outputs are held to the bars of
tests/golden/postfilter_bars.json: per case and output 16 times the distance between the fp64 and the longdouble restatement on that
case's input (tests/golden/make_postfilter_bars.py), never anything a kernel gave.  Every batch's padding is NaN."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import modspec as MS
from fastspeech2_amd import postfilter as PF
from tests import postfilter_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = json.load(open(os.path.join(ROOT, "tests", "golden", "postfilter_bars.json")))
SLACK = -7.0


def bar(case, key="y"):
    return BARS["factor"] * BARS["distance"][case][key]


def closed_form_bar(case):
    """against a closed form: the bar, and what the closed form itself is off by (the tables and the input are rounded to fp64)"""
    return bar(case) + BARS["distance"][case]["to_expected"]


def _batch(rows, dev, strided=False, dtype=np.float64):
    """(B, Tmax, K) with NaN beyond every row's frames; `strided`: a view into a larger NaN buffer, unit stride in k only"""
    lens, K = [len(r) for r in rows], rows[0].shape[1]
    pad = (3, 5) if strided else (0, 0)
    x = np.full((len(rows), max(lens) + pad[0], K + pad[1]), np.nan, dtype=dtype)
    for b, r in enumerate(rows):
        x[b, :lens[b], :K] = r
    return torch.from_numpy(x).to(dev)[:, :max(lens), :K], lens


def _tables(tab, n=2):
    return PF.Tables(tab["mu_n"], tab["sd_n"], tab["mu_g"], tab["sd_g"], n, n, 0, 0, tab["mu_n"].shape[0], 22050, 256)


@functools.lru_cache(maxsize=None)
def _filter_case(name):
    """the rows, the tables and the restatement's answer of a filter case, computed once"""
    rows, tab = ref.filter_input(name)
    return rows, tab, [ref.apply(c, tab, ref.FILTER_K[name]) for c in rows]


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("name", list(ref.STATS_CASES))
def test_statistics_in_unequal_batches_against_the_restatement(dev, name):
    rows = ref.stats_input(name)
    K = rows[0].shape[1]
    mean, sd, n, left = ref.statistics(rows)
    got = []
    for split in ref.STATS_SPLITS[name]:
        for rep in range(2 if len(split) == 3 else 1):                      # the first split twice: the same bytes
            s = PF.Stats(K, 22050, 256)
            kept = 0
            for lo, hi in zip(split[:-1], split[1:]):
                c, lens = _batch(rows[lo:hi], dev)
                kept += s.add_natural(c, lens)
                s.add_generated(c, lens)
            t = s.finalize()
            assert kept == n == t.n_natural == t.n_generated and t.left_out_natural == left == t.left_out_generated     # dropped rows are counted
            w_m, w_s = float(np.abs(t.mu_n - mean).max()), float(np.abs(t.sd_n - sd).max())
            print(f"{name} {split}: mean {w_m:.2e} (bar {bar(name, 'mean'):.2e}), sd {w_s:.2e} (bar {bar(name, 'sd'):.2e})")
            assert np.isfinite(t.mu_n).all() and np.isfinite(t.sd_n).all()
            assert w_m <= bar(name, "mean") and w_s <= bar(name, "sd")
            assert t.mu_g.tobytes() == t.mu_n.tobytes() and t.sd_g.tobytes() == t.sd_n.tobytes()
            got.append(t)
    assert got[0].mu_n.tobytes() == got[1].mu_n.tobytes() and got[0].sd_n.tobytes() == got[1].sd_n.tobytes()
    s = PF.Stats(K, 22050, 256)
    short = [r for r in rows if len(r) < ref.MIN_FRAMES]
    assert s.add_natural(*_batch(short, dev)) == 0 and s.left_out["natural"] == len(short)
    with pytest.raises(ValueError, match="at least 2"):
        s.finalize()


# ------------------------------------------------------------------------------------------------ filter
@pytest.mark.parametrize("name", list(ref.FILTER_CASES))
def test_filter_fp64_against_the_restatement(dev, name):
    """f80 runs on non-contiguous batch and frame strides and writes into a buffer larger than needed, whose slack and NaN padding
    must stay; rows shorter than MIN_FRAMES come back byte for byte"""
    rows, tab, want = _filter_case(name)
    odd = name == "f80"
    c, lens = _batch(rows, dev, strided=odd)
    B, K, Tmax = len(rows), rows[0].shape[1], max(lens)
    t = _tables(tab)
    out = torch.full((B, Tmax + 2, K + 3), SLACK, dtype=torch.float64, device=dev) if odd else None
    y = PF.apply(c, lens, t, ref.FILTER_K[name], out=out)
    assert y.dtype == torch.float64 and y.shape == ((B, Tmax + 2, K + 3) if odd else (B, Tmax, K))
    yh = y.cpu().numpy()
    worst = 0.0
    for b, T in enumerate(lens):
        got = yh[b, :T, :K]
        assert np.isfinite(got).all()
        if T < ref.MIN_FRAMES:
            assert got.tobytes() == np.ascontiguousarray(rows[b]).tobytes()
        else:
            worst = max(worst, float(np.abs(got - want[b]).max()))
            assert np.abs(got - rows[b]).max() > 1e-6                       # the filter did something
        rest = yh[b, T:, :K] if not odd else yh[b, T:Tmax, :K]
        assert np.all(rest == SLACK) if odd else np.isnan(rest).all()       # padding stays what it was
    print(f"{name}: y {worst:.2e} (bar {bar(name):.2e})")
    assert worst <= bar(name)
    if odd:
        assert np.all(yh[:, :, K:] == SLACK) and np.all(yh[:, Tmax:] == SLACK)
    again = PF.apply(c, lens, t, ref.FILTER_K[name]).cpu().numpy()          # a second run, into a buffer of its own: the same bytes
    for b, T in enumerate(lens):
        assert np.ascontiguousarray(again[b, :T]).tobytes() == np.ascontiguousarray(yh[b, :T, :K]).tobytes()
    assert PF.pass_through(lens) == sum(1 for T in lens if T < ref.MIN_FRAMES)
    assert PF.apply(c, lens, t, 0.0) is c                                   # k = 0: no launch, the input itself


@pytest.mark.parametrize("name", ["f13", "f80"])
def test_filter_float32_is_the_fp64_result_rounded(dev, name):
    rows, tab, _ = _filter_case(name)
    rows32 = [r.astype(np.float32) for r in rows]
    t = _tables(tab)
    k = ref.FILTER_K[name]
    c32, lens = _batch(rows32, dev, strided=name == "f80", dtype=np.float32)
    c64, _ = _batch([r.astype(np.float64) for r in rows32], dev)
    y32, y64 = PF.apply(c32, lens, t, k), PF.apply(c64, lens, t, k)
    assert y32.dtype == torch.float32 and y32.shape == c32.shape
    a, b = y32.cpu().numpy(), y64.cpu().numpy()
    for i, T in enumerate(lens):
        ulp = np.spacing(np.abs(b[i, :T]).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(a[i, :T].astype(np.float64) - b[i, :T]) <= ulp), (i, T)
        assert np.isnan(a[i, T:]).all()
        if T < ref.MIN_FRAMES:
            assert a[i, :T].tobytes() == rows32[i].tobytes()


def test_rows_longer_than_the_frame_bound_pass_through(dev):
    rows, tab, want = _filter_case("f1")
    long = np.random.default_rng(5).standard_normal((ref.MAX_FRAMES + 1, 1))
    c, lens = _batch([rows[4], long], dev)
    y = PF.apply(c, lens, _tables(tab), 1.0).cpu().numpy()
    assert y[1].tobytes() == long.tobytes() and np.abs(y[0, :lens[0]] - want[4]).max() <= bar("f1") and PF.pass_through(lens) == 1
    out = torch.full((2, ref.MAX_FRAMES + 1, 1), SLACK, dtype=torch.float64, device=dev)
    y = PF.apply(c, lens, _tables(tab), 1.0, out=out).cpu().numpy()
    assert y[1].tobytes() == long.tobytes() and np.all(y[0, lens[0]:] == SLACK)


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("name", list(ref.known_cases()))
def test_known_answers_on_the_device(dev, name):
    """equal statistics: y = x; mu_n = mu_g + 2 ln a: y - m = a^k (x - m); a constant; the clamp: 60 dB asked, exactly 20 dB given"""
    c, tab, k, expected = ref.known_cases()[name]
    x, lens = _batch([c], dev)
    y = PF.apply(x, lens, _tables(tab), k).cpu().numpy()[0]
    worst, to_ref = float(np.abs(y - expected).max()), float(np.abs(y - ref.apply(c, tab, k)).max())
    print(f"{name}: to the closed form {worst:.2e} (bar {closed_form_bar(name):.2e}), to the restatement {to_ref:.2e} (bar {bar(name):.2e})")
    assert worst <= closed_form_bar(name) and to_ref <= bar(name)
    if name == "clamp":
        assert np.abs(y - 3.25 * c).max() <= closed_form_bar(name) and np.abs(y).max() > 2.4


def test_the_corpus_moves_towards_natural_on_the_device(dev):
    """known answer 4, with the statistics trained and the filter run on the device and the scores those of `modspec`"""
    natural, generated = ref.corpus()
    bins, hz = MS.band_bins(*ref.RATE)
    s = PF.Stats(ref.CORPUS_K, *ref.RATE)
    for lo in range(0, len(natural), 7):
        s.add_natural(*_batch(natural[lo:lo + 7], dev))
        s.add_generated(*_batch(generated[lo:lo + 7], dev))
    t = s.finalize()
    assert t.n_natural == t.n_generated == len(natural) and t.left_out_natural == 0
    g, lens = _batch(generated, dev)
    n, _ = _batch(natural, dev)
    f = PF.apply(g, lens, t, 1.0)

    def summary(syn):
        (m2r, br), (m2s, bs) = MS.measure(n, lens, bins), MS.measure(syn, lens, bins)
        m2r, br, m2s, bs = (v.cpu().numpy() for v in (m2r, br, m2s, bs))
        rows = [dict(MS.row_scores(m2r[b], br[b], T, m2s[b], bs[b], T), frames_ref=T, frames_syn=T) for b, T in enumerate(lens)]
        return MS.summarize(rows)
    before, after = summary(g), summary(f)
    high = [j for j, (lo, _) in enumerate(hz) if lo >= 4]
    assert len(high) == 4
    print(before["ms_diff_db_by_band"], after["ms_diff_db_by_band"], before["gv_ratio_db_mean"], after["gv_ratio_db_mean"])
    for j in high:
        assert abs(after["ms_diff_db_by_band"][j]) < abs(before["ms_diff_db_by_band"][j]), j
    assert abs(after["gv_ratio_db_mean"]) < abs(before["gv_ratio_db_mean"])


def test_bad_arguments_are_refused_before_launch(dev):
    from fastspeech2_amd import _lib, ops
    _, tab, _ = _filter_case("f13")
    t = _tables(tab)
    c = torch.zeros(2, 40, 13, dtype=torch.float64, device=dev)
    for bad_c, lens in ((c, [0, 40]), (c, [40, 41]), (c, [40]), (c.half(), [40, 40]), (c[:, :, ::2], [40, 40]), (c[0], [40]),
                        (c[:, :, :12], [40, 40]), (c[:1].expand(2, 40, 13), [40, 40])):
        with pytest.raises(ValueError):
            PF.apply(bad_c, lens, t)
        with pytest.raises(ValueError):
            PF.Stats(13, 22050, 256).add_generated(bad_c, lens)
    for bad_out in (torch.zeros(2, 39, 13, dtype=torch.float64, device=dev), torch.zeros(2, 40, 13, device=dev), c,
                    torch.zeros(2, 40, 13, dtype=torch.float64)):
        with pytest.raises(ValueError):
            PF.apply(c, [40, 40], t, out=bad_out)
    # the C entry points themselves
    lens = torch.tensor([40, 40], dtype=torch.int32, device=dev)
    mean = torch.zeros(2, 13, dtype=torch.float64, device=dev)
    y = torch.zeros(2, 40, 13, dtype=torch.float64, device=dev)
    tw, tabs = MS._twiddles_on(dev), t.on(dev)
    call = lambda k, floor, db, minf, f64, T, K, ldt, lds: _lib.call(      # noqa: E731
        "fs2_ms_filter", c.data_ptr(), 40 * ldt, ldt, lens.data_ptr(), mean.data_ptr(), 13, 1, tw.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(),
        tabs[2].data_ptr(), tabs[3].data_ptr(), lds, k, floor, db, minf, y.data_ptr(), 520, 13, f64, 2, T, K, ops._stream())
    for args in ((1.5, 1e-12, 20.0, 32, 1, 40, 13, 13, 2049), (-0.1, 1e-12, 20.0, 32, 1, 40, 13, 13, 2049), (0.85, 0.0, 20.0, 32, 1, 40, 13, 13, 2049),
                 (0.85, 1e-12, -1.0, 32, 1, 40, 13, 13, 2049), (0.85, 1e-12, 20.0, 0, 1, 40, 13, 13, 2049), (0.85, 1e-12, 20.0, 32, 2, 40, 13, 13, 2049),
                 (0.85, 1e-12, 20.0, 32, 1, 2049, 13, 13, 2049), (0.85, 1e-12, 20.0, 32, 1, 0, 13, 13, 2049), (0.85, 1e-12, 20.0, 32, 1, 40, 129, 13, 2049),
                 (0.85, 1e-12, 20.0, 32, 1, 40, 13, 12, 2049), (0.85, 1e-12, 20.0, 32, 1, 40, 13, 13, 2048)):
        with pytest.raises(ValueError):
            call(*args)
    state = torch.zeros(13, 2049, 2, dtype=torch.float64, device=dev)
    logms = torch.zeros(2, 13, 2049, dtype=torch.float64, device=dev)
    for args in ((13 * 2049, 2048, 4098, 0, 2, 13), (13 * 2049, 2049, 4097, 0, 2, 13), (13 * 2049, 2049, 4098, -1, 2, 13),
                 (13 * 2049, 2049, 4098, 0, 2, 129), (12 * 2049, 2049, 4098, 0, 2, 13)):
        with pytest.raises(ValueError):
            _lib.call("fs2_ms_stats_update", logms.data_ptr(), args[0], args[1], lens.data_ptr(), state.data_ptr(), *args[2:], ops._stream())
    assert not y.any() and not state.any()


# ------------------------------------------------------------------------------------------------ pipeline and command lines
def _flat_tables(seed=3, K=80):
    rng = np.random.default_rng(seed)
    mu_g, sd_g = rng.standard_normal((K, ref.HALF + 1)), rng.uniform(0.5, 2.0, (K, ref.HALF + 1))
    return PF.Tables(mu_g + rng.uniform(0.0, 2.0, (K, ref.HALF + 1)), sd_g * rng.uniform(0.8, 1.25, (K, ref.HALF + 1)), mu_g, sd_g, 4, 4, 0, 0, K,
                     22050, 256)


def test_synth_pipeline_with_the_postfilter(dev):
    """SynthPipeline(postfilter=(tables, 0.85)) yields `postfilter.apply` of the unfiltered pipeline's mel, byte for byte, and wavs of
    the same lengths; with None and with k = 0 the wavs are today's bytes"""
    from oracle.weights import seeded_state_dict, synthetic_batch
    from tests.golden import configs
    from tests.helpers import make_model
    from tests.test_vocoder_stft_gpu import _generator, hifigan_weights
    from fastspeech2_amd import utils

    pcfg, mcfg = configs.make(dec_layers=2, enc_layers=2)
    model = make_model(pcfg, mcfg)
    sd = seeded_state_dict(model.state_dict(), 33)
    sd["variance_adaptor.duration_predictor.linear_layer.bias"] = torch.tensor([2.2])      # about ten frames a phone
    model.load_state_dict(sd)
    model.to(dev).eval()
    keys = sorted(hifigan_weights.__globals__["hifigan_shapes"]().keys())
    voc = _generator(hifigan_weights(14, keys), dev, dtype="fp32")
    batches = []
    for i, lens in enumerate([(3, 14, 9), (30, 2, 22, 17), (1, 9)]):
        b = synthetic_batch(40 + i, 0, 0, src_lens=lens, sort=False)
        batches.append(([f"b{i}u{j}" for j in range(len(lens))], None, b["speakers"].to(dev), b["texts"].to(dev), b["src_lens"].to(dev),
                        b["max_src_len"]))
    ctl = (1.1, 0.9, 1.3)
    t = _flat_tables()
    plain = list(utils.SynthPipeline(model, voc, (pcfg, mcfg), ctl, device=dev)(iter(batches)))
    none = list(utils.SynthPipeline(model, voc, (pcfg, mcfg), ctl, device=dev, postfilter=None)(iter(batches)))
    zero = list(utils.SynthPipeline(model, voc, (pcfg, mcfg), ctl, device=dev, postfilter=(t, 0.0))(iter(batches)))
    pipe = utils.SynthPipeline(model, voc, (pcfg, mcfg), ctl, device=dev, postfilter=(t, 0.85))
    filt = list(pipe(iter(batches)))
    moved, short = 0, 0
    for (_, o0, w0), (_, o1, w1), (_, o2, w2), (_, o3, w3) in zip(plain, none, zero, filt):
        assert torch.equal(o0[1], o1[1]) and torch.equal(o0[1], o2[1])
        assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(w0, w1, w2))
        lens = [int(n) for n in o0[9]._fs2_host]
        want = PF.apply(o0[1], lens, t, 0.85)
        assert o3[1].dtype == o0[1].dtype and torch.equal(o3[1], want) and torch.equal(o3[9], o0[9]) and len(o3) == len(o0)
        assert [len(w) for w in w3] == [len(w) for w in w0] == [n * 256 for n in lens]
        short += PF.pass_through(lens)
        print("frames", lens)
        for b, n in enumerate(lens):
            if n >= PF.MIN_FRAMES:
                moved += 1
                assert not torch.equal(o3[1][b, :n], o0[1][b, :n]) and not np.array_equal(w3[b], w0[b])
            else:
                assert torch.equal(o3[1][b, :n], o0[1][b, :n])
    assert moved >= 3 and short >= 1 and pipe.passed_through == short


def test_train_then_synthesize_with_the_postfilter_cli(dev, tmp_path, capsys):
    """`postfilter.py train` -> `synthesize.py --postfilter` on the tiny corpus with a random-init model and vocoder: the same file
    names as without the switch, through the vocoder and through Griffin-Lim; a file of another config is refused"""
    import postfilter as cli
    import synthesize as synth_cli
    from scipy.io import wavfile
    from tests.helpers import make_preprocessed_dir
    from tests.test_cli_gpu import _write_configs
    root = str(tmp_path)
    (pp, mp, tp), tcfg = _write_configs(root)
    cfgs = tuple(yaml.load(open(p), Loader=yaml.FullLoader) for p in (pp, mp, tp))
    data = cfgs[0]["path"]["preprocessed_path"]
    make_preprocessed_dir(data, seed=31, n_train=12, n_val=4, lo=14, hi=24)       # longer utterances: most hold 32 frames and more
    from fastspeech2_amd.model import FastSpeech2
    torch.manual_seed(0)
    os.makedirs(tcfg["path"]["ckpt_path"], exist_ok=True)
    sd = FastSpeech2(cfgs[0], cfgs[1]).state_dict()
    sd["variance_adaptor.duration_predictor.linear_layer.bias"] = torch.tensor([1.6])      # about four frames a phone
    torch.save({"model": sd}, os.path.join(tcfg["path"]["ckpt_path"], "5.pth.tar"))
    out = os.path.join(root, "stats.npz")
    tables = cli.main(["train", "-p", pp, "-m", mp, "-t", tp, "--restore_step", "5", "--batch_size", "5", "--max_utts", "11", out])
    said = capsys.readouterr().out
    assert "pooled over speakers" in said and f"natural: {tables.n_natural} utterances ({tables.left_out_natural} left out)" in said
    assert tables.n_natural + tables.left_out_natural == 11 == tables.n_generated + tables.left_out_generated and tables.n_natural >= 2
    back = PF.load(out, cfgs[0])
    assert back.mu_g.tobytes() == tables.mu_g.tobytes() and back.restore_step == 5 and back.n_mel == 80
    src = os.path.join(data, "val.txt")
    names = [ln.split("|")[0] for ln in open(src).read().strip().split("\n")]
    base = ["--restore_step", "5", "--mode", "batch", "--source", src, "-p", pp, "-m", mp, "-t", tp, "--batch_size", "3"]
    result = tcfg["path"]["result_path"]
    wavs = {}
    for tag, extra in (("plain", ["--random_vocoder"]), ("filtered", ["--random_vocoder", "--postfilter", out]),
                       ("zero", ["--random_vocoder", "--postfilter", out, "--postfilter_k", "0"]),
                       ("griffin", ["--griffin_iters", "2", "--postfilter", out, "--postfilter_k", "1"])):
        torch.manual_seed(11)                                               # the random-init vocoder: the same one every time
        synth_cli.main(synth_cli.parse_args(base + extra))
        assert sorted(os.listdir(result)) == sorted(n + ".wav" for n in names)
        wavs[tag] = [wavfile.read(os.path.join(result, n + ".wav"))[1] for n in names]
    assert all(len(a) == len(b) and a.dtype == b.dtype for a, b in zip(wavs["plain"], wavs["filtered"]))
    assert all(np.array_equal(a, b) for a, b in zip(wavs["plain"], wavs["zero"]))
    assert any(not np.array_equal(a, b) for a, b in zip(wavs["plain"], wavs["filtered"]))
    other = json.loads(json.dumps(cfgs[0]))
    other["preprocessing"]["stft"]["hop_length"] = 200
    with pytest.raises(ValueError, match="preprocess config"):
        PF.load(out, other)
