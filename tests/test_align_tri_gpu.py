"""GPU: the forced aligner's triphone stage (fastspeech2_amd.align tree_gains / Aligner(triphones=L), csrc/fs2_align_tree.hip)
against the numpy oracle tests/align_tri_ref.py: the gain kernel elementwise within the derived bounds on the seeded inputs of
tests/test_align_tri_cpu.py (`kernel_case`), the best question where the oracle can tell, ties and determinism, the argument checks,
the whole schedule and decoding on the corpus of tests/align_tri_corpus.py (under mixtures, and behind LDA and fMLLR), the accuracy,
the untouched default and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from fastspeech2_amd import _lib, align as A
from fastspeech2_amd import preprocess as P
from tests import align_corpus as C
from tests import align_fmllr_ref as FR
from tests import align_tri_corpus as TC
from tests import align_tri_ref as TR
from tests.test_align_cpu import config
from tests.test_align_gpu import NAN, ROOT, padded
from tests.test_align_tri_cpu import (E2E_ITERS, E2E_LEAVES, E2E_MIN_OCC, E2E_N_UTT, E2E_SEED, E2E_TRI_ITERS, KERNEL_DIMS, KERNEL_MIN_OCC,
                                      KERNEL_SETS, decided, kernel_case, kernel_reference, mono, tri)

pytestmark = pytest.mark.gpu


def upload(c, dev, pad_rows=5, pad_cols=3):
    """the case on the device; the item table is a strided view into a NaN-filled buffer with rows and columns to spare"""
    N, cols = c["sums"].shape
    buf = torch.full((N + pad_rows, cols + pad_cols), NAN, dtype=torch.float64, device=dev)
    buf[:N, :cols] = torch.from_numpy(c["sums"]).to(dev)
    offs = np.zeros(len(c["nodes"]) + 1, np.int32)
    np.cumsum([len(it) for it in c["nodes"]], out=offs[1:])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    extra = lambda a: torch.cat([t(a), torch.zeros(pad_rows, dtype=torch.int32, device=dev)])            # noqa: E731
    return (buf[:, :cols], extra(c["left"]), extra(c["right"]), t(offs), t(np.concatenate(c["nodes"]).astype(np.int32)), t(c["member"]),
            t(c["floor"]))


@pytest.mark.parametrize("n_sets", KERNEL_SETS)
@pytest.mark.parametrize("D", KERNEL_DIMS)
def test_gains_against_oracle(dev, D, n_sets):
    c, g, ny, nn, bound, unsure, eny = kernel_reference(D, n_sets)
    args = upload(c, dev)
    best_q, best_gain, gains, n_yes = A.tree_gains(*args, KERNEL_MIN_OCC, full=True)
    gk, nk, bq, bg = gains.cpu().numpy(), n_yes.cpu().numpy(), best_q.cpu().numpy(), best_gain.cpu().numpy()
    assert gk.shape == g.shape == (len(c["nodes"]), 2 * n_sets) and not np.isnan(gk).any() and not np.isnan(nk).any()
    sure, fin = ~unsure, np.isfinite(g)
    assert np.array_equal(np.isfinite(gk)[sure], fin[sure])                # eligibility, exactly
    assert (gk[sure & ~fin] == -np.inf).all()
    with np.errstate(invalid="ignore"):
        err = np.abs(gk - g)[sure & fin]
    print("D", D, "n_sets", n_sets, "gain err / bound", (err / bound[sure & fin]).max(), "largest bound", bound[sure & fin].max(),
          "n_yes err / bound", (np.abs(nk - ny)[eny > 0] / eny[eny > 0]).max())
    assert (err <= bound[sure & fin]).all()
    assert (np.abs(nk - ny) <= eny).all()
    sp = c["special"]                                                      # exact sums: exact n and exact eligibility at the threshold
    assert nk[sp["all_yes"], 0] == 18.0 and gk[sp["all_yes"], 0] == -np.inf
    assert nk[sp["at"], 0] == 8.0 and np.isfinite(gk[sp["at"], 0])
    assert nk[sp["below"], 0] == 8.0 - 2.0 ** -50 and gk[sp["below"], 0] == -np.inf
    assert nk[sp["no_at"], 0] == 13.0 and np.isfinite(gk[sp["no_at"], 0])
    for m in sp.values():
        assert np.array_equal(nk[m], ny[m])
    # the best question
    want = decided(c, g, bound, unsure)
    assert (want == -2).sum() <= 0.05 * len(want)
    for m, w in enumerate(want):
        assert bq[m] == int(np.argmax(gk[m])) if np.isfinite(gk[m]).any() else bq[m] == -1                 # the kernel's own table
        assert bg[m] == (gk[m, bq[m]] if bq[m] >= 0 else -np.inf)
        if w != -2:
            assert bq[m] == w, (m, bq[m], w)
    q2, g2 = A.tree_gains(*args, KERNEL_MIN_OCC)                           # without the tables, and a second run: the same bits
    assert torch.equal(q2, best_q) and torch.equal(g2, best_gain)
    _, _, gains3, n_yes3 = A.tree_gains(*args, KERNEL_MIN_OCC, full=True)
    assert torch.equal(gains3, gains) and torch.equal(n_yes3, n_yes)
    zero = list(args)                                                      # what the padding holds changes nothing
    zero[0] = torch.nan_to_num(args[0].clone(), nan=0.0)
    assert torch.equal(A.tree_gains(*zero, KERNEL_MIN_OCC, full=True)[2], gains)


@pytest.mark.parametrize("D,n_sets", [(3, 17), (40, 33), (160, 16)])
def test_identical_sets_tie_bit_for_bit_and_the_lower_index_wins(dev, D, n_sets):
    """A copy of a set placed elsewhere in the table (another lane, another tile, another wave) gives the same bits."""
    c = kernel_case(D, n_sets)
    base = A.tree_gains(*upload(c, dev), KERNEL_MIN_OCC, full=True)
    gb = base[2].cpu().numpy()
    for src, dst in ((0, n_sets - 1), (1, n_sets // 2), (n_sets - 1, 2)):
        member = c["member"].copy()
        member[dst] = member[src]
        q, _, gains, n_yes = A.tree_gains(*upload(dict(c, member=member), dev), KERNEL_MIN_OCC, full=True)
        gk = gains.cpu().numpy()
        for side in (0, n_sets):
            assert np.array_equal(gk[:, side + src], gk[:, side + dst]) and np.array_equal(gk[:, side + src], gb[:, side + src])
            assert torch.equal(n_yes[:, side + src], n_yes[:, side + dst])
        q = q.cpu().numpy()
        for m in range(len(gk)):
            if q[m] >= 0:
                assert q[m] == int(np.argmax(gk[m])) and q[m] % n_sets != max(src, dst)                     # the first of the largest


def test_bad_arguments(dev):
    assert A.max_tree_sets() == 1024 == _lib.load().fs2_align_max_tree_sets()
    c = kernel_case(3, 2)
    sums, left, right, offs, items, member, floor = upload(c, dev)
    good = lambda **kw: dict(dict(sums=sums, left=left, right=right, offs=offs, items=items, member=member, floor=floor, min_occ=8.0), **kw)   # noqa: E731
    A.tree_gains(**good())
    big = torch.zeros(A.max_tree_sets() + 1, member.shape[1], dtype=torch.uint8, device=dev)
    for kw in ({"min_occ": 0.5}, {"min_occ": float("nan")}, {"member": big}, {"sums": sums.float()}, {"left": left.long()},
               {"member": member.to(torch.int32)}, {"member": torch.cat([member, member], 1)[:, :member.shape[1]]},
               {"sums": torch.cat([sums, sums], 1)[:, ::2]}, {"floor": floor[:-1]}, {"left": left[:-1]}, {"offs": offs.to(torch.int64)},
               {"sums": sums[:, :-1]}):
        with pytest.raises(ValueError):
            A.tree_gains(**good(**kw))
    for name in ("sums", "left", "right", "offs", "items", "member", "floor"):
        with pytest.raises(ValueError, match="on the GPU"):
            A.tree_gains(**good(**{name: good()[name].cpu()}))
    q = torch.zeros(len(c["nodes"]), dtype=torch.int32, device=dev)
    g = torch.zeros(len(c["nodes"]), dtype=torch.float64, device=dev)
    s2 = sums.contiguous()
    call = lambda n_sets, occ: _lib.call("fs2_align_tree_gains", s2.data_ptr(), s2.stride(0), s2.shape[0], left.data_ptr(), right.data_ptr(),   # noqa: E731
                                         offs.data_ptr(), items.data_ptr(), items.shape[0], len(c["nodes"]), big.data_ptr(), n_sets,
                                         big.shape[1], floor.data_ptr(), 3, occ, q.data_ptr(), g.data_ptr(), None, None, 0, None)
    with pytest.raises(ValueError, match="question sets"):                 # the ABI itself refuses before any launch
        call(A.max_tree_sets() + 1, 8.0)
    with pytest.raises(ValueError, match="tri_min_occ"):
        call(2, 0.0)
    call(2, 8.0)
    ids = A.phone_table({"w": ["AA", "B"]})
    n = len(ids) * 2
    for kw in ({"triphones": n - 1}, {"triphones": n, "tri_min_occ": 0.5}, {"triphones": n, "tri_iters": -1}, {"triphones": n, "tri_min_gain": -1.0}):
        with pytest.raises(ValueError):
            A.Aligner(n, 160, 2, dev, phone_ids=ids, **kw)
    with pytest.raises(ValueError, match="phone_ids"):
        A.Aligner(n, 160, 2, dev, triphones=n)
    al = A.Aligner(n, 160, 2, dev, triphones=n, phone_ids=ids)
    with pytest.raises(ValueError, match="fit"):
        al.align(torch.zeros(1, 9, 160, dtype=torch.float64, device=dev), [9], [A.utterance_graph(["w"], {"w": ["AA", "B"]}, ids, 2)])


# ------------------------------------------------------------------------------------------------ the schedule
SPK = lambda i: i % 2                                                      # noqa: E731
FRONT = dict(lda=8, splice=1, lda_iters=2, fmllr=1, fmllr_rounds=1, fmllr_iters=1, fmllr_sweeps=5, fmllr_min_frames=100)
TRI = dict(triphones=E2E_LEAVES, tri_iters=E2E_TRI_ITERS, tri_min_occ=E2E_MIN_OCC)


@pytest.fixture(scope="module")
def corpus_run(dev):
    ids, graphs, xs, true, _, _ = mono(E2E_SEED, E2E_N_UTT, E2E_ITERS)
    _, utts = TC.corpus(E2E_SEED, E2E_N_UTT)
    n_classes, frames = len(ids) * C.STATES, [len(x) for x in xs]
    batches = []
    for batch in A.batches_by_bytes(frames, [len(g["sid"]) for g in graphs], 2 * C.N_MEL, 12 << 20, splice_dim=240, fmllr_dim=8):
        mel = padded([utts[i]["mel"].T for i in batch], NAN, np.float32, dev).transpose(1, 2).contiguous()
        lens = [frames[i] for i in batch]
        feats = A.features(mel, lens)
        for r, n in enumerate(lens):
            feats[r, n:] = NAN                                             # rows beyond an utterance must never be read
        batches.append((feats, lens, [graphs[i] for i in batch], batch))
    assert len(batches) >= 3
    speakers = [[SPK(i) for i in b[3]] for b in batches]

    def run(**kw):
        al = A.Aligner(n_classes, 2 * C.N_MEL, C.STATES, dev, phone_ids=ids if kw.get("triphones") else None, **kw)
        hist = al.fit([b[:3] for b in batches], E2E_ITERS, speakers if kw.get("fmllr") else None)
        got = [None] * len(utts)
        for (feats, lens, gs, batch), sp in zip(batches, speakers):
            for i, fr in zip(batch, al.align(feats, lens, gs, sp if kw.get("fmllr") else None)):
                got[i] = fr
        return al, hist, got
    return ids, graphs, xs, true, n_classes, run


def compare(al, hist, got, want, graphs):
    print("loglik per frame", hist, want["history"])
    assert len(hist) == len(want["history"])
    rel = np.abs(np.array(hist) - np.array(want["history"])) / np.abs(np.array(want["history"]))
    print("relative difference per pass", rel)
    assert (rel <= 1e-9).all()
    for key, ref in zip(("question", "yes", "no", "leaf"), want["tree"]):  # the tree, identical
        assert np.array_equal(al.tree[key], ref), key
    assert np.array_equal(al.tree["member"], want["member"]) and al.tree["n_items"] == len(want["items"])
    assert al.n_classes == want["n_leaves"] == al.tree["n_leaves"] and abs(al.tree["gain"] - want["tree"][4]) <= 1e-9 * want["tree"][4]
    mu, var = al.mu.cpu().numpy(), al.var.cpu().numpy()
    assert mu.shape == want["mu"].shape
    print("tables", np.abs(mu - want["mu"]).max() / np.abs(want["mu"]).max(), np.abs(var - want["var"]).max() / np.abs(want["var"]).max())
    assert np.abs(mu - want["mu"]).max() <= 1e-9 * np.abs(want["mu"]).max() and np.abs(var - want["var"]).max() <= 1e-9 * np.abs(want["var"]).max()
    frames = [TR.align(f, g, want) for f, g in zip(want["fs"], graphs)]
    differ = [i for i, (a, b) in enumerate(zip(got, frames)) if not np.array_equal(a, b)]
    assert not differ, differ


def test_fit_and_align_against_the_oracle_schedule(corpus_run):
    ids, graphs, xs, true, n_classes, run = corpus_run
    want = tri(E2E_SEED)
    al, hist, got = run(**TRI)
    assert len(hist) == E2E_ITERS + 1 + E2E_TRI_ITERS
    compare(al, hist, got, want, graphs)
    acc, ref = C.accuracy(true, got, 1), C.accuracy(true, [TR.align(x, g, want) for x, g in zip(xs, graphs)], 1)
    print("accuracy within one frame", acc, "oracle", ref)
    assert acc >= ref - 0.01                                               # the accuracy of tests/test_align_tri_cpu.py, on the GPU
    al2, hist2, got2 = run(**TRI)                                          # two runs: the same bits
    assert hist == hist2 and all(np.array_equal(a, b) for a, b in zip(got, got2))
    assert torch.equal(al.mu, al2.mu) and torch.equal(al.var, al2.var) and all(np.array_equal(al.tree[k], al2.tree[k]) for k in ("question", "leaf"))
    unseen = A.utterance_graph(["w00", "w01"], {"w00": ["S", "M", "AA", "S"], "w01": ["IY"]}, ids, C.STATES)    # words of no lexicon
    T = 4 * len(unseen["sid"])
    fr = al.align(torch.zeros(1, T, 2 * C.N_MEL, dtype=torch.float64, device=al.device), [T], [unseen])[0]
    assert fr.sum() == T


def test_mixtures_on_the_leaves(corpus_run):
    ids, graphs, xs, true, n_classes, run = corpus_run
    front = mono(E2E_SEED, E2E_N_UTT, E2E_ITERS)[5]
    want = TR.fit(xs, graphs, ids, C.STATES, E2E_ITERS, E2E_LEAVES, E2E_TRI_ITERS, E2E_MIN_OCC, mixtures=2, mix_iters=2, front=front)
    al, hist, got = run(mixtures=2, mix_iters=2, **TRI)
    assert len(hist) == E2E_ITERS + 1 + E2E_TRI_ITERS + 2
    compare(al, hist, got, want, graphs)
    assert np.array_equal(al.ncomp, want["ncomp"]) and al.ncomp.max() == 2 and al.gmu.shape == (E2E_LEAVES, 2, 2 * C.N_MEL)
    gmu = al.gmu.cpu().numpy()
    assert np.abs(gmu - want["gmu"]).max() <= 1e-9 * np.abs(want["gmu"]).max()


def test_behind_lda_and_fmllr(corpus_run):
    ids, graphs, xs, true, n_classes, run = corpus_run
    spk = [SPK(i) for i in range(len(xs))]
    f = FR.fit(xs, graphs, spk, n_classes, E2E_ITERS, C.N_MEL, FRONT["lda"], FRONT["splice"], FRONT["lda_iters"], FRONT["fmllr_rounds"],
               FRONT["fmllr_iters"], FRONT["fmllr_sweeps"], FRONT["fmllr_min_frames"])
    fhs, _, floor, jac = f["resume"]
    want = TR.fit(xs, graphs, ids, C.STATES, E2E_ITERS, E2E_LEAVES, E2E_TRI_ITERS, E2E_MIN_OCC,
                  front=(fhs, f["mu"], f["var"], floor, f["history"], jac))
    al, hist, got = run(**FRONT, **TRI)
    assert len(hist) == E2E_ITERS + 1 + FRONT["lda_iters"] + (1 + FRONT["fmllr_iters"]) + 1 + E2E_TRI_ITERS
    compare(al, hist, got, want, graphs)
    assert al.mu.shape == (want["n_leaves"], FRONT["lda"])


def test_triphones_zero_is_the_aligner_without_the_new_arguments(corpus_run):
    *_, run = corpus_run
    old, hist_old, got_old = run()
    new, hist_new, got_new = run(triphones=0, tri_iters=7, tri_min_occ=3, tri_min_gain=5.0)
    assert hist_old == hist_new and len(hist_old) == E2E_ITERS
    assert torch.equal(old.mu, new.mu) and torch.equal(old.var, new.var) and new.tree is None
    assert all(np.array_equal(a, b) for a, b in zip(got_old, got_new))


def test_command_line_triphones(dev, tmp_path):
    """`align.py cfg --triphones 40 --tri_min_occ 10` writes a TextGrid per utterance that the preprocessor's reader takes; a second
    run writes the same bytes; a third takes its question sets from a file."""
    root = str(tmp_path)
    lexicon_path, truth = C.wav_corpus(root, 99, 8)
    with open(os.path.join(root, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(config(root, lexicon_path), f)
    with open(os.path.join(root, "questions.txt"), "w") as f:
        f.write("first AA B CH D EH F\nsecond G IY K L M S\nedge #\n")
    cmd = [sys.executable, os.path.join(ROOT, "align.py"), os.path.join(root, "preprocess.yaml"), "--overwrite", "--triphones", "40",
           "--tri_min_occ", "10", "--tri_iters", "2"]
    tg = lambda name: os.path.join(root, "pre", "TextGrid", "spk", name + ".TextGrid")           # noqa: E731
    files = []
    for extra, n_questions in ((), 46), ((), 46), (("--questions", os.path.join(root, "questions.txt")), 6):
        run = subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        assert "8 TextGrids written, 0 utterances skipped" in run.stdout, run.stdout
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("triphones: ")]
        assert len(line) == 1 and f" {n_questions} questions, " in line[0], run.stdout
        assert 30 <= int(line[0].split(" questions, ")[1].split(" leaves")[0]) <= 40
        assert len(run.stdout.split("log-likelihood per frame: ")[1].splitlines()[0].split()) == 12 + 1 + 2
        files.append({name: open(tg(name), "rb").read() for name in truth})
        for name, segs in truth.items():
            iv = P.read_textgrid(tg(name))["phones"]
            assert iv[0][0] == 0.0 and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
            assert int(round(iv[-1][1] * C.SR / C.HOP)) == sum(d for _, d in segs) + 1
            assert [p for _, _, p in iv if p not in P.SIL_PHONES] == [p for p, _ in segs if p not in P.SIL_PHONES]
    assert files[0] == files[1]
