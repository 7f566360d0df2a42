"""Phone-loop recognition on the forced aligner's acoustic model: the phone sequence the model hears in an utterance, and its phone
error rate (PER) against the phones the synthesizer was asked to say.  `score.py` measures spectrum, pitch, energy and durations;
this measures whether the phones are there: intelligibility, not naturalness.  The acoustic model is the one `align.py --save_model`
trains on the recorded corpus (fastspeech2_amd/align.py); the decoder is a Viterbi pass over a free loop of all phones, a HIP kernel
(csrc/fs2_align_loop.hip) on the per-utterance scan of the forced Viterbi.  The specification below is what the kernel and the
numpy oracle (tests/align_loop_ref.py) implement.

Layout.  The model has P phones (the phone table in id order, `sil`, `sp` and `spn` included) of S states; state j = p S + s is
emission class j, C = P S <= `align.max_states()` (1024), P <= `max_loop_phones()` (253: a backpointer is one byte).  E[t, j], float64,
comes from the aligner's own emission kernels (`align.emit` / `align.emit_gmm`) called with sid = 0 .. C - 1, after the model's LDA
projection when it has one.

Costs, float64, each finite or -inf:  self_ (C,);  next_ (C,), the arc s - 1 -> s, unused at s = 0;  link (P, P), link[p, q] the
cost of leaving the last state of p and entering the first state of q;  init (P,);  final_ (P,).

Recurrence.  d[0, q S] = init[q] + E[0, q S], every other state -inf.  d[t, j] = E[t, j] + best, best the maximum over the candidates
taken in code order: code 0, d[t-1, j] + self_[j]; for s > 0 code 1, d[t-1, j-1] + next_[j]; for s = 0 code 2 + p, d[t-1, p S + S - 1] +
link[p, q] for p = 0 .. P - 1.  A later candidate replaces an earlier one only when strictly larger.  With S = 1 a state is both the
first and the last state of its phone.  End: the maximum over p ascending of d[T-1, p S + S - 1] + final_[p], strictly larger
replaces; `end` is that state, `score` that value; when the maximum is -inf (T < S, or everything forbidden) end = -1, score = -inf
and there are no segments.  Only adds and compares of float64 operands: kernel and oracle agree bit for bit.
Backtrack.  From `end` along the backpointers; frame 0 and every frame entered with a code >= 2 start a segment; the segments
(phone, first frame) come in time order, at most T of them.  A chain that leaves the table (a state outside [0, C), code 1 at a
first state, an entry code elsewhere or from a phone >= P) gives n_seg = -1.

Language model (host, numpy).  `phone_bigram(sequences, P, smoothing)`: counts (P + 1, P + 1), row P the start and column P the end
of a sequence (an empty sequence counts nothing); log-probabilities log((count + smoothing) / row sum), where the start row has
no arc to the end (-inf).  `align.build(save_model=...)` stores the counts of the training corpus's decoded alignments, a sequence
being the blocks with frames > 0, so the realised `sil` / `sp` are part of it.
`Recognizer(aligner, phone_names, bigram, lm, lm_scale, penalty)`:  with lm = "bigram" link[p, q] = lm_scale log P(q | p) + penalty,
init[q] = lm_scale log P(q | start), final_[p] = lm_scale log P(end | p); with `transitions` link[p, q] and final_[p] also take
log(1 - loop) of p's last state, the cost of leaving it.  With lm = "none" link, init and final_ are 0.  self_[j] = log loop[j] and
next_[j] = log(1 - loop[j - 1]) when the model has transitions, else 0.  lm_scale = 8 and penalty = 0 are choices, not
measurements: the scale only has to bring a bigram's few nats per phone into the range of an 80- or 40-dimensional Gaussian's
score per frame.  Models with `triphones` (a context-dependent loop) or `fmllr` (unsupervised speaker transforms) are refused.

Score (host, numpy).  `edit_counts(ref, hyp)`: Levenshtein with unit costs -> (hits, sub, del, ins) and the operation list; the
backtrace prefers the diagonal, then the deletion, then the insertion.  `sil`, `sp` and `spn` are dropped from both sides first.
PER = (sub + del + ins) / n_ref; the corpus PER is the sum of the errors over the sum of n_ref.

What is claimed.  The recurrence, pinned to its numpy restatement and to brute-force enumeration of all paths; on the synthetic
corpus of the tests the PER of the oracle pipeline is recorded in tests/golden/align_loop_bars.json.  No PER has been measured on
real speech.  A monophone-GMM recogniser has a high absolute PER on read speech: only the difference between the recorded and
the synthesized side under one model and one setting means anything.  There is no agreement with any ASR system, and no timing
measured yet."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, align as A, ops, ragged

SILENT = (A.SIL, A.SP, A.SPN)
SUMMARY_TOP = 10


# ------------------------------------------------------------------------------------------------ kernels
def max_loop_phones():
    return _lib.load().fs2_align_max_loop_phones()


def _cost(v, shape, what, device):
    A._no_host(**{what: v})
    v = A._dev(v, torch.float64, what, len(shape))
    if tuple(v.shape) != tuple(shape) or v.device != device:
        raise ValueError(f"{what} {tuple(v.shape)} is not {tuple(shape)} on {device}")
    return v


def _loop_shape(P, S):
    P, S = int(P), int(S)
    if not 1 <= P <= max_loop_phones() or not 1 <= S <= 3 or P * S > A.max_states():
        raise ValueError(f"{P} phones of {S} states, supported are 1..{max_loop_phones()} phones of 1..3 states and at most "
                         f"{A.max_states()} states")
    return P, S


def loop_viterbi(E, lens, self_, next_, link, init, final_, P, S, out=None):
    """The recurrence of the module docstring on E (B, Tmax, >= P S) float64 -> (backpointers uint8 (B, Tmax, >= P S), end (B,)
    int32, score (B,) float64) on the device.  link may be a view of a wider table (row stride >= P); `out` may be a strided
    view for the backpointers; nothing at t >= lens[b] or j >= P S is read or written."""
    A._no_host(E=E, out=out)
    P, S = _loop_shape(P, S)
    C = P * S
    E = A._dev(E, torch.float64, "E")
    B, Tmax, W = E.shape
    if W < C:
        raise ValueError(f"E {tuple(E.shape)} does not hold {C} states")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", E.device)
    self_, next_ = _cost(self_, (C,), "self_", E.device).contiguous(), _cost(next_, (C,), "next_", E.device).contiguous()
    init, final_ = _cost(init, (P,), "init", E.device).contiguous(), _cost(final_, (P,), "final_", E.device).contiguous()
    link = _cost(link, (P, P), "link", E.device)
    bp = A._out(out, (B, Tmax, C), E.device, least=(2,), dtype=torch.uint8)
    end = torch.empty(B, dtype=torch.int32, device=E.device)
    score = torch.empty(B, dtype=torch.float64, device=E.device)
    _lib.call("fs2_align_loop_viterbi", E.data_ptr(), E.stride(0), E.stride(1), lens_d.data_ptr(), self_.data_ptr(), next_.data_ptr(),
              link.data_ptr(), max(link.stride(0), P), init.data_ptr(), final_.data_ptr(), bp.data_ptr(), bp.stride(0), bp.stride(1),
              end.data_ptr(), score.data_ptr(), B, Tmax, P, S, ops._stream())
    return bp, end, score


def loop_backtrack(bp, lens, end, P, S, out=None):
    """-> (seg_phone, seg_start int32 (B, >= Tmax), n_seg int32 (B,)) on the device: the segments of the best path in time order.
    `out` = (seg_phone, seg_start) may give the buffers (the same strides); nothing at k >= n_seg[b] is written (fresh buffers hold
    -1 there)."""
    A._no_host(bp=bp, end=end)
    P, S = _loop_shape(P, S)
    bp = A._dev(bp, torch.uint8, "bp")
    B, Tmax, W = bp.shape
    if W < P * S:
        raise ValueError(f"bp {tuple(bp.shape)} does not hold {P * S} states")
    _, lens_d = ragged.lengths(lens, B, Tmax, "lens", bp.device)
    end = A._dev(end, torch.int32, "end", 1)
    if end.shape[0] != B:
        raise ValueError(f"end holds {end.shape[0]} values for {B} utterances")
    if out is None:
        both = torch.full((2, B, max(Tmax, 1)), -1, dtype=torch.int32, device=bp.device)
        phone, start = both[0], both[1]
    else:
        A._no_host(seg_phone=out[0], seg_start=out[1])
        phone, start = A._dev(out[0], torch.int32, "seg_phone", 2), A._dev(out[1], torch.int32, "seg_start", 2)
        if phone.shape[0] != B or phone.shape[1] < Tmax or phone.shape != start.shape or phone.stride() != start.stride():
            raise ValueError(f"out must be twice ({B}, >= {Tmax}) int32 with the same strides")
    n_seg = torch.empty(B, dtype=torch.int32, device=bp.device)
    _lib.call("fs2_align_loop_backtrack", bp.data_ptr(), bp.stride(0), bp.stride(1), lens_d.data_ptr(), end.data_ptr(), phone.data_ptr(),
              start.data_ptr(), phone.stride(0), n_seg.data_ptr(), B, Tmax, P, S, ops._stream())
    return phone, start, n_seg


# ------------------------------------------------------------------------------------------------ language model, edit distance
def phone_bigram(sequences, P, smoothing=0.5):
    """The bigram of the module docstring over sequences of phone ids < P -> (counts, log-probabilities), both (P + 1, P + 1)."""
    counts = np.zeros((P + 1, P + 1))
    for seq in sequences:
        seq = np.asarray(seq, np.int64).reshape(-1)
        if seq.size == 0:
            continue
        if seq.min() < 0 or seq.max() >= P:
            raise ValueError(f"phone id outside [0, {P})")
        np.add.at(counts, (np.concatenate([[P], seq]), np.concatenate([seq, [P]])), 1.0)
    return counts, bigram_logprob(counts, smoothing)


def bigram_logprob(counts, smoothing=0.5):
    """log((count + smoothing) / row sum); the start row has no arc to the end."""
    counts = np.asarray(counts, np.float64)
    if counts.ndim != 2 or counts.shape[0] != counts.shape[1] or counts.shape[0] < 2 or not smoothing > 0:
        raise ValueError(f"counts {counts.shape} must be (P + 1, P + 1) and smoothing positive")
    sm = counts + smoothing
    sm[-1, -1] = 0.0
    with np.errstate(divide="ignore"):
        return np.log(sm / sm.sum(axis=1, keepdims=True))


def edit_counts(ref, hyp):
    """Levenshtein with unit costs -> ((hits, sub, del, ins), ops); ops = [(kind, ref index or None, hyp index or None)] in sequence
    order, kind one of "hit", "sub", "del", "ins".  The backtrace prefers the diagonal, then the deletion, then the insertion."""
    ref, hyp = list(ref), list(hyp)
    n, m = len(ref), len(hyp)
    differ = np.array([[r != h for h in hyp] for r in ref], np.int64).reshape(n, m)
    D = np.zeros((n + 1, m + 1), np.int64)
    D[:, 0], D[0, :] = np.arange(n + 1), np.arange(m + 1)
    for i in range(1, n + 1):
        row, up = D[i], D[i - 1]
        for j in range(1, m + 1):
            row[j] = min(up[j - 1] + differ[i - 1, j - 1], up[j] + 1, row[j - 1] + 1)
    ops_, i, j = [], n, m
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + differ[i - 1, j - 1]:
            ops_.append(("sub" if differ[i - 1, j - 1] else "hit", i - 1, j - 1))
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            ops_.append(("del", i - 1, None))
            i -= 1
        else:
            ops_.append(("ins", None, j - 1))
            j -= 1
    ops_.reverse()
    kinds = [o[0] for o in ops_]
    return tuple(kinds.count(k) for k in ("hit", "sub", "del", "ins")), ops_


# ------------------------------------------------------------------------------------------------ the recogniser
class _LoopGraphs:
    """What `align.emit` takes of a batch's graphs when every utterance has the states 0 .. C - 1: sid = the class of every state."""

    def __init__(self, B, C, device):
        self.jl, self.Jmax, self.ldg = [C] * B, C, C
        self.sid = torch.arange(C, dtype=torch.int32, device=device).repeat(B, 1)
        self.jlens = torch.full((B,), C, dtype=torch.int32, device=device)


class Recognizer:
    """The phone loop over a trained `align.Aligner` (monophone; single Gaussians or mixtures, with or without LDA and
    transitions).  `phone_names`: the phone table in id order; `bigram`: the counts (P + 1, P + 1) `phone_bigram` returns (needed
    with lm = "bigram")."""

    def __init__(self, aligner, phone_names, bigram=None, lm="bigram", lm_scale=8.0, penalty=0.0, smoothing=0.5):
        for option in ("triphones", "fmllr"):
            if getattr(aligner, option):
                raise ValueError(f"the phone loop does not take a model trained with {option}")
        if lm not in ("bigram", "none"):
            raise ValueError(f"lm must be 'bigram' or 'none', got {lm}")
        self.aligner, self.names = aligner, list(phone_names)
        self.P, self.S = _loop_shape(len(self.names), aligner.states)
        P, S, C = self.P, self.S, self.P * self.S
        if C != aligner.n_classes:
            raise ValueError(f"{P} phones of {S} states are not the model's {aligner.n_classes} classes")
        self.self_, self.next_ = np.zeros(C), np.zeros(C)
        leave = np.zeros(P)
        if aligner.transitions:
            loop = np.asarray(aligner.loop, np.float64)
            self.self_ = np.log(loop)
            self.next_[1:] = np.log(1.0 - loop[:-1])
            self.next_[::S] = 0.0                                          # unused at s = 0
            leave = np.log(1.0 - loop[S - 1::S])
        if lm == "none":
            self.link, self.init, self.final_ = np.zeros((P, P)), np.zeros(P), np.zeros(P)
        else:
            if bigram is None or np.asarray(bigram).shape != (P + 1, P + 1):
                raise ValueError(f"lm = 'bigram' needs the ({P + 1}, {P + 1}) bigram counts of the model")
            logp = bigram_logprob(bigram, smoothing)
            self.link = float(lm_scale) * logp[:P, :P] + float(penalty) + leave[:, None]
            self.init = float(lm_scale) * logp[P, :P]
            self.final_ = float(lm_scale) * logp[:P, P] + leave
        dev = aligner.device
        self._dev = tuple(A._up(v, dev) for v in (self.self_, self.next_, self.link, self.init, self.final_))

    def emissions(self, feats, lens):
        """E (B, Tmax, C) of feats (B, Tmax, the model's input dimension) float64, through the model's LDA when it has one."""
        al = self.aligner
        if feats.dim() != 3 or feats.shape[2] != al.dim or feats.dtype != torch.float64:
            raise ValueError(f"feats must be (B, Tmax, {al.dim}) float64, got {feats.dtype} {tuple(feats.shape)}")
        lens = ragged.lengths(lens, feats.shape[0], feats.shape[1], "lens")
        x = feats.to(al.device, non_blocking=True)
        if al.lda:
            if al.P is None:
                raise ValueError("an Aligner with lda has no transform before `fit`")
            x = al._project(x, lens)
        G = _LoopGraphs(x.shape[0], self.P * self.S, al.device)
        E = A.emit(x, lens, G, al.mu, al.var) if al.mixtures == 1 else A.emit_gmm(x, lens, G, al.gw, al.gmu, al.gvar)
        return E, lens

    def decode(self, feats, lens):
        """-> ([[(phone id, first frame, frames)] per utterance], [score per utterance])"""
        E, lens = self.emissions(feats, lens)
        bp, end, score = loop_viterbi(E, lens, *self._dev, self.P, self.S)
        phone, start, n_seg = (v.cpu().numpy() for v in loop_backtrack(bp, lens, end, self.P, self.S))
        out = []
        for b, T in enumerate(lens):
            n = int(n_seg[b])
            if n < 0:
                raise RuntimeError(f"the backpointers of utterance {b} are not a path of the loop")
            edges = np.concatenate([start[b, :n], [T]])
            out.append([(int(p), int(a), int(z - a)) for p, a, z in zip(phone[b, :n], edges[:-1], edges[1:])])
        return out, [float(v) for v in score.cpu().numpy()]


# ------------------------------------------------------------------------------------------------ the corpus pass
def feature_config(config):
    """The settings of a preprocess config the acoustic features depend on (stored in a model file, compared on load)."""
    pp = config["preprocessing"]
    return {"sampling_rate": pp["audio"]["sampling_rate"], "filter_length": pp["stft"]["filter_length"],
            "hop_length": pp["stft"]["hop_length"], "win_length": pp["stft"]["win_length"], "n_mel": pp["mel"]["n_mel_channels"],
            "fmin": pp["mel"]["mel_fmin"], "fmax": pp["mel"]["mel_fmax"]}


def read_source(source):
    """`basename|speaker|{phones}|...` lines -> [(basename, [phones])]; a line without a `{...}` field is a ValueError."""
    out = []
    with open(source, encoding="utf-8") as f:
        for no, ln in enumerate(f, 1):
            if not ln.strip():
                continue
            parts = ln.strip("\n").split("|")
            field = [p for p in parts[1:] if p.startswith("{") and p.endswith("}")]
            if not field:
                raise ValueError(f"{source}:{no}: no {{...}} phone field")
            out.append((parts[0], field[0][1:-1].split()))
    return out


def summarize(rows, missing, setting):
    """The corpus line: PER = the sum of the errors over the sum of n_ref, the counts, the most frequent substitutions, the most
    deleted and the most inserted phones."""
    tot = {k: sum(r[k] for r in rows) for k in ("n_ref", "hits", "sub", "del", "ins")}
    pairs, dels, inss = {}, {}, {}
    for r in rows:
        for kind, a, b in r["_ops"]:
            if kind == "sub":
                pairs[a, b] = pairs.get((a, b), 0) + 1
            elif kind == "del":
                dels[a] = dels.get(a, 0) + 1
            elif kind == "ins":
                inss[b] = inss.get(b, 0) + 1
    top = lambda d: sorted(d.items(), key=lambda kv: (-kv[1], kv[0]))[:SUMMARY_TOP]            # noqa: E731
    return {"utterances": len(rows), "missing": len(missing), **tot,
            "per": (tot["sub"] + tot["del"] + tot["ins"]) / tot["n_ref"] if tot["n_ref"] else None,
            "substitutions": [[a, b, c] for (a, b), c in top(pairs)], "deleted": [[a, c] for a, c in top(dels)],
            "inserted": [[a, c] for a, c in top(inss)], **setting}


def run(model_path, config, source, wav_dir, lm="bigram", lm_scale=8.0, penalty=0.0, out_path=None, device="cuda", batch_bytes=2 << 30,
        batch_seconds=1800.0, num_workers=8):
    """Decode `{wav_dir}/{basename}.wav` for every line of `source` with the model file `model_path` and score the phones against
    the line's `{...}` field -> (rows, missing, summary).  The wavs go through the wav -> mel -> `align.features` path of
    `align.build`, in ragged batches under a byte budget.  `rows` are the JSON objects written to `out_path`."""
    from . import audio as Audio
    from .preprocess import load_wav
    dev = ragged.require_device(torch.device(device), "fastspeech2_amd.recognize")
    al = A.Aligner.load(model_path, dev)
    fc = feature_config(config)
    if fc != al.feature_config:
        diff = ", ".join(f"{k} {fc[k]} (model: {al.feature_config.get(k)})" for k in fc if fc[k] != al.feature_config.get(k))
        raise ValueError(f"the config's feature settings are not the model's: {diff}")
    rec = Recognizer(al, al.phone_names, al.bigram, lm, lm_scale, penalty)
    sr, hop, n_mel = fc["sampling_rate"], fc["hop_length"], fc["n_mel"]
    stft = Audio.TacotronSTFT(fc["filter_length"], hop, fc["win_length"], n_mel, sr, fc["fmin"], fc["fmax"])
    entries, missing = [], []
    for name, phones in read_source(source):
        path = os.path.join(wav_dir, name + ".wav")
        (entries if os.path.exists(path) else missing).append((name, phones, path))
    missing = [(name, "missing " + path) for name, _, path in missing]

    def read(e):
        return np.clip(load_wav(e[2], sr), -1.0, 1.0).astype(np.float32)
    with ThreadPoolExecutor(max_workers=max(1, num_workers)) as pool:
        wavs = list(pool.map(read, entries))
    short = [i for i, w in enumerate(wavs) if len(w) <= fc["filter_length"] // 2]
    missing += [(entries[i][0], f"{len(wavs[i])} samples are too few") for i in short]
    keep = [i for i in range(len(entries)) if i not in set(short)]
    entries, wavs = [entries[i] for i in keep], [wavs[i] for i in keep]

    staging, xs = ragged.Staging(), [None] * len(entries)
    for batch in ragged.greedy_batches([(len(w),) for w in wavs], int(batch_seconds * sr), ragged.padded_samples):
        staging.pack([wavs[i] for i in batch])
        mel, _, fr = stft.mel_spectrogram_ragged(staging.to(dev), [len(wavs[i]) for i in batch])
        x = A.features(mel.contiguous(), fr.tolist()).cpu()
        for r, i in enumerate(batch):
            xs[i] = x[r, :int(fr[r])].clone()

    C, D = rec.P * rec.S, 2 * n_mel
    cost = lambda n, T: n * T * (C * 9 + (D + al.splice_dim + al.lda) * 8 + 8)                  # noqa: E731  E, bp, features, segments
    rows = [None] * len(entries)
    drop = {i for i, p in enumerate(rec.names) if p in SILENT}
    for batch in ragged.greedy_batches([(x.shape[0],) for x in xs], batch_bytes, cost):
        lens = [xs[i].shape[0] for i in batch]
        feats = torch.zeros(len(batch), max(lens), D, dtype=torch.float64)
        for r, i in enumerate(batch):
            feats[r, :lens[r]] = xs[i]
        segs, scores = rec.decode(feats, lens)
        for i, T, seg, sc in zip(batch, lens, segs, scores):
            name, ref, _ = entries[i]
            ref = [p for p in ref if p not in SILENT]
            hyp = [rec.names[p] for p, _, _ in seg if p not in drop]
            (hits, sub, dele, ins), ops_ = edit_counts(ref, hyp)
            rows[i] = {"basename": name, "n_ref": len(ref), "hits": hits, "sub": sub, "del": dele, "ins": ins,
                       "per": (sub + dele + ins) / len(ref) if ref else None, "score_per_frame": sc / T if np.isfinite(sc) else None,
                       "hyp": [[rec.names[p], a * hop / sr, (a + n) * hop / sr] for p, a, n in seg],
                       "_ops": [(k, ref[a] if a is not None else None, hyp[b] if b is not None else None) for k, a, b in ops_]}
    summary = summarize(rows, missing, {"lm": lm, "lm_scale": lm_scale, "penalty": penalty})
    for r in rows:
        del r["_ops"]
    if out_path is not None:
        with open(out_path, "w", encoding="utf-8") as f:
            for r in rows:
                f.write(json.dumps(r, allow_nan=False) + "\n")
    return rows, missing, summary
