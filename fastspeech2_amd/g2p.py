"""Grapheme-to-phoneme conversion trained from the user's own lexicon: a joint-sequence (graphone) n-gram (Bisani & Ney 2008) over
many-to-many EM alignments (Jiampojamarn et al. 2007).  The lattices of training and the beam search of decoding run as HIP kernels
(csrc/fs2_g2p.hip); the n-gram is estimated on the host.  This docstring is the specification; tests/g2p_ref.py restates it in
plain numpy and Python loops.

Units.  Letters are the characters of the lexicon's lower-cased words, phones its phones with stress marks kept; both get ids in
sorted order.  Only the first pronunciation of a word is used (`align.read_lexicon`).  A graphone pairs a chunk of letters with a
chunk of phones; the allowed (letters, phones) shapes are the four arcs, codes 0..3: (1,0), (1,1), (1,2), (2,1).  With A letters and
P phones the type of a graphone is its index in a dense table of A NQ + A A P entries, NQ = 1 + P + P P: codes 0..2 at a NQ + q
with q = 0 | 1 + p | 1 + P + p0 P + p1, code 3 at A NQ + (a0 A + a1) P + p.  Limits come from the library (`limits()`): 64 letters,
128 phones, 32 letters and 48 phones per word, a table of at most 64 MiB; a larger alphabet is refused.  A lexicon entry is skipped
and counted, never an error, when it exceeds a word limit ("limit"), has an empty pronunciation ("empty") or has no path through
its lattice ("no_path": more phones than twice its letters).

Alignment.  Word w has the lattice of cells (i, j), i <= Lg letters and j <= Lp phones consumed; an arc of code c leaves (i, j) for
(i + dl, j + dp) when that cell exists.  theta is a multinomial over types, held as log theta in the dense table (-inf for a type
that has no count).
  E-step (`fs2_g2p_m2m_expect`).  alpha(0, 0) = 0, alpha(i, j) = lse over the arcs INTO (i, j), in code order, of alpha(source) +
  log theta(type); lse(t0..t3) = m + log(exp(t0 - m) + exp(t1 - m) + exp(t2 - m) + exp(t3 - m)), m the maximum, -inf when m is;
  an arc that does not exist contributes -inf.  beta(Lg, Lp) = 0, beta(i, j) = lse over the arcs OUT of (i, j), in code order, of
  u_c = log theta(type) + beta(target).  loglik = alpha(Lg, Lp).  The posterior of the arc of code c that leaves (i, j) is
  post[i][j][c] = exp((alpha(i, j) + u_c) - loglik), exactly 0 when the arc does not exist or loglik = -inf.
  Counts.  count[t] = the sum of the posteriors of the arcs of type t in ascending (word, i, j, code) order within a batch
  (`fs2_align_reduce` over a host-built list, one column), the batches accumulated in batch order.  The types of training are the
  distinct types of all arcs of the used entries, ascending.  Batches are `ragged.greedy_batches` under a byte budget.
  M-step (host).  theta[t] = count[t] / S, S the sum of the counts in ascending type order, one addition at a time.
  Schedule.  Flat start: one E-step with log theta = 0 for every type, then the M-step.  Then up to `iters` (8) E-steps, each
  followed by the M-step; the total log-likelihood of each is recorded; training stops early when the gain per used entry over the
  last E-step falls below `tol` (1e-5).
  Viterbi (`fs2_g2p_m2m_viterbi`).  The same lattice with max; the code of the best arc into every cell, the lowest code on ties.
  The host walks the codes back from (Lg, Lp): the word's graphone sequence.

N-gram.  Tokens: the T types that occur in the Viterbi sequences, ascending, ids 0..T-1; <s> = T, </s> = T + 1 (T < 65534).  Every
sequence is N - 1 times <s>, its graphones, </s>; an n-gram is a window of n tokens that ends at a graphone or </s>.  c_N is the
number of occurrences; for n < N, c_n(u) is the number of distinct tokens v with c_{n+1}(v u) > 0.  Per order D_n = n1 / (n1 + 2 n2)
with n1, n2 the numbers of n-grams with c_n = 1 and 2, or 0.5 when either is 0.  With c_n(h .) the sum of c_n(h w) over w and
N1+(h .) the number of such w:
    P_1(w)     = max(c_1(w) - D_1, 0) / c_1(.) + (D_1 N1+(.) / c_1(.)) / (T + 1)          over the T types and </s>
    P_n(w | h) = (c_n(h w) - D_n) / c_n(h .) + g_n(h) P_{n-1}(w | h'),   g_n(h) = D_n N1+(h .) / c_n(h .),  h' = h without its oldest token
Back-off form: order n stores, per n-gram seen, key (n ids of 16 bits packed in a uint64, the oldest highest), logp = log P_n and,
when the n-gram is the history of a seen (n+1)-gram, bow = log g_{n+1}, else 0.  Order 1 holds all T + 2 tokens (<s> with logp =
-inf); a history that is no n-gram itself (all <s>) is stored with logp = -inf.  Lookup (`fs2_g2p_ngram_score`): found at order n
-> logp; else the history's bow (0 when the history has no entry) + the lookup under h'.  The weights are added from the longest
history down, the log-probability last.  Per letter chunk the model lists the ascending token ids that spell it.

Decoding (`fs2_g2p_decode`).  Beam search, synchronous in the letter position i, no recombination.  A hypothesis is (score, last
three tokens, parent).  Position 0 holds one hypothesis of score 0 after <s> <s> <s>.  The candidates of position i are, in this
order: for every hypothesis of position i - 1 (slot ascending) every token that spells letters[i-1:i] (ascending), then for every
hypothesis of position i - 2 every token that spells letters[i-2:i]; score = parent's score + lookup.  The `beam` (64) best are
kept, ties to the earlier candidate, -inf never.  At position Lg, log P(</s> | history) is added; the best hypothesis (the lower
slot on ties) is walked back.  A word with a letter outside the model or a position nothing reaches has no pronunciation (None).

File.  `.npz` of arrays only (loaded with allow_pickle=False): letters, phones, the token table (letters and phones per token), the
n-gram (keys, logp, bow, offsets, discounts), the spelling lists, order, beam and the training summary as a JSON string.

Quality against g2p_en is unmeasured: no real pronunciation lexicon is shipped with this repository.
"""
import json
import time

import numpy as np
import torch

from . import _lib, ragged
from .align import read_lexicon

ARCS = ((1, 0), (1, 1), (1, 2), (2, 1))
SPLIT_CHARS = ",;.-?! \t\n\r\f\v+"
PAUSE_CHARS = ",;.-?!"
_WHO = "fastspeech2_amd.g2p"


def limits():
    lib = _lib.load()
    return {"letters": lib.fs2_g2p_max_letters(), "phones": lib.fs2_g2p_max_phones(), "word_letters": lib.fs2_g2p_max_word_letters(),
            "word_phones": lib.fs2_g2p_max_word_phones(), "beam": lib.fs2_g2p_max_beam(), "order": lib.fs2_g2p_max_order(),
            "table_bytes": lib.fs2_g2p_max_table_mib() << 20}


def table_size(A, P):
    return A * (1 + P + P * P) + A * A * P


# ------------------------------------------------------------------------------------------------ lexicon -> id rows
def alphabets(lexicon):
    """(letters, phones) of a {word: phones} lexicon, each sorted; refuses what the kernels' table cannot hold."""
    letters = sorted({ch for w in lexicon for ch in w.lower()})
    phones = sorted({p for ps in lexicon.values() for p in ps})
    lim = limits()
    if not letters or not phones:
        raise ValueError("the lexicon has no letters or no phones")
    if len(letters) > lim["letters"] or len(phones) > lim["phones"] or table_size(len(letters), len(phones)) * 8 > lim["table_bytes"]:
        raise ValueError(f"{len(letters)} letters and {len(phones)} phones exceed the supported {lim['letters']} and {lim['phones']} "
                         f"(a table of at most {lim['table_bytes']} bytes)")
    return letters, phones


def select_entries(lexicon):
    """-> (used [(word, phones)], skipped {"limit": n, "empty": n, "no_path": n}) in the lexicon's order."""
    lim = limits()
    used, skipped = [], {"limit": 0, "empty": 0, "no_path": 0}
    for word, pron in lexicon.items():
        word = word.lower()                                                # what the kernels see
        if len(word) > lim["word_letters"] or len(pron) > lim["word_phones"]:
            skipped["limit"] += 1
        elif not pron:
            skipped["empty"] += 1
        elif len(pron) > 2 * len(word):
            skipped["no_path"] += 1
        else:
            used.append((word, list(pron)))
    return used, skipped


def pack_ids(rows, width=None):
    """id lists -> (int32 [n][width] padded with -1, lengths int32)"""
    lens = np.array([len(r) for r in rows], np.int32)
    out = np.full((len(rows), max(int(width if width is not None else (lens.max() if len(rows) else 0)), 1)), -1, np.int32)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out, lens


def arc_types(L, Ph, gl, pl, A, P):
    """The dense type of the arc of code c that leaves cell (i, j) of every word: int64 [W][Lgmax][Lpmax + 1][4], -1 where the arc
    does not exist.  L, Ph are the padded id rows, gl, pl the lengths."""
    W, Lg, Lp = L.shape[0], int(max(gl.max(), 1)), int(pl.max())
    NQ = 1 + P + P * P
    Lx = np.concatenate([L[:, :Lg].astype(np.int64), np.full((W, 2), -1, np.int64)], axis=1)
    Px = np.concatenate([Ph[:, :Lp].astype(np.int64), np.full((W, 2), -1, np.int64)], axis=1)
    i, j = np.arange(Lg)[None, :, None], np.arange(Lp + 1)[None, None, :]
    n1, n2 = Lx[:, :Lg, None], Lx[:, 1:Lg + 1, None]
    q1, q2 = Px[:, None, :Lp + 1], Px[:, None, 1:Lp + 2]
    g, p = gl[:, None, None], pl[:, None, None]
    x0 = (i + 1 <= g) & (j <= p)
    x1, x2, x3 = x0 & (j + 1 <= p), x0 & (j + 2 <= p), (i + 2 <= g) & (j + 1 <= p)
    out = np.full((W, Lg, Lp + 1, 4), -1, np.int64)
    out[..., 0] = np.where(x0, n1 * NQ, -1)
    out[..., 1] = np.where(x1, n1 * NQ + 1 + q1, -1)
    out[..., 2] = np.where(x2, n1 * NQ + 1 + P + q1 * P + q2, -1)
    out[..., 3] = np.where(x3, A * NQ + (n1 * A + n2) * P + q1, -1)
    return out


def type_chunks(t, A, P):
    """dense type -> (letter ids, phone ids)"""
    NQ = 1 + P + P * P
    t = int(t)
    if t >= A * NQ:
        r = t - A * NQ
        return [r // P // A, r // P % A], [r % P]
    a, q = divmod(t, NQ)
    if q == 0:
        return [a], []
    if q <= P:
        return [a], [q - 1]
    return [a], [(q - 1 - P) // P, (q - 1 - P) % P]


# ------------------------------------------------------------------------------------------------ kernels
def _i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _lattice_args(letters, phones, glens, plens, logtheta, A, P):
    for t in (letters, phones, glens, plens, logtheta):
        ragged.require_device(t, _WHO)
    if letters.dtype != torch.int32 or phones.dtype != torch.int32 or letters.dim() != 2 or phones.dim() != 2 or \
            letters.stride(1) != 1 or phones.stride(1) != 1 or glens.dtype != torch.int32 or plens.dtype != torch.int32:
        raise ValueError("letters / phones must be 2-D int32 rows with unit inner stride, glens / plens int32")
    if logtheta.dtype != torch.float64 or not logtheta.is_contiguous():
        raise ValueError("logtheta must be a contiguous float64 table")
    W = letters.shape[0]
    if phones.shape[0] != W or glens.numel() != W or plens.numel() != W:
        raise ValueError("letters, phones, glens and plens must describe the same number of words")
    return W


def m2m_expect(letters, phones, glens, plens, logtheta, A, P, Lgmax, Lpmax, loglik=None, post=None):
    """-> (loglik [W], post [W][Lgmax][Lpmax + 1][4]); `loglik` / `post` may be given (nothing outside a word's cells is written)."""
    W = _lattice_args(letters, phones, glens, plens, logtheta, A, P)
    dev = letters.device
    if loglik is None:
        loglik = torch.empty(W, dtype=torch.float64, device=dev)
    if post is None:
        post = torch.zeros(W, max(Lgmax, 1), Lpmax + 1, 4, dtype=torch.float64, device=dev)
    if post.dtype != torch.float64 or not post.is_contiguous() or post.dim() != 4 or post.shape[0] != W or post.shape[3] != 4:
        raise ValueError("post must be a contiguous float64 [W][>= Lgmax][>= Lpmax + 1][4] tensor")
    _lib.call("fs2_g2p_m2m_expect", letters.data_ptr(), letters.stride(0), phones.data_ptr(), phones.stride(0), glens.data_ptr(),
              plens.data_ptr(), logtheta.data_ptr(), logtheta.numel(), A, P, loglik.data_ptr(), post.data_ptr(), post.stride(0),
              post.stride(1), W, Lgmax if post.shape[1] >= Lgmax else -1, Lpmax, torch.cuda.current_stream(dev).cuda_stream)
    return loglik, post


def m2m_viterbi(letters, phones, glens, plens, logtheta, A, P, Lgmax, Lpmax, score=None, bp=None):
    """-> (score [W], bp uint8 [W][Lgmax + 1][Lpmax + 1])"""
    W = _lattice_args(letters, phones, glens, plens, logtheta, A, P)
    dev = letters.device
    if score is None:
        score = torch.empty(W, dtype=torch.float64, device=dev)
    if bp is None:
        bp = torch.full((W, Lgmax + 1, Lpmax + 1), 255, dtype=torch.uint8, device=dev)
    if bp.dtype != torch.uint8 or not bp.is_contiguous() or bp.dim() != 3 or bp.shape[0] != W:
        raise ValueError("bp must be a contiguous uint8 [W][>= Lgmax + 1][>= Lpmax + 1] tensor")
    _lib.call("fs2_g2p_m2m_viterbi", letters.data_ptr(), letters.stride(0), phones.data_ptr(), phones.stride(0), glens.data_ptr(),
              plens.data_ptr(), logtheta.data_ptr(), logtheta.numel(), A, P, score.data_ptr(), bp.data_ptr(), bp.stride(0), bp.stride(1),
              W, Lgmax if bp.shape[1] >= Lgmax + 1 else -1, Lpmax, torch.cuda.current_stream(dev).cuda_stream)
    return score, bp


def backtrack(bp, glens, plens):
    """Host walk of the Viterbi codes from (Lg, Lp): per word the list of (i, j, code) of its arcs in order (source cell), or None
    when the end cell was not reached."""
    bp = np.asarray(bp)
    out = []
    for w in range(bp.shape[0]):
        i, j, arcs = int(glens[w]), int(plens[w]), []
        while (i, j) != (0, 0):
            c = int(bp[w, i, j])
            if c > 3:
                arcs = None
                break
            i, j = i - ARCS[c][0], j - ARCS[c][1]
            if i < 0 or j < 0:
                arcs = None
                break
            arcs.append((i, j, c))
        out.append(arcs[::-1] if arcs is not None else None)
    return out


class NGram:
    """The back-off model on the device: keys uint64 (carried as int64 bits), logp, bow, offs."""

    def __init__(self, keys, logp, bow, offs, order, device):
        self.order, self.n_keys = int(order), int(len(keys))
        self.keys = torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).to(device)
        self.logp = torch.as_tensor(np.ascontiguousarray(logp, dtype=np.float64)).to(device)
        self.bow = torch.as_tensor(np.ascontiguousarray(bow, dtype=np.float64)).to(device)
        self.offs = _i32(offs, device)
        if len(offs) != self.order + 1 or int(offs[-1]) != self.n_keys or len(logp) != self.n_keys or len(bow) != self.n_keys:
            raise ValueError("n-gram arrays do not match their offsets")
        if self.n_keys == 0:                                              # a pointer the library accepts
            self.keys, self.logp, self.bow = (torch.zeros(1, dtype=t.dtype, device=device) for t in (self.keys, self.logp, self.bow))


def ngram_score(hist, tok, lm):
    """hist int32 [n][>= N - 1] (oldest first), tok int32 [n] on the device -> log P(tok | hist) float64 [n]"""
    ragged.require_device(hist, _WHO)
    ragged.require_device(tok, _WHO)
    if hist.dtype != torch.int32 or tok.dtype != torch.int32 or hist.dim() != 2 or hist.stride(1) != 1 or not tok.is_contiguous():
        raise ValueError("hist must be int32 [n][N - 1], tok int32 [n]")
    n = tok.numel()
    out = torch.empty(n, dtype=torch.float64, device=tok.device)
    _lib.call("fs2_g2p_ngram_score", hist.data_ptr(), hist.stride(0) if hist.shape[1] >= lm.order - 1 else -1, tok.data_ptr(),
              lm.keys.data_ptr(), lm.logp.data_ptr(), lm.bow.data_ptr(), lm.offs.data_ptr(), lm.n_keys, lm.order, out.data_ptr(),
              hist.shape[0] if hist.shape[0] == n else -1, torch.cuda.current_stream(tok.device).cuda_stream)
    return out


class Speller:
    """The decoding tables on the device: per letter chunk (a | A + a0 A + a1) the ascending tokens that spell it, and the phones
    of every token."""

    def __init__(self, spell_offs, spell_types, type_phones, A, device):
        self.A, self.T = int(A), int(len(type_phones))
        offs = np.asarray(spell_offs, np.int64)
        if len(offs) != A + A * A + 1 or int(offs[-1]) != len(spell_types) or np.any(np.diff(offs) < 0):
            raise ValueError("spelling lists do not match the alphabet")
        fan = np.diff(offs)
        self.fan1, self.fan2 = int(fan[:A].max(initial=0)), int(fan[A:].max(initial=0))
        self.n_spell = int(len(spell_types))
        self.offs = _i32(offs, device)
        self.types = _i32(spell_types if len(spell_types) else [0], device)
        self.type_phones = _i32(np.asarray(type_phones).reshape(-1, 2), device)


def decode(letters, glens, speller, lm, beam, Lgmax, full=False):
    """letters int32 [W][>= Lgmax], glens int32 [W] on the device -> (phones int32 [W][2 Lgmax], n int32 [W], score float64 [W]);
    with `full` also the beams {score, hist, bp, n} the search left in its workspace."""
    ragged.require_device(letters, _WHO)
    if letters.dtype != torch.int32 or letters.dim() != 2 or letters.stride(1) != 1 or glens.dtype != torch.int32:
        raise ValueError("letters must be int32 rows with unit inner stride, glens int32")
    dev, W, K = letters.device, letters.shape[0], int(beam)
    ldc = max(K * (speller.fan1 + speller.fan2), 1)
    bs = torch.full((W, Lgmax + 1, max(K, 1)), float("nan"), dtype=torch.float64, device=dev)
    bh = torch.full((W, Lgmax + 1, max(K, 1)), -1, dtype=torch.int64, device=dev)
    bb = torch.full((W, Lgmax + 1, max(K, 1)), -1, dtype=torch.int32, device=dev)
    bn = torch.full((W, Lgmax + 1), -1, dtype=torch.int32, device=dev)
    cand = torch.empty(W, ldc, dtype=torch.float64, device=dev)
    ph = torch.full((W, max(2 * Lgmax, 1)), -1, dtype=torch.int32, device=dev)
    n = torch.empty(W, dtype=torch.int32, device=dev)
    score = torch.empty(W, dtype=torch.float64, device=dev)
    _lib.call("fs2_g2p_decode", letters.data_ptr(), letters.stride(0) if letters.shape[1] >= Lgmax else -1, glens.data_ptr(), speller.A,
              speller.offs.data_ptr(), speller.types.data_ptr(), speller.n_spell, speller.fan1, speller.fan2,
              speller.type_phones.data_ptr(), speller.T, lm.keys.data_ptr(), lm.logp.data_ptr(), lm.bow.data_ptr(), lm.offs.data_ptr(),
              lm.n_keys, lm.order, K, bs.data_ptr(), bh.data_ptr(), bb.data_ptr(), bn.data_ptr(), cand.data_ptr(), ldc, ph.data_ptr(),
              ph.stride(0), n.data_ptr(), score.data_ptr(), W if glens.numel() == W else -1, Lgmax,
              torch.cuda.current_stream(dev).cuda_stream)
    if full:
        return ph, n, score, {"score": bs, "hist": bh, "bp": bb, "n": bn}
    return ph, n, score


def decode_bytes(n, L, beam, fan):
    """device bytes of `decode` for n words padded to L letters"""
    return n * ((L + 1) * (beam * 20 + 4) + beam * fan * 8 + 2 * L * 4 + 4 * L + 16)


def batches_by_bytes(glens, plens, budget):
    """`ragged.greedy_batches` of (letters, phones) under `budget` bytes: the posteriors (32 B per cell), the host's arc list (12 B per
    arc) and the id rows."""
    cost = lambda n, Lg, Lp: n * (Lg * (Lp + 1) * (32 + 48) + (Lg + 1) * (Lp + 1) + 4 * (Lg + Lp) + 24)   # noqa: E731
    return ragged.greedy_batches(list(zip([int(v) for v in glens], [int(v) for v in plens])), budget, cost)


# ------------------------------------------------------------------------------------------------ the n-gram (host)
def _pack(cols):
    key = np.zeros(len(cols[0]), np.uint64)
    for c in cols:
        key = (key << np.uint64(16)) | c.astype(np.uint64)
    return key


def kneser_ney(seqs, T, order):
    """Token sequences (ids < T) -> dict(keys uint64, logp, bow, offs int32 [order + 1], discounts [order]) in back-off form."""
    if not 1 <= order <= limits()["order"]:
        raise ValueError(f"order must be 1..{limits()['order']}, got {order}")
    if not 1 <= T < 65534:
        raise ValueError(f"{T} graphone types: the packed keys hold 1..65533")
    N, BOS, EOS, V = order, T, T + 1, T + 1
    flat, pos = [], []
    for s in seqs:
        flat += [BOS] * (N - 1)
        pos += range(len(flat), len(flat) + len(s) + 1)
        flat += list(s) + [EOS]
    flat, pos = np.asarray(flat, np.int64), np.asarray(pos, np.int64)
    keys, counts = [None] * (N + 1), [None] * (N + 1)
    k, c = np.unique(_pack([flat[pos - (N - 1) + d] for d in range(N)]), return_counts=True)
    keys[N], counts[N] = k, c.astype(np.float64)
    for n in range(N - 1, 0, -1):                                          # distinct left extensions
        k, c = np.unique(keys[n + 1] & np.uint64((1 << (16 * n)) - 1), return_counts=True)
        keys[n], counts[n] = k, c.astype(np.float64)
    disc, logp, bow = [0.0] * (N + 1), [None] * (N + 1), [None] * (N + 1)
    prob = [None] * (N + 1)
    for n in range(1, N + 1):
        n1, n2 = int(np.sum(counts[n] == 1)), int(np.sum(counts[n] == 2))
        disc[n] = n1 / (n1 + 2.0 * n2) if n1 and n2 else 0.5
    # order 1: every token has an entry
    c1 = np.zeros(T + 2)
    c1[keys[1].astype(np.int64)] = counts[1]
    tot, n1p = float(np.cumsum(counts[1])[-1]), len(counts[1])
    p1 = np.maximum(c1 - disc[1], 0.0) / tot + (disc[1] * n1p / tot) / V
    p1[BOS] = 0.0
    keys[1], prob[1] = np.arange(T + 2, dtype=np.uint64), p1
    gammas = [None] * (N + 2)
    for n in range(2, N + 1):
        ctx = keys[n] >> np.uint64(16)
        uctx, inv = np.unique(ctx, return_inverse=True)
        tot = np.bincount(inv, weights=counts[n], minlength=len(uctx))
        n1p = np.bincount(inv, minlength=len(uctx)).astype(np.float64)
        gam = disc[n] * n1p / tot
        lower = np.searchsorted(keys[n - 1], keys[n] & np.uint64((1 << (16 * (n - 1))) - 1))
        prob[n] = (counts[n] - disc[n]) / tot[inv] + gam[inv] * prob[n - 1][lower]
        gammas[n] = (uctx, gam)
    for n in range(1, N + 1):                                              # histories: their weights, and entries for the all-<s> ones
        k, p = keys[n], prob[n]
        b = np.zeros(len(k))
        if n < N:
            uctx, gam = gammas[n + 1]
            at = np.searchsorted(k, uctx)
            have = (at < len(k)) & (k[np.minimum(at, len(k) - 1)] == uctx)
            b[at[have]] = np.log(gam[have])
            if np.any(~have):
                k = np.concatenate([k, uctx[~have]])
                p = np.concatenate([p, np.zeros(int(np.sum(~have)))])
                b = np.concatenate([b, np.log(gam[~have])])
                o = np.argsort(k, kind="stable")
                k, p, b = k[o], p[o], b[o]
                # the lower order's probabilities were looked up before this insertion: nothing refers to these rows by index
        with np.errstate(divide="ignore"):
            keys[n], logp[n], bow[n] = k, np.log(p), b
    offs = np.cumsum([0] + [len(keys[n]) for n in range(1, N + 1)]).astype(np.int32)
    return {"keys": np.concatenate(keys[1:]).astype(np.uint64), "logp": np.concatenate(logp[1:]), "bow": np.concatenate(bow[1:]),
            "offs": offs, "discounts": np.asarray(disc[1:])}


# ------------------------------------------------------------------------------------------------ scoring, text
def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def error_rates(truth, got):
    """-> (word error rate, phone error rate) of pronunciations `got` (None = no pronunciation) against `truth`"""
    wrong = sum(1 for t, g in zip(truth, got) if g is None or list(t) != list(g))
    edits = sum(edit_distance(t, g or []) for t, g in zip(truth, got))
    return wrong / max(len(truth), 1), edits / max(sum(len(t) for t in truth), 1)


def split_text(text):
    """Free text -> tokens: ("word", w) and ("pause", ch), split at , ; . - ? ! + and white space, punctuation at the end of the text
    dropped first; white space and + leave nothing."""
    from string import punctuation
    tokens, word = [], ""
    for ch in text.rstrip(punctuation) + " ":
        if ch in SPLIT_CHARS:
            if word:
                tokens.append(("word", word))
            word = ""
            if ch in PAUSE_CHARS:
                tokens.append(("pause", ch))
        else:
            word += ch
    return tokens


def text_to_phones(text, lexicon, g2p):
    """-> (braced phoneme string, tokens left out).  A word of `lexicon` (lower-cased) gets its phones, any other word `g2p.pronounce`'s,
    punctuation `sp`; a word the model cannot pronounce is left out and returned."""
    tokens = split_text(text)
    oov = sorted({w.lower() for kind, w in tokens if kind == "word" and w.lower() not in lexicon})
    said = dict(zip(oov, g2p.pronounce(oov))) if oov else {}
    phones, dropped = [], []
    for kind, w in tokens:
        if kind == "pause":
            phones.append("sp")
        elif w.lower() in lexicon:
            phones += lexicon[w.lower()]
        elif said[w.lower()] is not None:
            phones += said[w.lower()]
        else:
            dropped.append(w)
    return "{" + " ".join(phones) + "}", dropped


# ------------------------------------------------------------------------------------------------ the model
class G2P:
    def __init__(self, letters, phones, type_letters, type_phones, lm, order, beam, summary, device="cuda"):
        self.letters, self.phones = list(letters), list(phones)
        self.type_letters = np.asarray(type_letters, np.int32).reshape(-1, 2)          # -1 = none
        self.type_phones = np.asarray(type_phones, np.int32).reshape(-1, 2)
        self.lm, self.order, self.beam, self.summary = lm, int(order), int(beam), summary
        self.device = torch.device(device)
        A = len(self.letters)
        chunk = np.where(self.type_letters[:, 1] < 0, self.type_letters[:, 0], A + self.type_letters[:, 0] * A + self.type_letters[:, 1])
        o = np.argsort(chunk, kind="stable")                               # token ids stay ascending within a chunk
        self.spell_types = o.astype(np.int32)
        self.spell_offs = np.searchsorted(chunk[o], np.arange(A + A * A + 1)).astype(np.int32)
        self._dev = None

    def _tables(self):
        if self._dev is None:
            ragged.require_device(self.device, _WHO)
            self._dev = (Speller(self.spell_offs, self.spell_types, self.type_phones, len(self.letters), self.device),
                         NGram(self.lm["keys"], self.lm["logp"], self.lm["bow"], self.lm["offs"], self.order, self.device))
        return self._dev

    # ---- training
    @classmethod
    def train(cls, lexicon, order=4, iters=8, beam=64, device="cuda", holdout=0.0, seed=0, tol=1e-5, batch_bytes=1 << 30):
        dev = ragged.require_device(torch.device(device), _WHO)
        lim = limits()
        if not 1 <= beam <= lim["beam"]:
            raise ValueError(f"beam must be 1..{lim['beam']}, got {beam}")
        if not 1 <= order <= lim["order"]:
            raise ValueError(f"order must be 1..{lim['order']}, got {order}")
        if isinstance(lexicon, str):
            lexicon = read_lexicon(lexicon)
        letters, phones = alphabets(lexicon)
        A, P = len(letters), len(phones)
        used, skipped = select_entries(lexicon)
        held = []
        if holdout > 0.0:
            perm = np.random.RandomState(seed).permutation(len(used))
            out = set(perm[:int(round(holdout * len(used)))].tolist())
            held, used = [e for k, e in enumerate(used) if k in out], [e for k, e in enumerate(used) if k not in out]
        if not used:
            raise ValueError("no lexicon entry is left to train on")
        lid, pid = {c: k for k, c in enumerate(letters)}, {p: k for k, p in enumerate(phones)}
        Lrows, Prows = [[lid[c] for c in w] for w, _ in used], [[pid[p] for p in ps] for _, ps in used]
        gl, pl = [len(r) for r in Lrows], [len(r) for r in Prows]

        batches, em_types = [], []
        for idx in batches_by_bytes(gl, pl, batch_bytes):
            L, g = pack_ids([Lrows[k] for k in idx])
            Ph, p = pack_ids([Prows[k] for k in idx])
            flat = arc_types(L, Ph, g, p, A, P).ravel()
            at = np.nonzero(flat >= 0)[0]
            batches.append({"idx": idx, "L": _i32(L, dev), "Ph": _i32(Ph, dev), "g": _i32(g, dev), "p": _i32(p, dev), "gh": g, "ph": p,
                            "Lg": int(g.max()), "Lp": int(p.max()), "at": at, "types": flat[at]})
            em_types.append(np.unique(flat[at]))
        em_types = np.unique(np.concatenate(em_types))
        for b in batches:                                                  # the lists of fs2_align_reduce, once per lexicon
            comp = np.searchsorted(em_types, b.pop("types"))
            o = np.argsort(comp, kind="stable")
            b["items"] = _i32(b.pop("at")[o], dev)
            b["offs"] = _i32(np.searchsorted(comp[o], np.arange(len(em_types) + 1)), dev)

        table = torch.zeros(table_size(A, P), dtype=torch.float64, device=dev)
        em_at = torch.as_tensor(em_types).to(dev)
        counts = torch.empty(len(em_types), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def e_step():
            total = 0.0
            for n, b in enumerate(batches):
                ll, post = m2m_expect(b["L"], b["Ph"], b["g"], b["p"], table, A, P, b["Lg"], b["Lp"])
                for c0 in range(0, len(em_types), 65535):                  # the reduce kernel takes at most 65535 classes a launch
                    nc = min(65535, len(em_types) - c0)
                    _lib.call("fs2_align_reduce", post.data_ptr(), 1, post.numel(), b["offs"][c0:].data_ptr(), b["items"].data_ptr(), nc, 1,
                              counts[c0:].data_ptr(), 1 if n else 0, stream)
                total += float(np.cumsum(ll.cpu().numpy())[-1])
            return total, counts.cpu().numpy()

        def m_step(cnt):
            with np.errstate(divide="ignore"):
                logt = np.log(cnt / np.cumsum(cnt)[-1])
            table.fill_(float("-inf"))
            table[em_at] = torch.as_tensor(logt).to(dev)

        _, cnt = e_step()                                                  # flat start: every arc at weight 1
        m_step(cnt)
        history, seconds = [], []
        for _ in range(iters):
            t0 = time.perf_counter()                                       # e_step ends with a copy to the host: the device is idle
            ll, cnt = e_step()
            m_step(cnt)
            history.append(ll)
            seconds.append(time.perf_counter() - t0)
            if len(history) > 1 and (history[-1] - history[-2]) / len(used) < tol:
                break

        seqs_dense, lost = [None] * len(used), 0
        for b in batches:
            _, bp = m2m_viterbi(b["L"], b["Ph"], b["g"], b["p"], table, A, P, b["Lg"], b["Lp"])
            types = arc_types(b["L"].cpu().numpy(), b["Ph"].cpu().numpy(), b["gh"], b["ph"], A, P)
            for r, arcs in enumerate(backtrack(bp.cpu().numpy(), b["gh"], b["ph"])):
                if arcs is None:
                    lost += 1
                else:
                    seqs_dense[b["idx"][r]] = [int(types[r, i, j, c]) for i, j, c in arcs]
        skipped["no_path"] += lost
        kept = [k for k, s in enumerate(seqs_dense) if s is not None]      # indices into the used entries
        seqs_dense = [seqs_dense[k] for k in kept]
        tokens = np.unique(np.concatenate([np.asarray(s, np.int64) for s in seqs_dense]))
        if len(tokens) >= 65534:
            raise ValueError(f"{len(tokens)} graphone types: the n-gram's packed keys hold fewer than 65534")
        seqs = [np.searchsorted(tokens, np.asarray(s, np.int64)).tolist() for s in seqs_dense]
        lm = kneser_ney(seqs, len(tokens), order)
        tl, tp = np.full((len(tokens), 2), -1, np.int32), np.full((len(tokens), 2), -1, np.int32)
        for k, t in enumerate(tokens):
            ls, ps = type_chunks(t, A, P)
            tl[k, :len(ls)], tp[k, :len(ps)] = ls, ps
        summary = {"entries_used": len(seqs), "entries_held_out": len(held), "skipped": skipped, "loglik": history, "em_seconds": seconds,
                   "em_types": int(len(em_types)), "graphone_types": int(len(tokens)),
                   "ngrams": [int(v) for v in np.diff(lm["offs"])], "discounts": [float(v) for v in lm["discounts"]]}
        model = cls(letters, phones, tl, tp, lm, order, beam, summary, dev)
        model.alignments = {used[k][0]: q for k, q in zip(kept, seqs)}        # word -> its token sequence
        if held:
            got = model.pronounce([w for w, _ in held])
            wer, per = error_rates([ps for _, ps in held], got)
            summary["holdout_wer"], summary["holdout_per"] = wer, per
            model.held_out = held
        return model

    # ---- decoding
    def pronounce(self, words, beam=None, batch_bytes=1 << 30):
        """-> per word its phones, or None when the model has no pronunciation (an unknown letter, an unseen spelling, no letters,
        more letters than the kernels take)."""
        speller, lm = self._tables()
        K, cap = int(beam or self.beam), limits()["word_letters"]
        lid = {c: k for k, c in enumerate(self.letters)}
        rows = [[lid.get(c, -1) for c in w.lower()] for w in words]
        out = [None] * len(rows)
        todo = [k for k, r in enumerate(rows) if 1 <= len(r) <= cap]
        if not todo:
            return out
        cost = lambda n, L: decode_bytes(n, L, K, speller.fan1 + speller.fan2)          # noqa: E731
        for idx in ragged.greedy_batches([(len(rows[k]),) for k in todo], batch_bytes, cost):
            L, g = pack_ids([rows[todo[k]] for k in idx])
            ph, n, _ = decode(_i32(L, self.device), _i32(g, self.device), speller, lm, K, int(g.max()))
            ph, n = ph.cpu().numpy(), n.cpu().numpy()
            for r, k in enumerate(idx):
                if n[r] >= 0:
                    out[todo[k]] = [self.phones[p] for p in ph[r, :n[r]]]
        return out

    # ---- file
    def save(self, path):
        np.savez(path, letters=np.array(self.letters), phones=np.array(self.phones), type_letters=self.type_letters,
                 type_phones=self.type_phones, keys=self.lm["keys"], logp=self.lm["logp"], bow=self.lm["bow"], offs=self.lm["offs"],
                 discounts=self.lm["discounts"], spell_offs=self.spell_offs, spell_types=self.spell_types,
                 order=np.array(self.order), beam=np.array(self.beam), summary=np.array(json.dumps(self.summary)))

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            lm = {k: z[k] for k in ("keys", "logp", "bow", "offs", "discounts")}
            return cls([str(c) for c in z["letters"]], [str(p) for p in z["phones"]], z["type_letters"], z["type_phones"], lm,
                       int(z["order"]), int(z["beam"]), json.loads(str(z["summary"])), device)
