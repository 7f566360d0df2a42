"""float64 numpy oracle of the phone-loop recogniser, written from the specification in fastspeech2_amd/recognize.py's docstring (not
from the kernel or the product's host code): the Viterbi recurrence over a free loop of P phones of S states with its backtrack,
one utterance at a time with a plain loop over frames (vector operations over the states; `argmax` returns the first of the
largest, which is the rule "strictly larger replaces" over ascending p); the bigram counts; the edit distance with its operation list."""
import numpy as np

NINF = -np.inf


def loop_viterbi(E, self_, next_, link, init, final_, P, S):
    """E (T, >= P S); costs as the specification names them -> (bp uint8 (T, P S), end state or -1, score).  Candidates are taken in
    code order, 0 self, 1 next, 2 + p entry from phone p; a later one wins only when strictly larger."""
    T, C = E.shape[0], P * S
    bp = np.zeros((T, C), np.uint8)
    if T == 0:
        return bp, -1, NINF
    self_, next_, link = np.asarray(self_, np.float64), np.asarray(next_, np.float64), np.asarray(link, np.float64)[:P, :P]
    first = np.arange(P) * S
    last, inner = first + S - 1, np.arange(C) % S > 0
    d = np.full(C, NINF)
    d[first] = np.asarray(init, np.float64) + E[0, first]
    for t in range(1, T):
        best, code = d + self_, np.zeros(C, np.int64)
        nxt = np.full(C, NINF)
        nxt[inner] = d[np.nonzero(inner)[0] - 1] + next_[inner]
        better = nxt > best
        best, code = np.where(better, nxt, best), np.where(better, 1, code)
        enter = d[last][:, None] + link                                    # [p, q]
        arg = np.argmax(enter, axis=0)                                     # the first of the largest: the lowest p
        val = enter[arg, np.arange(P)]
        better = val > best[first]
        best[first], code[first] = np.where(better, val, best[first]), np.where(better, 2 + arg, code[first])
        d, bp[t] = E[t, :C] + best, code
    end, score = -1, NINF
    for p in range(P):
        v = d[p * S + S - 1] + final_[p]
        if v > score:
            end, score = p * S + S - 1, v
    return bp, end, score


def loop_backtrack(bp, end, P, S):
    """-> [(phone, first frame)] in time order; [] when there is no path (end < 0 or T = 0); None when the chain leaves the table."""
    T, C = bp.shape[0], P * S
    if T == 0 or end < 0:
        return []
    if end >= C:
        return None
    segs, j = [], int(end)
    for t in range(T - 1, 0, -1):
        code, s = int(bp[t, j]), j % S
        if code == 1:
            if s == 0:
                return None
            j -= 1
        elif code >= 2:
            if s != 0 or code - 2 >= P:
                return None
            segs.append((j // S, t))
            j = (code - 2) * S + S - 1
    segs.append((j // S, 0))
    return segs[::-1]


def decode(E, self_, next_, link, init, final_, P, S):
    """-> ([(phone, first frame, frames)], score)"""
    bp, end, score = loop_viterbi(E, self_, next_, link, init, final_, P, S)
    segs = loop_backtrack(bp, end, P, S)
    starts = [t for _, t in segs] + [E.shape[0]]
    return [(p, a, b - a) for (p, a), b in zip(segs, starts[1:])], score


def phone_bigram(sequences, P, smoothing=0.5):
    """-> (counts (P + 1, P + 1), log-probabilities): row P is the start, column P the end; a row's probabilities are (count +
    smoothing) over their row sum.  The start row has no arc to the end (an empty utterance is not a sequence): -inf there."""
    counts = np.zeros((P + 1, P + 1))
    for seq in sequences:
        if len(seq) == 0:
            continue
        prev = P
        for p in seq:
            counts[prev, p] += 1.0
            prev = p
        counts[prev, P] += 1.0
    sm = counts + smoothing
    sm[P, P] = 0.0
    with np.errstate(divide="ignore"):
        return counts, np.log(sm / sm.sum(axis=1, keepdims=True))


def edit_counts(ref, hyp):
    """Levenshtein with unit costs -> ((hits, sub, del, ins), ops): ops lists ("hit" | "sub" | "del" | "ins", ref index or None, hyp
    index or None) in sequence order; walking back from the end the backtrace prefers the diagonal, then the deletion, then the
    insertion."""
    n, m = len(ref), len(hyp)
    D = np.zeros((n + 1, m + 1), np.int64)
    D[:, 0], D[0, :] = np.arange(n + 1), np.arange(m + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = min(D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    ops, i, j = [], n, m
    while i or j:
        if i and j and D[i, j] == D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]):
            ops.append(("hit" if ref[i - 1] == hyp[j - 1] else "sub", i - 1, j - 1))
            i, j = i - 1, j - 1
        elif i and D[i, j] == D[i - 1, j] + 1:
            ops.append(("del", i - 1, None))
            i -= 1
        else:
            ops.append(("ins", None, j - 1))
            j -= 1
    ops.reverse()
    c = [sum(1 for o in ops if o[0] == k) for k in ("hit", "sub", "del", "ins")]
    return tuple(c), ops
