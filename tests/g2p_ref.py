"""float64 oracle of the grapheme-to-phoneme model, written from the specification in fastspeech2_amd/g2p.py's docstring (not from
the kernels): the lattice recursions, the EM schedule, the Kneser-Ney estimate, the back-off lookup, the beam search and a brute-force
decoder, one word at a time with plain loops.  Words are lists of letter ids, pronunciations lists of phone ids."""
import math
from collections import defaultdict

import numpy as np

NINF = -math.inf
ARCS = ((1, 0), (1, 1), (1, 2), (2, 1))


def table_size(A, P):
    return A * (1 + P + P * P) + A * A * P


def arc_type(c, ls, ps, A, P):
    """dense type of the arc of code c over the letter ids ls and phone ids ps; -1 when an id is outside the alphabets"""
    if any(not 0 <= a < A for a in ls) or any(not 0 <= p < P for p in ps):
        return -1
    NQ = 1 + P + P * P
    if c == 3:
        return A * NQ + (ls[0] * A + ls[1]) * P + ps[0]
    return ls[0] * NQ + (0 if c == 0 else 1 + ps[0] if c == 1 else 1 + P + ps[0] * P + ps[1])


def lse(ts):
    m = max(ts)
    if m == NINF:
        return NINF
    acc = 0.0
    for t in ts:                                                           # left to right, one addition at a time
        acc = acc + math.exp(t - m)
    return m + math.log(acc)


def out_arcs(L, Ph, i, j, table, A, P):
    """per code (exists, log theta, type) of the arcs that leave (i, j)"""
    res = []
    for c, (dl, dp) in enumerate(ARCS):
        if i + dl <= len(L) and j + dp <= len(Ph):
            t = arc_type(c, L[i:i + dl], Ph[j:j + dp], A, P)
            res.append((True, table[t] if t >= 0 else NINF, t))
        else:
            res.append((False, NINF, -1))
    return res


def expect(L, Ph, table, A, P):
    """-> (loglik, post [Lg][Lp + 1][4])"""
    Lg, Lp = len(L), len(Ph)
    alpha = np.full((Lg + 1, Lp + 1), NINF)
    for s in range(Lg + Lp + 1):
        for i in range(max(0, s - Lp), min(Lg, s) + 1):
            j = s - i
            if s == 0:
                alpha[0, 0] = 0.0
                continue
            ts = []
            for c, (dl, dp) in enumerate(ARCS):
                if i - dl >= 0 and j - dp >= 0:
                    ts.append(alpha[i - dl, j - dp] + out_arcs(L, Ph, i - dl, j - dp, table, A, P)[c][1])
                else:
                    ts.append(NINF)
            alpha[i, j] = lse(ts)
    ll = alpha[Lg, Lp]
    beta = np.full((Lg + 1, Lp + 1), NINF)
    post = np.zeros((Lg, Lp + 1, 4))
    for s in range(Lg + Lp, -1, -1):
        for i in range(max(0, s - Lp), min(Lg, s) + 1):
            j = s - i
            arcs = out_arcs(L, Ph, i, j, table, A, P)
            us = [lt + beta[i + ARCS[c][0], j + ARCS[c][1]] if ex else NINF for c, (ex, lt, _) in enumerate(arcs)]
            beta[i, j] = 0.0 if (i, j) == (Lg, Lp) else lse(us)
            if i < Lg and ll != NINF:
                for c in range(4):
                    if arcs[c][0]:
                        post[i, j, c] = math.exp((alpha[i, j] + us[c]) - ll)
    return ll, post


def viterbi(L, Ph, table, A, P):
    """-> (score, bp [Lg + 1][Lp + 1] with 255 for no arc, arcs [(i, j, code)] or None, the smallest gap between the best and the
    second best arc into a cell of the path)"""
    Lg, Lp = len(L), len(Ph)
    best = np.full((Lg + 1, Lp + 1), NINF)
    bp = np.full((Lg + 1, Lp + 1), 255, np.int64)
    gaps = np.full((Lg + 1, Lp + 1), math.inf)
    best[0, 0] = 0.0
    for s in range(1, Lg + Lp + 1):
        for i in range(max(0, s - Lp), min(Lg, s) + 1):
            j = s - i
            cs = []
            for c, (dl, dp) in enumerate(ARCS):
                ok = i - dl >= 0 and j - dp >= 0
                cs.append(best[i - dl, j - dp] + out_arcs(L, Ph, i - dl, j - dp, table, A, P)[c][1] if ok else NINF)
            v, code = cs[0], 0
            for c in (1, 2, 3):
                if cs[c] > v:
                    v, code = cs[c], c
            if v != NINF:
                best[i, j], bp[i, j] = v, code
                rest = [x for c, x in enumerate(cs) if c != code]
                gaps[i, j] = v - max(rest)
    if best[Lg, Lp] == NINF:
        return NINF, bp, None, math.inf
    i, j, arcs, gap = Lg, Lp, [], math.inf
    while (i, j) != (0, 0):
        c = int(bp[i, j])
        gap = min(gap, gaps[i, j])
        i, j = i - ARCS[c][0], j - ARCS[c][1]
        arcs.append((i, j, c))
    return best[Lg, Lp], bp, arcs[::-1], gap


def counts_of(entries, table, A, P):
    """-> (total loglik, {type: count}) with the counts added in (word, i, j, code) order"""
    total, cnt = 0.0, defaultdict(float)
    for L, Ph in entries:
        ll, post = expect(L, Ph, table, A, P)
        total += ll
        for i in range(len(L)):
            for j in range(len(Ph) + 1):
                for c, (ex, _, t) in enumerate(out_arcs(L, Ph, i, j, table, A, P)):
                    if ex:
                        cnt[t] += post[i, j, c]
    return total, cnt


def m_step(cnt, A, P):
    table = np.full(table_size(A, P), NINF)
    S = 0.0
    for t in sorted(cnt):
        S += cnt[t]
    for t in sorted(cnt):
        q = cnt[t] / S
        table[t] = math.log(q) if q > 0 else NINF
    return table


def train(entries, A, P, iters=8, tol=1e-5):
    """-> (table, [loglik per E-step after the flat start])"""
    _, cnt = counts_of(entries, np.zeros(table_size(A, P)), A, P)
    table, history = m_step(cnt, A, P), []
    for _ in range(iters):
        ll, cnt = counts_of(entries, table, A, P)
        table = m_step(cnt, A, P)
        history.append(ll)
        if len(history) > 1 and (history[-1] - history[-2]) / len(entries) < tol:
            break
    return table, history


def sequences(entries, table, A, P):
    """-> (token table: the sorted dense types of the Viterbi sequences, sequences of token ids, the per-entry tie gaps)"""
    dense, gaps = [], []
    for L, Ph in entries:
        _, _, arcs, gap = viterbi(L, Ph, table, A, P)
        dense.append([arc_type(c, L[i:i + ARCS[c][0]], Ph[j:j + ARCS[c][1]], A, P) for i, j, c in arcs])
        gaps.append(gap)
    tokens = sorted({t for s in dense for t in s})
    at = {t: k for k, t in enumerate(tokens)}
    return tokens, [[at[t] for t in s] for s in dense], gaps


# ------------------------------------------------------------------------------------------------ the n-gram
def kneser_ney(seqs, T, N):
    """-> {n: {ngram tuple: [logp, bow]}} in back-off form"""
    BOS, EOS, V = T, T + 1, T + 1
    c = {n: defaultdict(float) for n in range(1, N + 1)}
    for s in seqs:
        padded = [BOS] * (N - 1) + list(s) + [EOS]
        for k in range(N - 1, len(padded)):
            c[N][tuple(padded[k - N + 1:k + 1])] += 1.0
    for n in range(N - 1, 0, -1):
        for g in c[n + 1]:
            c[n][g[1:]] += 1.0
    D = {}
    for n in range(1, N + 1):
        n1, n2 = sum(1 for v in c[n].values() if v == 1), sum(1 for v in c[n].values() if v == 2)
        D[n] = n1 / (n1 + 2.0 * n2) if n1 and n2 else 0.5
    prob, gam = {n: {} for n in range(1, N + 1)}, {n: {} for n in range(2, N + 2)}
    tot = sum(c[1][g] for g in sorted(c[1]))
    for w in list(range(T)) + [EOS]:
        prob[1][(w,)] = max(c[1].get((w,), 0.0) - D[1], 0.0) / tot + (D[1] * len(c[1]) / tot) / V
    prob[1][(BOS,)] = 0.0
    for n in range(2, N + 1):
        tot, n1p = defaultdict(float), defaultdict(float)
        for g in sorted(c[n]):
            tot[g[:-1]] += c[n][g]
            n1p[g[:-1]] += 1.0
        for h in tot:
            gam[n][h] = D[n] * n1p[h] / tot[h]
        for g in c[n]:
            prob[n][g] = (c[n][g] - D[n]) / tot[g[:-1]] + gam[n][g[:-1]] * prob[n - 1][g[1:]]
    model = {}
    for n in range(1, N + 1):
        model[n] = {g: [math.log(p) if p > 0 else NINF, 0.0] for g, p in prob[n].items()}
        for h, v in gam[n + 1].items() if n < N else ():
            model[n].setdefault(h, [NINF, 0.0])[1] = math.log(v)
    return model, D


def model_from_arrays(lm, N):
    """the product's arrays (keys, logp, bow, offs) -> the dict form"""
    model = {}
    for n in range(1, N + 1):
        model[n] = {}
        for k in range(int(lm["offs"][n - 1]), int(lm["offs"][n])):
            key = int(lm["keys"][k])
            model[n][tuple((key >> (16 * (n - 1 - d))) & 0xffff for d in range(n))] = [float(lm["logp"][k]), float(lm["bow"][k])]
    return model


def lookup(model, N, hist, tok):
    """log P(tok | the last N - 1 ids of hist)"""
    hist, acc = tuple(hist)[len(hist) - (N - 1):] if N > 1 else (), 0.0
    for n in range(N, 0, -1):
        ctx = hist[len(hist) - (n - 1):] if n > 1 else ()
        e = model[n].get(ctx + (tok,))
        if e is not None:
            return acc + e[0]
        if n == 1:
            break
        h = model[n - 1].get(ctx)
        if h is not None:
            acc += h[1]
    return NINF


# ------------------------------------------------------------------------------------------------ decoding
def spelling(type_letters, A):
    """{letter chunk tuple: ascending token ids}"""
    sp = defaultdict(list)
    for t, ls in enumerate(type_letters):
        sp[tuple(int(a) for a in ls if a >= 0)].append(t)
    return sp


def beam_search(L, sp, model, N, K, T, type_phones):
    """-> (phones or None, score, beams [per position [(score, hist tuple of 3, parent position, parent slot)]], the smallest gap
    that decided anything)"""
    BOS, EOS = T, T + 1
    beams, gap = [[(0.0, (BOS, BOS, BOS), -1, -1)]], math.inf
    for i in range(1, len(L) + 1):
        cands = []
        for back in (1, 2):
            if i - back < 0:
                continue
            for k, (sc, hist, _, _) in enumerate(beams[i - back]):
                for t in sp.get(tuple(L[i - back:i]), []):
                    cands.append((sc + lookup(model, N, hist, t), hist[1:] + (t,), i - back, k))
        cands = [x for x in cands if x[0] != NINF]
        order = sorted(range(len(cands)), key=lambda e: (-cands[e][0], e))
        if len(order) > K:
            gap = min(gap, cands[order[K - 1]][0] - cands[order[K]][0])
        beams.append([cands[e] for e in order[:K]])
    finals = [(sc + lookup(model, N, hist, EOS), k) for k, (sc, hist, _, _) in enumerate(beams[len(L)])] if L else []
    finals = [f for f in finals if f[0] != NINF]
    if not finals:
        return None, NINF, beams, gap
    order = sorted(finals, key=lambda f: (-f[0], f[1]))
    if len(order) > 1:
        gap = min(gap, order[0][0] - order[1][0])
    pos, slot, toks = len(L), order[0][1], []
    while pos > 0:
        _, hist, ppos, pslot = beams[pos][slot]
        toks.append(hist[-1])
        pos, slot = ppos, pslot
    phones = [int(p) for t in toks[::-1] for p in type_phones[t] if p >= 0]
    return phones, order[0][0], beams, gap


def brute_force(L, sp, model, N, T, type_phones):
    """every segmentation and token sequence of a short word -> (phones of the best or None, its score, number of complete paths).
    Ties are broken as the specification breaks them when nothing is pruned: a hypothesis's rank at its position is the order of
    key = (-score, 0 | 1 for a parent one | two letters back, the parent's key, token), and of two complete paths with the same final
    score the one of the lower rank at the last position wins."""
    BOS, EOS = T, T + 1
    best, n_paths = None, 0

    def walk(i, sc, hist, toks, key):
        nonlocal best, n_paths
        if sc == NINF:                                                     # the search never keeps such a hypothesis
            n_paths += i == len(L)
            return
        if i == len(L):
            n_paths += 1
            v = sc + lookup(model, N, hist, EOS)
            if v != NINF and (best is None or (-v, key) < (-best[0], best[2])):
                best = (v, list(toks), key)
            return
        for fwd in (1, 2):
            if i + fwd <= len(L):
                for t in sp.get(tuple(L[i:i + fwd]), []):
                    s2 = sc + lookup(model, N, hist, t)
                    walk(i + fwd, s2, hist[1:] + (t,), toks + [t], (-s2, fwd - 1, key, t))

    walk(0, 0.0, (BOS, BOS, BOS), [], ())
    if best is None:
        return None, NINF, n_paths
    return [int(p) for t in best[1] for p in type_phones[t] if p >= 0], best[0], n_paths


# ------------------------------------------------------------------------------------------------ the whole pipeline
def split(n, holdout, seed):
    """indices (train, held out) of n used entries: the first round(holdout n) of a seeded permutation are held out"""
    perm = np.random.RandomState(seed).permutation(n)
    out = set(perm[:int(round(holdout * n))].tolist())
    return [k for k in range(n) if k not in out], [k for k in range(n) if k in out]


def train_model(entries, A, P, order=4, iters=8, tol=1e-5):
    """entries [(letter ids, phone ids)] -> dict(table, history, tokens, type_letters, type_phones, model, spelling, align_gaps)"""
    table, history = train(entries, A, P, iters, tol)
    tokens, seqs, gaps = sequences(entries, table, A, P)
    NQ = 1 + P + P * P
    tl, tp = [], []
    for t in tokens:
        if t >= A * NQ:
            r = t - A * NQ
            tl.append([r // P // A, r // P % A]), tp.append([r % P, -1])
        else:
            a, q = divmod(t, NQ)
            tl.append([a, -1])
            tp.append([-1, -1] if q == 0 else [q - 1, -1] if q <= P else [(q - 1 - P) // P, (q - 1 - P) % P])
    model, D = kneser_ney(seqs, len(tokens), order)
    return {"table": table, "history": history, "tokens": tokens, "seqs": seqs, "type_letters": tl, "type_phones": tp, "model": model,
            "discounts": D, "spelling": spelling(tl, A), "align_gaps": gaps, "order": order}


def pronounce(m, L, K):
    return beam_search(L, m["spelling"], m["model"], m["order"], K, len(m["tokens"]), m["type_phones"])
