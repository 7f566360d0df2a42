"""float64 numpy oracle of the objective scores, written from the specification in fastspeech2_amd/metrics.py's docstring (not from
the kernels): cepstra, DTW with backtracking, the F0 sums along the path and the per-pair scores, one pair at a time with a plain
loop over the rows of the accumulated-cost matrix.  `brute_force` enumerates every monotone path of a small matrix."""
import math

import numpy as np

INF = np.inf
MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)


def dct_table(n_mel, K):
    C = np.empty((K, n_mel))
    for k in range(1, K + 1):
        for m in range(n_mel):
            C[k - 1, m] = math.sqrt(2.0 / n_mel) * math.cos(math.pi * k * (2 * m + 1) / (2 * n_mel))
    return C


def cepstra(mel, K=13):
    """mel (n_mel, T) -> c (T, K), summed over m in ascending order"""
    x = np.asarray(mel, np.float64)
    C = dct_table(x.shape[0], K)
    c = np.zeros((x.shape[1], K))
    for m in range(x.shape[0]):
        c += x[m][:, None] * C[:, m][None, :]
    return c


def cepstra_bound(mel, K=13):
    """n_mel 2^-52 sum_m |x_m| |C_km| per element (T, K): twice the standard bound n u sum |x_m C_km| (u = 2^-53) of a length-n_mel
    sum of rounded products in any order, fused or not"""
    x = np.abs(np.asarray(mel, np.float64))
    return x.shape[0] * 2.0 ** -52 * (x.T @ np.abs(dct_table(x.shape[0], K)).T)


def local_cost(a, b):
    """d (T1, T2) = sqrt(sum_k (a_k[i] - b_k[j])^2), k ascending"""
    acc = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        df = a[:, k][:, None] - b[:, k][None, :]
        acc = acc + df * df
    return np.sqrt(acc)


def dtw_on_cost(d):
    """-> (total, pi, pj, backpointers uint8 (T1, T2))"""
    T1, T2 = d.shape
    D = np.full((T1, T2), INF)
    bp = np.zeros((T1, T2), np.uint8)
    for i in range(T1):
        for j in range(T2):
            if i == 0 and j == 0:
                D[0, 0] = d[0, 0]
                continue
            best, code = (D[i - 1, j - 1] if i and j else INF), 0
            up = D[i - 1, j] if i else INF
            left = D[i, j - 1] if j else INF
            if up < best:                                                  # a later code wins only when strictly smaller
                best, code = up, 1
            if left < best:
                best, code = left, 2
            D[i, j] = d[i, j] + best
            bp[i, j] = code
    i, j, pi, pj = T1 - 1, T2 - 1, [], []
    while True:
        pi.append(i)
        pj.append(j)
        if i == 0 and j == 0:
            break
        code = bp[i, j]
        i, j = (i - 1, j - 1) if code == 0 else ((i - 1, j) if code == 1 else (i, j - 1))
    return D[T1 - 1, T2 - 1], np.array(pi[::-1], np.int32), np.array(pj[::-1], np.int32), bp


def dtw_fast(d):
    """`dtw_on_cost` with the inner loop over an anti-diagonal vectorised (the same operations on the same operands)"""
    T1, T2 = d.shape
    D = np.full((T1 + 1, T2 + 1), INF)
    bp = np.zeros((T1, T2), np.uint8)
    D[0, 0] = 0.0                                                          # D(-1, -1) = 0: D(0, 0) = d(0, 0) + 0 by the general rule
    for s in range(T1 + T2 - 1):
        i = np.arange(max(0, s - T2 + 1), min(s, T1 - 1) + 1)
        j = s - i
        best, code = D[i, j].copy(), np.zeros(len(i), np.uint8)
        for c, cand in ((1, D[i, j + 1]), (2, D[i + 1, j])):
            better = cand < best
            best, code = np.where(better, cand, best), np.where(better, c, code).astype(np.uint8)
        D[i + 1, j + 1] = d[i, j] + best
        bp[i, j] = code
    i, j, pi, pj = T1 - 1, T2 - 1, [], []
    while True:
        pi.append(i)
        pj.append(j)
        if i == 0 and j == 0:
            break
        code = bp[i, j]
        i, j = (i - 1, j - 1) if code == 0 else ((i - 1, j) if code == 1 else (i, j - 1))
    return D[T1, T2], np.array(pi[::-1], np.int32), np.array(pj[::-1], np.int32), bp


def dtw(a, b):
    return dtw_fast(local_cost(a, b))[:3]


def path_cost(d, pi, pj):
    """the cost of a path over d, added in path order"""
    total = 0.0
    for i, j in zip(pi, pj):
        total += d[i, j]
    return total


def brute_force(d):
    """every monotone path from (0, 0) to (T1-1, T2-1): -> (the least cost, added in path order, and the path the tie rule picks).
    Among paths of equal cost the rule's choice is found backwards from the end: at each cell the predecessor with the lowest code
    among those that lie on SOME optimal path to that cell."""
    T1, T2 = d.shape
    best = {}

    def walk(i, j, acc, path):
        acc = acc + d[i, j]
        path = path + [(i, j)]
        key = (i, j)
        if key not in best or acc < best[key][0]:
            best[key] = (acc, [path])
        elif acc == best[key][0]:
            best[key][1].append(path)
        if i + 1 < T1 and j + 1 < T2:
            walk(i + 1, j + 1, acc, path)
        if i + 1 < T1:
            walk(i + 1, j, acc, path)
        if j + 1 < T2:
            walk(i, j + 1, acc, path)
    walk(0, 0, 0.0, [])
    opt = {k: v[0] for k, v in best.items()}                               # the least cost of reaching every cell
    i, j, rev = T1 - 1, T2 - 1, []
    while True:
        rev.append((i, j))
        if i == 0 and j == 0:
            break
        cands = [(i - 1, j - 1), (i - 1, j), (i, j - 1)]
        vals = [opt.get(c, INF) if c[0] >= 0 and c[1] >= 0 else INF for c in cands]
        i, j = cands[int(np.argmin(vals))]                                 # argmin takes the first (lowest code) of equal values
    return opt[(T1 - 1, T2 - 1)], rev[::-1]


def f0_sums(pi, pj, f0_ref, f0_syn):
    """-> (V/UV mismatches, both-voiced cells, sum of squared cents)"""
    mism = voiced = 0
    sq = 0.0
    for i, j in zip(pi, pj):
        r, s = float(f0_ref[i]), float(f0_syn[j])
        if (r == 0.0) != (s == 0.0):
            mism += 1
        if r > 0.0 and s > 0.0:
            voiced += 1
            sq += (1200.0 * math.log2(s / r)) ** 2
    return mism, voiced, sq


def scores(total, pi, pj, T1, T2, f0_ref=None, f0_syn=None):
    P = len(pi)
    row = {"mcd_db": MCD_SCALE * float(total) / P, "path_len": P, "frames_ref": int(T1), "frames_syn": int(T2)}
    if f0_ref is not None:
        mism, voiced, sq = f0_sums(pi, pj, f0_ref, f0_syn)
        row["vuv_error"] = mism / P
        row["f0_rmse_cents"] = math.sqrt(sq / voiced) if voiced else float("nan")
        row["n_voiced_pairs"] = voiced
    return row


def score_pair(mel_ref, mel_syn, f0_ref=None, f0_syn=None, K=13):
    """mel (n_mel, frames) and optional F0 tracks of one pair -> the score dict; both sides are cut to min(mel frames, F0 frames)"""
    T1 = mel_ref.shape[1] if f0_ref is None else min(mel_ref.shape[1], len(f0_ref))
    T2 = mel_syn.shape[1] if f0_syn is None else min(mel_syn.shape[1], len(f0_syn))
    total, pi, pj = dtw(cepstra(mel_ref[:, :T1], K), cepstra(mel_syn[:, :T2], K))
    return scores(total, pi, pj, T1, T2, None if f0_ref is None else f0_ref[:T1], None if f0_syn is None else f0_syn[:T2])


def summarize(rows):
    w = np.array([r["path_len"] for r in rows], np.float64)
    out = {"utterances": len(rows)}
    mcd = np.array([r["mcd_db"] for r in rows])
    out["mcd_db_mean"], out["mcd_db_weighted"] = float(np.mean(mcd)), float(np.sum(mcd * w) / np.sum(w))
    if "vuv_error" in rows[0]:
        vuv = np.array([r["vuv_error"] for r in rows])
        out["vuv_error_mean"], out["vuv_error_weighted"] = float(np.mean(vuv)), float(np.sum(vuv * w) / np.sum(w))
        good = [r for r in rows if not math.isnan(r["f0_rmse_cents"])]
        out["f0_nan_utterances"] = len(rows) - len(good)
        if good:
            f0 = np.array([r["f0_rmse_cents"] for r in good])
            nv = np.array([r["n_voiced_pairs"] for r in good], np.float64)
            out["f0_rmse_cents_mean"], out["f0_rmse_cents_weighted"] = float(np.mean(f0)), float(np.sum(f0 * nv) / np.sum(nv))
        else:
            out["f0_rmse_cents_mean"] = out["f0_rmse_cents_weighted"] = float("nan")
    return out
