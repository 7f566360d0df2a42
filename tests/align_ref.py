"""float64 numpy oracle of the forced aligner, written from the specification in fastspeech2_amd/align.py's docstring (not from the
kernels): features, emissions, forward / backward, statistics, the update, Viterbi and backtracking, one utterance at a time with
a plain loop over frames (vector operations over the states).  A graph is the dict `align.utterance_graph` returns (sid, skip,
block, alt, blocks)."""
import numpy as np

NINF = -np.inf


def features(mel):
    """mel (n_mel, T) -> x (T, 2 n_mel)"""
    m = np.asarray(mel, np.float64).T
    x = m - m.mean(axis=0, keepdims=True)
    T = x.shape[0]
    hi = x[np.minimum(np.arange(T) + 1, T - 1)]
    lo = x[np.maximum(np.arange(T) - 1, 0)]
    return np.concatenate([x, (hi - lo) / 2.0], axis=1)


def emissions(x, sid, mu, var):
    """E[t, j] = -1/2 sum_d ((x_d - mu_d)^2 / var_d + log(2 pi var_d))"""
    E = np.empty((x.shape[0], len(sid)))
    for j, c in enumerate(sid):
        E[:, j] = -0.5 * np.sum((x - mu[c]) ** 2 / var[c] + np.log(2.0 * np.pi * var[c]), axis=1)
    return E


def lse(*v):
    """elementwise m + log(sum exp(v - m)), m the maximum, terms in argument order; -inf where every argument is"""
    v = [np.asarray(a, np.float64) for a in v]
    m = v[0]
    for a in v[1:]:
        m = np.maximum(m, a)
    safe = np.where(m == NINF, 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(m == NINF, NINF, safe + np.log(sum(np.exp(a - safe) for a in v)))


def starts(graph):
    return [0] + ([graph["alt"][0]] if graph["alt"][0] >= 0 else [])


def ends(graph):
    J = len(graph["sid"])
    return ([graph["alt"][1]] if graph["alt"][1] >= 0 else []) + [J - 1]           # index order


def _pred(row, skip):
    """the three predecessor values of every state: self, next (j - 1), skip"""
    nxt = np.concatenate([[NINF], row[:-1]])
    skp = np.where(skip >= 0, row[np.maximum(skip, 0)], NINF)
    return row, nxt, skp


def forward(E, graph):
    T, J = E.shape
    alpha = np.full((T, J), NINF)
    for j in starts(graph):
        alpha[0, j] = E[0, j]
    for t in range(1, T):
        alpha[t] = E[t] + lse(*_pred(alpha[t - 1], graph["skip"]))
    return alpha, float(lse(*[alpha[T - 1, j] for j in ends(graph)]))


def backward(E, graph):
    T, J = E.shape
    to = np.full(J, -1)
    for j, s in enumerate(graph["skip"]):
        if s >= 0:
            to[s] = j
    beta = np.full((T, J), NINF)
    for j in ends(graph):
        beta[T - 1, j] = 0.0
    for t in range(T - 2, -1, -1):
        eb = E[t + 1] + beta[t + 1]
        beta[t] = lse(eb, np.concatenate([eb[1:], [NINF]]), np.where(to >= 0, eb[np.maximum(to, 0)], NINF))
    return beta


def posteriors(E, graph):
    alpha, ll = forward(E, graph)
    with np.errstate(invalid="ignore"):
        g = np.exp(alpha + backward(E, graph) - ll)
    return np.where(np.isnan(g), 0.0, g), alpha, ll


def partials(gamma, x):
    """[J][1 + 2 D]: sum_t gamma [1, x, x^2]"""
    return np.concatenate([gamma.sum(axis=0)[:, None], gamma.T @ x, gamma.T @ (x * x)], axis=1)


def class_sums(parts, graphs, n_classes):
    out = np.zeros((n_classes, parts[0].shape[1]))
    for P, g in zip(parts, graphs):
        np.add.at(out, g["sid"], P)
    return out


def update(sums, mu, var, floor):
    D = mu.shape[1]
    mu, var = mu.copy(), var.copy()
    for c in range(len(sums)):
        n = sums[c, 0]
        if n >= 1.0:
            mu[c] = sums[c, 1:1 + D] / n
            var[c] = np.maximum(sums[c, 1 + D:] / n - mu[c] ** 2, floor)
    return mu, var


def flat_gamma(graph, T):
    opt = [b[2] for b in graph["blocks"]]
    mand = [j for j, k in enumerate(graph["block"]) if not opt[k]]
    g = np.zeros((T, len(graph["sid"])))
    for t in range(T):
        g[t, mand[(t * len(mand)) // T]] = 1.0
    return g


def fit(xs, graphs, n_classes, iters, perturb=None):
    """Flat start + `iters` Baum-Welch passes -> (mu, var, [loglik per frame]).  `perturb(E)` may replace each emission matrix (the
    1-ulp sensitivity run of the tests)."""
    allx = np.concatenate(xs)
    g_mean, g_var = allx.mean(axis=0), allx.var(axis=0)
    floor = 1e-2 * g_var
    sums = class_sums([partials(flat_gamma(g, len(x)), x) for x, g in zip(xs, graphs)], graphs, n_classes)
    mu, var = update(sums, np.tile(g_mean, (n_classes, 1)), np.tile(g_var, (n_classes, 1)), floor)
    history, n_frames = [], sum(len(x) for x in xs)
    for _ in range(iters):
        parts, total = [], 0.0
        for x, g in zip(xs, graphs):
            E = emissions(x, g["sid"], mu, var)
            if perturb is not None:
                E = perturb(E)
            gamma, _, ll = posteriors(E, g)
            parts.append(partials(gamma, x))
            total += ll
        mu, var = update(class_sums(parts, graphs, n_classes), mu, var, floor)
        history.append(total / n_frames)
    return mu, var, history


def viterbi(E, graph):
    """-> (backpointers uint8 [T][J], end state, frames per block)"""
    T, J = E.shape
    skip = graph["skip"]
    delta = np.full(J, NINF)
    for j in starts(graph):
        delta[j] = E[0, j]
    bp = np.zeros((T, J), np.uint8)
    for t in range(1, T):
        own, nxt, skp = _pred(delta, skip)
        best, code = own.copy(), np.zeros(J, np.uint8)
        for c, cand in ((1, nxt), (2, skp)):                               # a later code wins only when strictly larger
            better = cand > best
            best, code = np.where(better, cand, best), np.where(better, c, code).astype(np.uint8)
        delta, bp[t] = E[t] + best, code
    end = None
    for j in ends(graph):
        if end is None or delta[j] > delta[end]:
            end = j
    frames = np.zeros(len(graph["blocks"]), np.int32)
    j = end
    for t in range(T - 1, -1, -1):
        frames[graph["block"][j]] += 1
        if t:
            j = (j, j - 1, skip[j])[bp[t, j]]
    return bp, end, frames


def align(x, graph, mu, var, perturb=None):
    E = emissions(x, graph["sid"], mu, var)
    return viterbi(E if perturb is None else perturb(E), graph)[2]
