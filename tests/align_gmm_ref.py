"""float64 numpy oracle of the forced aligner's Gaussian-mixture emissions, written from the "Mixtures" part of the specification in
fastspeech2_amd/align.py's docstring (not from the kernels, and without the product's host code): emissions and responsibilities,
partials, class sums, the update, the split, `fit` and `align`.  The recursions are tests/align_ref.py's.  Tables are w (C, M),
mu (C, M, D), var (C, M, D) and ncomp (C,), the active components per class."""
import numpy as np

from tests.align_ref import flat_gamma, posteriors, viterbi

NINF = -np.inf


def emissions(x, sid, w, mu, var):
    """-> (E [T][J], r [T][J][M])"""
    T, M = x.shape[0], w.shape[1]
    E, r = np.empty((T, len(sid))), np.empty((T, len(sid), M))
    with np.errstate(divide="ignore"):
        logw = np.log(w)                                                   # log 0 = -inf
    done = {}
    for j, c in enumerate(sid):
        if c in done:                                                      # the states of one class share their columns
            E[:, j], r[:, j] = E[:, done[c]], r[:, done[c]]
            continue
        done[c] = j
        N = np.full((T, M), NINF)
        for m in range(M):
            if w[c, m] > 0.0:                                              # -inf + a finite sum otherwise
                N[:, m] = logw[c, m] + -0.5 * np.sum((x - mu[c, m]) ** 2 / var[c, m] + np.log(2.0 * np.pi * var[c, m]), axis=1)
        mx = N[:, 0]
        for m in range(1, M):
            mx = np.maximum(mx, N[:, m])
        s = np.exp(N[:, 0] - mx)
        for m in range(1, M):                                              # ascending m
            s = s + np.exp(N[:, m] - mx)
        E[:, j] = mx + np.log(s)
        r[:, j] = np.exp(N - E[:, j, None])
    return E, r


def partials(gamma, r, x):
    """[J][M][1 + 2 D]: sum_t gamma r [1, x, x^2]"""
    out = []
    for m in range(r.shape[2]):
        g = gamma * r[:, :, m]
        out.append(np.concatenate([g.sum(axis=0)[:, None], g.T @ x, g.T @ (x * x)], axis=1))
    return np.stack(out, axis=1)


def class_sums(parts, graphs, n_classes):
    """-> (C, M, 1 + 2 D), utterances in order, the states of one in ascending order"""
    out = np.zeros((n_classes,) + parts[0].shape[1:])
    for P, g in zip(parts, graphs):
        np.add.at(out, g["sid"], P)
    return out


def update(sums, w, mu, var, ncomp, floor):
    D = mu.shape[2]
    w, mu, var = w.copy(), mu.copy(), var.copy()
    for c in range(len(sums)):
        K = int(ncomp[c])
        n_c = 0.0
        for m in range(K):
            n_c = n_c + sums[c, m, 0]
        for m in range(K):
            n = sums[c, m, 0]
            if n_c >= 1.0:
                w[c, m] = n / n_c
            if n >= 1.0:
                mu[c, m] = sums[c, m, 1:1 + D] / n
                var[c, m] = np.maximum(sums[c, m, 1 + D:] / n - mu[c, m] ** 2, floor)
    return w, mu, var


def split(w, mu, var, ncomp, occ, k, min_split_occ=40.0):
    """split step k: every class with fewer than k + 1 components whose heaviest component (lowest index on ties) had at least
    `min_split_occ` frames in the last pass gains one"""
    w, mu, var, ncomp = w.copy(), mu.copy(), var.copy(), np.array(ncomp).copy()
    for c in range(len(w)):
        K = int(ncomp[c])
        h = 0
        for m in range(1, K):
            if w[c, m] > w[c, h]:
                h = m
        if K < k + 1 and occ[c, h] >= min_split_occ:
            half, d = w[c, h] / 2.0, 0.2 * np.sqrt(var[c, h])
            w[c, h], w[c, K] = half, half
            mu[c, K] = mu[c, h] + d
            mu[c, h] = mu[c, h] - d
            var[c, K] = var[c, h]
            ncomp[c] = K + 1
    return w, mu, var, ncomp


def fit(xs, graphs, n_classes, iters, mixtures=1, mix_iters=4, min_split_occ=40.0):
    """Flat start and `iters` passes with one component, then for k = 1 .. M - 1 a split and `mix_iters` passes
    -> (w, mu, var, ncomp, [loglik per frame of every pass], [ncomp after every split], (mu, var) of the one-component system the
    splits started from)."""
    M, D = mixtures, xs[0].shape[1]
    allx = np.concatenate(xs)
    g_mean, g_var = allx.mean(axis=0), allx.var(axis=0)
    floor = 1e-2 * g_var
    w, mu, var = np.zeros((n_classes, M)), np.zeros((n_classes, M, D)), np.ones((n_classes, M, D))
    w[:, 0], mu[:, 0], var[:, 0] = 1.0, g_mean, g_var
    ncomp = np.ones(n_classes, np.int64)
    ones = [np.ones((len(x), len(g["sid"]), M)) for x, g in zip(xs, graphs)]
    sums = class_sums([partials(flat_gamma(g, len(x)), r, x) for x, g, r in zip(xs, graphs, ones)], graphs, n_classes)
    sums[:, 1:] = 0.0                                                      # the flat start knows one component
    w, mu, var = update(sums, w, mu, var, ncomp, floor)
    history, stages, n_frames = [], [], sum(len(x) for x in xs)

    def one_pass(w, mu, var):
        parts, total = [], 0.0
        for x, g in zip(xs, graphs):
            E, r = emissions(x, g["sid"], w, mu, var)
            gamma, _, ll = posteriors(E, g)
            parts.append(partials(gamma, r, x))
            total += ll
        sums = class_sums(parts, graphs, n_classes)
        history.append(total / n_frames)
        return update(sums, w, mu, var, ncomp, floor) + (sums[:, :, 0],)

    occ = sums[:, :, 0]
    for _ in range(iters):
        w, mu, var, occ = one_pass(w, mu, var)
    single = (mu[:, 0].copy(), var[:, 0].copy())
    for k in range(1, M):
        w, mu, var, ncomp = split(w, mu, var, ncomp, occ, k, min_split_occ)
        stages.append(ncomp.copy())
        for _ in range(mix_iters):
            w, mu, var, occ = one_pass(w, mu, var)
    return w, mu, var, ncomp, history, stages, single


def align(x, graph, w, mu, var):
    return viterbi(emissions(x, graph["sid"], w, mu, var)[0], graph)[2]
