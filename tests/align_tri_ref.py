"""float64 numpy oracle of the forced aligner's triphone stage, written from the "Triphones" part of the specification in
fastspeech2_amd/align.py's docstring (not from the kernel, and without the product's host code): word-internal contexts, the items,
the generated questions, the node likelihood, the gain of every (node, question), the level-by-level tree, the replay under the leaf
budget, the walk of an unseen triple, the whole schedule and decoding, and `gain_bounds`, the rounding bound the GPU test holds
the kernel's gains to.  The recursions and the single-Gaussian update are tests/align_ref.py's, the mixture stages
tests/align_gmm_ref.py's; the stages in front (LDA, fMLLR) come from tests/align_lda_ref.py and tests/align_fmllr_ref.py through
`front`.

Bounds.  U = 2^-53.  A sum of m terms in any order is within m U sum |terms| of the exact sum (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2, with 1 / (1 - m U) < 1 + 1e-9); the kernel's sum over a node's m items (the products with 0 and
1 are exact, the items that answer the other way add exact zeros) takes one such error and numpy's sum that stands for the exact
one another: e_x = BOUND_CONSTANT m U sum |x_i| for x = n, a_d, q_d of a side.  They are carried to first order (second-order terms are
covered by the factor 1 + 1e-6, the perturbations being below 1e-9 relative) through
  v_d = max(q_d / n - (a_d / n)^2, floor_d):   e_v = e_q / n + |q| e_n / n^2 + 2 |mu| e_a / n + 2 mu^2 e_n / n, plus the roundings of the
      two quotients, the square and the difference on either side, 2 U (2 |q| / n + 4 mu^2); the maximum with the floor does not
      increase an error;
  t_d = log(2 pi v_d) + 1:   the conditioning of the logarithm, e_v / (v - e_v) (infinite when e_v >= v: such an entry is not
      checked), the kernel's logarithm (3 ulp, the OpenCL bound the device library keeps), numpy's (1 ulp), the two roundings of
      2 pi v on either side and the addition: U (6 (|t| + 1) + 4);
  S = sum_d t_d:   sum e_t + BOUND_CONSTANT D U sum |t_d|;
  L = -n S / 2:   (n e_S + e_n |S|) / 2 + 6 U |L|;
  gain = (L(yes) + L(no)) - L(node):   the three bounds and 4 U (|L(yes)| + |L(no)| + |L(node)|) for the two additions on either side.
No subtraction of pooled sums occurs: the kernel accumulates the no side directly."""
import heapq

import numpy as np

from tests import align_gmm_ref as GR
from tests import align_ref as R

U = 2.0 ** -53
BOUND_CONSTANT = 2.0
CI = ("sil", "sp", "spn")


# ------------------------------------------------------------------------------------------------ contexts and items
def contexts(graph, phone_ids, states):
    """(J, 4) int: (l, p, r, s) per state; `#` = len(phone_ids)"""
    bnd, blocks = len(phone_ids), graph["blocks"]
    rows = []
    for k, (p, w, _) in enumerate(blocks):
        l = r = bnd
        if p not in CI and w >= 0:
            if k > 0 and blocks[k - 1][1] == w and blocks[k - 1][0] not in CI:
                l = phone_ids[blocks[k - 1][0]]
            if k + 1 < len(blocks) and blocks[k + 1][1] == w and blocks[k + 1][0] not in CI:
                r = phone_ids[blocks[k + 1][0]]
        rows += [(l, phone_ids[p], r, s) for s in range(states)]
    return np.array(rows, dtype=np.int64)


def item_table(ctxs):
    """the distinct (p, s, l, r) over all utterances, sorted -> list of tuples"""
    return sorted({(int(p), int(s), int(l), int(r)) for c in ctxs for l, p, r, s in c})


def item_sums(parts, ctxs, items):
    """partials [J][1 + 2 D] of every utterance -> (N_items, 1 + 2 D), utterances in order, states ascending"""
    at = {key: i for i, key in enumerate(items)}
    out = np.zeros((len(items), parts[0].shape[1]))
    for P, c in zip(parts, ctxs):
        for j, (l, p, r, s) in enumerate(c):
            out[at[(int(p), int(s), int(l), int(r))]] += P[j]
    return out


# ------------------------------------------------------------------------------------------------ likelihood, gains, bounds
def loglik(n, a, q, floor):
    if not n > 0.0:
        return 0.0
    v = np.maximum(q / n - (a / n) ** 2, floor)
    s = 0.0
    for t in np.log(2.0 * np.pi * v) + 1.0:                                # d ascending
        s += t
    return -0.5 * n * s


def _answers(member, left, right, items):
    """(2 n_sets, m) bool: the answers of the items to every question"""
    return np.concatenate([member[:, left[items]], member[:, right[items]]], axis=0) != 0


def gains(sums, left, right, nodes, member, floor, min_occ):
    """-> (gain (n_nodes, 2 n_sets), -inf where a side has n < min_occ; n_yes; n_no)"""
    D = (sums.shape[1] - 1) // 2
    Q = 2 * member.shape[0]
    g, ny, nn = np.full((len(nodes), Q), -np.inf), np.zeros((len(nodes), Q)), np.zeros((len(nodes), Q))
    for m, items in enumerate(nodes):
        T = sums[items]
        tot = T.sum(axis=0)
        l_node = loglik(tot[0], tot[1:1 + D], tot[1 + D:], floor)
        ans = _answers(member, left, right, items)
        for q in range(Q):
            y, n = T[ans[q]].sum(axis=0), T[~ans[q]].sum(axis=0)
            ny[m, q], nn[m, q] = y[0], n[0]
            if y[0] >= min_occ and n[0] >= min_occ:
                g[m, q] = (loglik(y[0], y[1:1 + D], y[1 + D:], floor) + loglik(n[0], n[1:1 + D], n[1 + D:], floor)) - l_node
    return g, ny, nn


def _lik_bound(tab, err, floor):
    """tab, err (..., 1 + 2 D): pooled sums and their bounds -> (|L|, bound of L), arrays over the leading axes; n = 0 gives (0, 0)"""
    D = (tab.shape[-1] - 1) // 2
    n, en = tab[..., :1], err[..., :1]
    ok = n > 0.0
    n1 = np.where(ok, n, 1.0)
    a, q, ea, eq = tab[..., 1:1 + D], tab[..., 1 + D:], err[..., 1:1 + D], err[..., 1 + D:]
    mu = a / n1
    v = np.maximum(q / n1 - mu * mu, floor)
    ev = (eq / n1 + np.abs(q) * en / n1 ** 2 + 2.0 * np.abs(mu) * ea / n1 + 2.0 * mu * mu * en / n1) * (1.0 + 1e-6) \
        + 2.0 * U * (2.0 * np.abs(q) / n1 + 4.0 * mu * mu)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ev < v, ev / (v - ev), np.inf)
    t = np.log(2.0 * np.pi * v) + 1.0
    et = rel + U * (6.0 * (np.abs(t) + 1.0) + 4.0)
    S, eS = t.sum(axis=-1), et.sum(axis=-1) + BOUND_CONSTANT * D * U * np.abs(t).sum(axis=-1)
    n, en = n[..., 0], en[..., 0]
    L = 0.5 * n * np.abs(S)
    eL = 0.5 * (n * eS + en * np.abs(S)) * (1.0 + 1e-6) + 6.0 * U * L
    return np.where(ok[..., 0], L, 0.0), np.where(ok[..., 0], eL, 0.0)


def gain_bounds(sums, left, right, nodes, member, floor, min_occ):
    """-> (bound of the gain (n_nodes, 2 n_sets); unsure (same shape, bool): the oracle's n of a side is within its own bound of
    `min_occ`, so eligibility (and with it the gain and n_yes) is not compared there; the bound of n_yes)"""
    Q = 2 * member.shape[0]
    bound, unsure, eny = np.zeros((len(nodes), Q)), np.zeros((len(nodes), Q), bool), np.zeros((len(nodes), Q))
    for m, items in enumerate(nodes):
        T, k = sums[items], BOUND_CONSTANT * len(items) * U
        ans = _answers(member, left, right, items).astype(np.float64)
        Y, N, aY, aN = ans @ T, (1.0 - ans) @ T, ans @ np.abs(T), (1.0 - ans) @ np.abs(T)
        Ly, ey = _lik_bound(Y, k * aY, floor)
        Ln, en = _lik_bound(N, k * aN, floor)
        L0, e0 = _lik_bound(T.sum(axis=0), k * np.abs(T).sum(axis=0), floor)
        bound[m] = ey + en + e0 + 4.0 * U * (Ly + Ln + L0)
        unsure[m] = (np.abs(Y[:, 0] - min_occ) <= k * aY[:, 0]) | (np.abs(N[:, 0] - min_occ) <= k * aN[:, 0])
        eny[m] = k * aY[:, 0]
    return bound, unsure, eny


def best(g):
    """per node (the question of the largest gain, the lowest on ties, -1 when none is eligible; that gain)"""
    q = np.argmax(g, axis=1)
    top = g[np.arange(len(g)), q]
    return np.where(np.isfinite(top), q, -1), top


# ------------------------------------------------------------------------------------------------ questions
def questions(mono, phones, states, floor, n_symbols):
    """bottom-up clustering of the real phones on the pooled monophone sums mono (n_phones states, 1 + 2 D) -> member (2 P - 1,
    n_symbols) uint8: singletons ascending, merged sets in merge order without the full set, {#}"""
    D = (mono.shape[1] - 1) // 2

    def lik(ids):
        tot = 0.0
        for s in range(states):
            t = sum(mono[p * states + s] for p in ids)
            tot += loglik(t[0], t[1:1 + D], t[1 + D:], floor)
        return tot
    clusters = [[int(p)] for p in sorted(phones)]
    sets = [list(c) for c in clusters]
    while len(clusters) > 2:
        pick, low = None, None
        for i in range(len(clusters)):                                     # clusters stay ordered by their lowest phone
            for j in range(i + 1, len(clusters)):
                c = lik(clusters[i]) + lik(clusters[j]) - lik(clusters[i] + clusters[j])
                if low is None or c < low:
                    pick, low = (i, j), c
        i, j = pick
        clusters[i] = sorted(clusters[i] + clusters[j])
        del clusters[j]
        sets.append(list(clusters[i]))
    sets.append([n_symbols - 1])
    member = np.zeros((len(sets), n_symbols), np.uint8)
    for k, ids in enumerate(sets):
        member[k, ids] = 1
    return member


# ------------------------------------------------------------------------------------------------ tree
def grow(items, states, n_phones, fixed, sums, member, floor, min_occ, min_gain):
    """the full tree: nodes as dicts(items, q, yes, no, gain), roots p S + s first, then every level's children in ascending parent
    order, yes before no"""
    left, right = np.array([k[2] for k in items]), np.array([k[3] for k in items])
    n_sets = member.shape[0]
    nodes = [{"items": np.array([i for i, k in enumerate(items) if k[0] * states + k[1] == m], dtype=np.int64), "q": -1, "yes": -1,
              "no": -1, "gain": -np.inf} for m in range(n_phones * states)]
    level = [m for m in range(len(nodes)) if m not in fixed and len(nodes[m]["items"])]
    while level:
        g, _, _ = gains(sums, left, right, [nodes[m]["items"] for m in level], member, floor, min_occ)
        q, top = best(g)
        nxt = []
        for m, qq, gg in zip(level, q, top):
            if qq < 0 or not gg > min_gain:
                continue
            it = nodes[m]["items"]
            ans = member[qq % n_sets, (right if qq >= n_sets else left)[it]] != 0
            nodes[m].update(q=int(qq), yes=len(nodes), no=len(nodes) + 1, gain=float(gg))
            nodes.append({"items": it[ans], "q": -1, "yes": -1, "no": -1, "gain": -np.inf})
            nodes.append({"items": it[~ans], "q": -1, "yes": -1, "no": -1, "gain": -np.inf})
            nxt += [nodes[m]["yes"], nodes[m]["no"]]
        level = nxt
    return nodes


def replay(nodes, n_roots, budget):
    """-> (question, yes, no, leaf: int arrays over the nodes, -1 where not split / no leaf; total gain)"""
    if budget < n_roots:
        raise ValueError("the leaf budget is below the number of roots")
    heap = [(-nodes[m]["gain"], m) for m in range(n_roots) if nodes[m]["q"] >= 0]
    heapq.heapify(heap)
    split, reach, count, total = set(), set(range(n_roots)), n_roots, 0.0
    while heap and count < budget:
        g, m = heapq.heappop(heap)
        split.add(m)
        count, total = count + 1, total - g
        for c in (nodes[m]["yes"], nodes[m]["no"]):
            reach.add(c)
            if nodes[c]["q"] >= 0:
                heapq.heappush(heap, (-nodes[c]["gain"], c))
    question, yes, no, leaf = (np.full(len(nodes), -1, np.int64) for _ in range(4))
    k = 0
    for m in range(len(nodes)):
        if m in split:
            question[m], yes[m], no[m] = nodes[m]["q"], nodes[m]["yes"], nodes[m]["no"]
        elif m in reach:
            leaf[m], k = k, k + 1
    return question, yes, no, leaf, total


def best_first(nodes, n_roots, budget):
    """naive best-first splitting over the same recorded best splits: at every step the leaf of the largest gain (the lowest node on
    ties) -> the set of split nodes"""
    leaves, split = set(range(n_roots)), set()
    while len(leaves) < budget:
        cand = [m for m in sorted(leaves) if nodes[m]["q"] >= 0]
        if not cand:
            break
        m = max(cand, key=lambda c: (nodes[c]["gain"], -c))
        leaves.remove(m)
        leaves |= {nodes[m]["yes"], nodes[m]["no"]}
        split.add(m)
    return split


def walk(tree, member, key, states):
    """the leaf of one logical state key = (p, s, l, r)"""
    question, yes, no, leaf = tree[:4]
    m, n_sets = key[0] * states + key[1], member.shape[0]
    while question[m] >= 0:
        q = question[m]
        m = yes[m] if member[q % n_sets, key[3] if q >= n_sets else key[2]] else no[m]
    return int(leaf[m])


def leaf_graph(graph, phone_ids, states, model):
    sid = [walk(model["tree"], model["member"], (int(p), int(s), int(l), int(r)), states) for l, p, r, s in contexts(graph, phone_ids, states)]
    return dict(graph, sid=np.array(sid, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the schedule
def fit(xs, graphs, phone_ids, states, iters, leaves, tri_iters=4, min_occ=100.0, min_gain=0.0, member=None, mixtures=1, mix_iters=4,
        min_split_occ=40.0, front=None):
    """The schedule -> dict(mu, var, history and, with leaves > 0: tree (question, yes, no, leaf, total gain), member, items, n_leaves,
    fs (the features the stage saw); with mixtures > 1: w, gmu, gvar, ncomp).  leaves = 0 is tests/align_ref.py's `fit` exactly.
    `front` = (fs, mu, var, floor, history, jac) replaces the monophone passes in x by the result of the stages in front."""
    n_classes = len(phone_ids) * states
    if front is None:
        mu, var, history = R.fit(xs, graphs, n_classes, iters)
        fs, floor, jac = xs, 1e-2 * np.concatenate(xs).var(axis=0), 0.0
    else:
        fs, mu, var, floor, history, jac = front
    out = {"mu": mu, "var": var, "history": list(history), "states": states, "phone_ids": phone_ids}
    if not leaves:
        return out
    n_frames = sum(len(f) for f in fs)
    ctxs = [contexts(g, phone_ids, states) for g in graphs]
    items = item_table(ctxs)
    parts, total = [], 0.0
    for f, g in zip(fs, graphs):                                           # the statistics pass under the monophone table
        gamma, _, ll = R.posteriors(R.emissions(f, g["sid"], mu, var), g)
        parts.append(R.partials(gamma, f))
        total += ll
    history = list(history) + [(total + jac) / n_frames]
    sums = item_sums(parts, ctxs, items)
    fixed = {phone_ids[p] * states + s for p in CI for s in range(states)}
    if member is None:
        mono = np.zeros((n_classes, sums.shape[1]))
        for i, k in enumerate(items):                                      # items ascending
            mono[k[0] * states + k[1]] += sums[i]
        member = questions(mono, [p for p in range(len(phone_ids)) if p * states not in fixed], states, floor, len(phone_ids) + 1)
    nodes = grow(items, states, len(phone_ids), fixed, sums, member, floor, min_occ, min_gain)
    tree = replay(nodes, n_classes, leaves)
    n_leaves = int(tree[3].max()) + 1
    out.update(tree=tree, member=member, items=items, n_leaves=n_leaves, fs=fs)
    leaf_of = [walk(tree, member, k, states) for k in items]
    lsums, lmu, lvar = np.zeros((n_leaves, sums.shape[1])), np.zeros((n_leaves, mu.shape[1])), np.zeros((n_leaves, mu.shape[1]))
    for i, k in enumerate(items):
        lsums[leaf_of[i]] += sums[i]
    for m in range(len(nodes)):                                            # every leaf starts from its root's monophone
        if tree[3][m] >= 0:
            root = m
            if m >= n_classes:
                k = items[nodes[m]["items"][0]]
                root = k[0] * states + k[1]
            lmu[tree[3][m]], lvar[tree[3][m]] = mu[root], var[root]
    mu, var = R.update(lsums, lmu, lvar, floor)
    lgraphs = [leaf_graph(g, phone_ids, states, out) for g in graphs]
    sums = lsums
    for _ in range(tri_iters):
        parts, total = [], 0.0
        for f, g in zip(fs, lgraphs):
            gamma, _, ll = R.posteriors(R.emissions(f, g["sid"], mu, var), g)
            parts.append(R.partials(gamma, f))
            total += ll
        sums = R.class_sums(parts, lgraphs, n_leaves)
        mu, var = R.update(sums, mu, var, floor)
        history.append((total + jac) / n_frames)
    out.update(mu=mu, var=var, history=history)
    if mixtures > 1:
        M, D = mixtures, mu.shape[1]
        w, gmu, gvar = np.zeros((n_leaves, M)), np.zeros((n_leaves, M, D)), np.ones((n_leaves, M, D))
        w[:, 0], gmu[:, 0], gvar[:, 0] = 1.0, mu, var
        ncomp, occ = np.ones(n_leaves, np.int64), np.zeros((n_leaves, M))
        occ[:, 0] = sums[:, 0]
        for step in range(1, M):
            w, gmu, gvar, ncomp = GR.split(w, gmu, gvar, ncomp, occ, step, min_split_occ)
            for _ in range(mix_iters):
                parts, total = [], 0.0
                for f, g in zip(fs, lgraphs):
                    E, r = GR.emissions(f, g["sid"], w, gmu, gvar)
                    gamma, _, ll = R.posteriors(E, g)
                    parts.append(GR.partials(gamma, r, f))
                    total += ll
                msums = GR.class_sums(parts, lgraphs, n_leaves)
                occ = msums[:, :, 0]
                w, gmu, gvar = GR.update(msums, w, gmu, gvar, ncomp, floor)
                history.append((total + jac) / n_frames)
        out.update(w=w, gmu=gmu, gvar=gvar, ncomp=ncomp)
    return out


def align(f, graph, model):
    """frames per block of one utterance from the feature f the stage saw (x, or the output of the stages in front)"""
    if "tree" in model:
        graph = leaf_graph(graph, model["phone_ids"], model["states"], model)
    if "w" in model:
        return GR.align(f, graph, model["w"], model["gmu"], model["gvar"])
    return R.align(f, graph, model["mu"], model["var"])
