"""float64 numpy oracle of the forced aligner's trained transition and optional-silence probabilities, written from the "Transitions"
paragraph of the specification in fastspeech2_amd/align.py's docstring (not from the kernels, and without the product's host code):
the kinds of the optional blocks, the arc costs, forward / backward / the arc posteriors xi / Viterbi under the costs, the update,
and `fit`: the monophone passes, then optionally the triphone stage and the mixture stages, every Baum-Welch pass under the current
costs and followed by the update.  Emissions, statistics and the Gaussian updates are those of tests/align_ref.py and
tests/align_gmm_ref.py, the tree is grown with the functions of tests/align_tri_ref.py.  One utterance at a time, loops over frames."""
import numpy as np

from tests import align_gmm_ref as GR
from tests import align_ref as R
from tests import align_tri_ref as TR

NINF = -np.inf
FLOOR = 0.01


def kinds(graph):
    """per block: -1 mandatory, 0 optional and first, 2 optional and last, 1 any other optional block"""
    out = []
    for k, (_, _, optional) in enumerate(graph["blocks"]):
        out.append(-1 if not optional else (0 if k == 0 else (2 if k == len(graph["blocks"]) - 1 else 1)))
    return out


def first_states(graph):
    """the first state of every block"""
    block = list(graph["block"])
    return [j for j in range(len(block)) if j == 0 or block[j] != block[j - 1]]


def arc_costs(graph, loop, opt):
    """-> (w [3][J], edge [4])"""
    sid, skip, block, alt = graph["sid"], graph["skip"], graph["block"], graph["alt"]
    J, kind, first = len(sid), kinds(graph), set(first_states(graph))
    w, edge = np.zeros((3, J)), np.zeros(4)
    for j in range(J):
        w[0, j] = np.log(loop[sid[j]])
        if j >= 1:
            w[1, j] = np.log(1.0 - loop[sid[j - 1]])
            if j in first and kind[block[j]] >= 0:
                w[1, j] += np.log(opt[kind[block[j]]])
        if skip[j] >= 0:
            w[2, j] = np.log(1.0 - loop[sid[skip[j]]]) + np.log(1.0 - opt[kind[block[j] - 1]])
    edge[0] = np.log(opt[0]) if kind[0] == 0 else 0.0
    edge[1] = np.log(1.0 - opt[0])
    edge[2] = np.log(1.0 - loop[sid[J - 1]])
    if alt[1] >= 0:
        edge[3] = np.log(1.0 - loop[sid[alt[1]]]) + np.log(1.0 - opt[2])
    return w, edge


def start_edges(graph, edge):
    """[(state, cost)] of the start states"""
    return [(0, edge[0])] + ([(graph["alt"][0], edge[1])] if graph["alt"][0] >= 0 else [])


def end_edges(graph, edge):
    """[(state, cost)] of the end states, in index order"""
    J = len(graph["sid"])
    return ([(graph["alt"][1], edge[3])] if graph["alt"][1] >= 0 else []) + [(J - 1, edge[2])]


def _pred(row, skip, w):
    """the three predecessor values of every state with their arc costs: self, next (j - 1), skip"""
    nxt = np.concatenate([[NINF], row[:-1]]) + w[1]
    skp = np.where(skip >= 0, row[np.maximum(skip, 0)] + w[2], NINF)
    return row + w[0], nxt, skp


def forward(E, graph, w, edge):
    T, J = E.shape
    alpha = np.full((T, J), NINF)
    for j, c in start_edges(graph, edge):
        alpha[0, j] = c + E[0, j]
    for t in range(1, T):
        alpha[t] = E[t] + R.lse(*_pred(alpha[t - 1], graph["skip"], w))
    return alpha, float(R.lse(*[alpha[T - 1, j] + c for j, c in end_edges(graph, edge)]))


def backward(E, graph, w, edge):
    T, J = E.shape
    to = np.full(J, -1)
    for j, s in enumerate(graph["skip"]):
        if s >= 0:
            to[s] = j
    beta = np.full((T, J), NINF)
    for j, c in end_edges(graph, edge):
        beta[T - 1, j] = c
    for t in range(T - 2, -1, -1):
        eb = E[t + 1] + beta[t + 1]
        beta[t] = R.lse(eb + w[0], np.concatenate([eb[1:] + w[1, 1:], [NINF]]),
                        np.where(to >= 0, eb[np.maximum(to, 0)] + w[2, np.maximum(to, 0)], NINF))
    return beta


def posteriors(E, graph, w, edge):
    """-> (gamma [T][J], xi [J][5]: self, next, skip, start mass, end mass; alpha; loglik)"""
    T, J = E.shape
    alpha, ll = forward(E, graph, w, edge)
    beta = backward(E, graph, w, edge)
    with np.errstate(invalid="ignore"):
        gamma = np.exp(alpha + beta - ll)
    gamma = np.where(np.isnan(gamma), 0.0, gamma)
    xi = np.zeros((J, 5))
    if T > 1:                                                              # all frames at once: row t - 1 holds the transition into frame t
        prev, skip = alpha[:-1], graph["skip"]
        preds = (prev + w[0], np.concatenate([np.full((T - 1, 1), NINF), prev[:, :-1]], axis=1) + w[1],
                 np.where(skip >= 0, prev[:, np.maximum(skip, 0)] + w[2], NINF))
        with np.errstate(invalid="ignore"):
            for a, p in enumerate(preds):
                term = np.exp(p + E[1:] + beta[1:] - ll)
                xi[:, a] = np.where(np.isnan(term), 0.0, term)[::-1].sum(axis=0)
    xi[:, 3], xi[:, 4] = gamma[0], gamma[T - 1]
    return gamma, xi, alpha, ll


def viterbi(E, graph, w, edge):
    """-> (backpointers uint8 [T][J], end state, frames per block, score)"""
    T, J = E.shape
    skip = graph["skip"]
    delta = np.full(J, NINF)
    for j, c in start_edges(graph, edge):
        delta[j] = c + E[0, j]
    bp = np.zeros((T, J), np.uint8)
    for t in range(1, T):
        own, nxt, skp = _pred(delta, skip, w)
        best, code = own.copy(), np.zeros(J, np.uint8)
        for c, cand in ((1, nxt), (2, skp)):                               # a later code wins only when strictly larger
            better = cand > best
            best, code = np.where(better, cand, best), np.where(better, c, code).astype(np.uint8)
        delta, bp[t] = E[t] + best, code
    end, score = None, NINF
    for j, c in end_edges(graph, edge):                                    # the lower index wins ties
        if end is None or delta[j] + c > score:
            end, score = j, delta[j] + c
    frames = np.zeros(len(graph["blocks"]), np.int32)
    j = end
    for t in range(T - 1, -1, -1):
        frames[graph["block"][j]] += 1
        if t:
            j = (j, j - 1, skip[j])[bp[t, j]]
    return bp, end, frames, score


def opt_masses(xi, graph):
    """-> (enter [3], skipped [3]) of one utterance"""
    enter, skipped = np.zeros(3), np.zeros(3)
    first, alt = first_states(graph), graph["alt"]
    for k, kind in enumerate(kinds(graph)):
        if kind == 0:
            enter[0] += xi[0, 3]
            skipped[0] += xi[alt[0], 3]
        elif kind == 1:
            enter[1] += xi[first[k], 1]
            skipped[1] += xi[first[k + 1], 2]
        elif kind == 2:
            enter[2] += xi[first[k], 1]
            skipped[2] += xi[alt[1], 4]
    return enter, skipped


def clip(p):
    return min(max(p, FLOOR), 1.0 - FLOOR)


def update(n, s, enter, skipped, loop, opt):
    loop, opt = np.array(loop, dtype=np.float64), np.array(opt, dtype=np.float64)
    for c in range(len(loop)):
        if n[c] >= 1.0:
            loop[c] = clip(s[c] / n[c])
    for k in range(3):
        if enter[k] + skipped[k] >= 1.0:
            opt[k] = clip(enter[k] / (enter[k] + skipped[k]))
    return loop, opt


def _pass(fs, graphs, n_classes, loop, opt, emit, partials):
    """one Baum-Welch pass: emit(f, sid) -> (E, whatever `partials(gamma, extra, f)` needs) -> (partials per utterance, the class sums
    of xi[:, self], enter, skipped, the total log-likelihood)"""
    parts, total, s, enter, skipped = [], 0.0, np.zeros(n_classes), np.zeros(3), np.zeros(3)
    for f, g in zip(fs, graphs):
        E, extra = emit(f, g["sid"])
        gamma, xi, _, ll = posteriors(E, g, *arc_costs(g, loop, opt))
        parts.append(partials(gamma, extra, f))
        np.add.at(s, g["sid"], xi[:, 0])
        e, k = opt_masses(xi, g)
        enter, skipped, total = enter + e, skipped + k, total + ll
    return parts, s, enter, skipped, total


def fit_mono(xs, graphs, n_classes, iters):
    """Flat start (unchanged) and `iters` passes -> dict(mu, var, loop, opt, history, sums: the class sums of the last pass, floor)"""
    allx = np.concatenate(xs)
    g_mean, g_var = allx.mean(axis=0), allx.var(axis=0)
    floor = 1e-2 * g_var
    sums = R.class_sums([R.partials(R.flat_gamma(g, len(x)), x) for x, g in zip(xs, graphs)], graphs, n_classes)
    mu, var = R.update(sums, np.tile(g_mean, (n_classes, 1)), np.tile(g_var, (n_classes, 1)), floor)
    loop, opt, history, n_frames = np.full(n_classes, 0.5), np.full(3, 0.5), [], sum(len(x) for x in xs)
    for _ in range(iters):
        parts, s, enter, skipped, total = _pass(xs, graphs, n_classes, loop, opt, lambda f, sid: (R.emissions(f, sid, mu, var), None),
                                                lambda gamma, _, f: R.partials(gamma, f))
        sums = R.class_sums(parts, graphs, n_classes)
        mu, var = R.update(sums, mu, var, floor)
        loop, opt = update(sums[:, 0], s, enter, skipped, loop, opt)
        history.append(total / n_frames)
    return {"mu": mu, "var": var, "loop": loop, "opt": opt, "history": history, "sums": sums, "floor": floor}


def fit(xs, graphs, n_classes, iters, mixtures=1, mix_iters=4, min_split_occ=40.0, leaves=0, tri_iters=4, min_occ=100.0, phone_ids=None,
        states=2, front=None):
    """The schedule with transitions -> dict(mu, var, loop, opt, history, graphs: the graphs the last stage decodes on and, with
    mixtures > 1, w, gmu, gvar, ncomp; with leaves > 0, tree, member, n_leaves).  `front` = the result of `fit_mono` on the same
    corpus replaces the monophone passes."""
    m = dict(front) if front is not None else fit_mono(xs, graphs, n_classes, iters)
    mu, var, loop, opt, history, sums, floor = m["mu"], m["var"], m["loop"], m["opt"], list(m["history"]), m["sums"], m["floor"]
    n_frames = sum(len(x) for x in xs)
    out = {"graphs": graphs}
    if leaves:
        ctxs = [TR.contexts(g, phone_ids, states) for g in graphs]
        items = TR.item_table(ctxs)
        parts, total = [], 0.0
        for x, g in zip(xs, graphs):                                       # the statistics pass: current costs, nothing updated
            gamma, _, _, ll = posteriors(R.emissions(x, g["sid"], mu, var), g, *arc_costs(g, loop, opt))
            parts.append(R.partials(gamma, x))
            total += ll
        history.append(total / n_frames)
        isums = TR.item_sums(parts, ctxs, items)
        fixed = {phone_ids[p] * states + s for p in TR.CI for s in range(states)}
        mono = np.zeros((n_classes, isums.shape[1]))
        for i, k in enumerate(items):
            mono[k[0] * states + k[1]] += isums[i]
        member = TR.questions(mono, [p for p in range(len(phone_ids)) if p * states not in fixed], states, floor, len(phone_ids) + 1)
        nodes = TR.grow(items, states, len(phone_ids), fixed, isums, member, floor, min_occ, 0.0)
        tree = TR.replay(nodes, n_classes, leaves)
        n_leaves = int(tree[3].max()) + 1
        model = {"tree": tree, "member": member}
        leaf_of = [TR.walk(tree, member, k, states) for k in items]
        lsums, lmu, lvar, lloop = np.zeros((n_leaves, isums.shape[1])), np.zeros((n_leaves, mu.shape[1])), np.zeros((n_leaves, mu.shape[1])), np.zeros(n_leaves)
        for i in range(len(items)):
            lsums[leaf_of[i]] += isums[i]
        for node in range(len(nodes)):                                     # every leaf starts from its root's monophone
            if tree[3][node] >= 0:
                root = node
                if node >= n_classes:
                    k = items[nodes[node]["items"][0]]
                    root = k[0] * states + k[1]
                lmu[tree[3][node]], lvar[tree[3][node]], lloop[tree[3][node]] = mu[root], var[root], loop[root]
        mu, var = R.update(lsums, lmu, lvar, floor)
        loop, n_classes, sums = lloop, n_leaves, lsums
        graphs = [TR.leaf_graph(g, phone_ids, states, model) for g in graphs]
        for _ in range(tri_iters):
            parts, s, enter, skipped, total = _pass(xs, graphs, n_classes, loop, opt, lambda f, sid: (R.emissions(f, sid, mu, var), None),
                                                    lambda gamma, _, f: R.partials(gamma, f))
            sums = R.class_sums(parts, graphs, n_classes)
            mu, var = R.update(sums, mu, var, floor)
            loop, opt = update(sums[:, 0], s, enter, skipped, loop, opt)
            history.append(total / n_frames)
        out.update(tree=tree, member=member, n_leaves=n_leaves, graphs=graphs)
    if mixtures > 1:
        M, D = mixtures, mu.shape[1]
        w, gmu, gvar = np.zeros((n_classes, M)), np.zeros((n_classes, M, D)), np.ones((n_classes, M, D))
        w[:, 0], gmu[:, 0], gvar[:, 0] = 1.0, mu, var
        ncomp, occ = np.ones(n_classes, np.int64), np.zeros((n_classes, M))
        occ[:, 0] = sums[:, 0]
        for step in range(1, M):
            w, gmu, gvar, ncomp = GR.split(w, gmu, gvar, ncomp, occ, step, min_split_occ)
            for _ in range(mix_iters):
                parts, s, enter, skipped, total = _pass(xs, graphs, n_classes, loop, opt, lambda f, sid: GR.emissions(f, sid, w, gmu, gvar),
                                                        GR.partials)
                msums = GR.class_sums(parts, graphs, n_classes)
                occ = msums[:, :, 0]
                w, gmu, gvar = GR.update(msums, w, gmu, gvar, ncomp, floor)
                n_c = np.array([sum(occ[c, k] for k in range(int(ncomp[c]))) for c in range(n_classes)])
                loop, opt = update(n_c, s, enter, skipped, loop, opt)
                history.append(total / n_frames)
        out.update(w=w, gmu=gmu, gvar=gvar, ncomp=ncomp)
    out.update(mu=mu, var=var, loop=loop, opt=opt, history=history)
    return out


def align(x, graph, model):
    """frames per block of one utterance; `graph` is the graph of the last stage (`model["graphs"]`)"""
    E = GR.emissions(x, graph["sid"], model["w"], model["gmu"], model["gvar"])[0] if "w" in model else \
        R.emissions(x, graph["sid"], model["mu"], model["var"])
    return viterbi(E, graph, *arc_costs(graph, model["loop"], model["opt"]))[2]
