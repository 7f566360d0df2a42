"""float64 numpy oracle of the aligner's confidence scores, written from the "Confidence" paragraph of fastspeech2_amd/align.py's
docstring (not from the kernels): the class scores F, own / best / arg per frame, the Viterbi path from backpointers, the block and
utterance means, and the phone of every class.  Tables are the mixture tables w (C, M), mu, var (C, M, D); a single-Gaussian table
(C, D) is M = 1 with w = 1 (`as_mixture`)."""
import numpy as np

NINF = -np.inf


def as_mixture(mu, var):
    """(C, D) tables -> w (C, 1) = 1, mu, var (C, 1, D)"""
    return np.ones((mu.shape[0], 1)), mu[:, None, :], var[:, None, :]


def class_scores(f, w, mu, var):
    """F (T, C): per component N = log w - 1/2 sum_d ((f_d - mu_d)^2 / var_d + log(2 pi var_d)), d ascending; F = mx + log(sum_m
    exp(N_m - mx)) over ascending m, mx the maximum; a component of weight 0 contributes -inf."""
    T, (C, M, D) = f.shape[0], mu.shape
    acc = np.zeros((T, C, M))
    for d in range(D):                                                     # ascending d
        acc = acc + ((f[:, None, None, d] - mu[None, :, :, d]) ** 2 / var[None, :, :, d] + np.log(2.0 * np.pi * var[None, :, :, d]))
    with np.errstate(divide="ignore"):
        N = np.log(w)[None] - 0.5 * acc
    mx = N.max(axis=2)
    safe = np.where(mx == NINF, 0.0, mx)
    s = np.zeros((T, C))
    for m in range(M):                                                     # ascending m
        s = s + np.exp(N[:, :, m] - safe)
    with np.errstate(divide="ignore"):
        return np.where(mx == NINF, NINF, safe + np.log(s))


def frame_scores(F, cls):
    """-> (own, best, arg, margin): own[t] = F[t, cls[t]] (NaN for a class outside the table), best = max_c, arg = the lowest c that
    attains it, margin = best - the runner-up (inf with one class)."""
    T, C = F.shape
    cls = np.asarray(cls)
    ok = (cls >= 0) & (cls < C)
    own = np.where(ok, F[np.arange(T), np.where(ok, cls, 0)], np.nan)
    arg = np.argmax(F, axis=1)                                             # the first of the largest
    best = F[np.arange(T), arg]
    rest = F.copy()
    rest[np.arange(T), arg] = NINF
    margin = best - rest.max(axis=1) if C > 1 else np.full(T, np.inf)
    return own, best, arg.astype(np.int32), margin


def path_states(bp, end, graph):
    """the state of every frame from the backpointers (T, J) and the end state: code 0 stays, 1 comes from j - 1, 2 from skip[j]; a
    chain that leaves the graph stops and the frames before it are -1"""
    T, J = bp.shape
    state = np.full(T, -1, np.int32)
    j = int(end) if 0 <= int(end) < J else -1
    for t in range(T - 1, -1, -1):
        state[t] = j
        if j < 0:
            break
        if t:
            j = (j, j - 1, int(graph["skip"][j]))[int(bp[t, j])] if bp[t, j] < 3 else -1
            if not 0 <= j < J:
                j = -1
    return state


def run_lengths(graph, state):
    """frames per block of a path"""
    return np.bincount(np.asarray(graph["block"])[state], minlength=len(graph["blocks"])).astype(np.int32)


def class_phone_mono(n_classes, states):
    return np.arange(n_classes) // states


def class_phone_tree(question, yes, no, leaf, n_roots, states):
    """the phone of every leaf: the phone of the root p S + s it descends from"""
    out = np.full(int(np.max(leaf)) + 1, -1)

    def down(node, phone):
        if leaf[node] >= 0:
            out[leaf[node]] = phone
        else:
            down(yes[node], phone), down(no[node], phone)
    for r in range(n_roots):
        down(r, r // states)
    return out


def reductions(graph, state, cls, own, best, arg, class_phone, viterbi):
    """-> dict(frames, viterbi, loglik, gop, match; blocks (n_blocks, 3) = (loglik, gop, match), NaN for a block without frames): the
    means over ascending t of own, own - best and [class_phone[arg] == the block's phone] per block, over the frames of the mandatory
    blocks (gop, match) and over all frames (loglik) per utterance."""
    T = len(state)
    blk = np.asarray(graph["block"])[state]
    blocks = np.full((len(graph["blocks"]), 3), np.nan)
    tot = [0.0, 0.0, 0.0, 0]
    ll = 0.0
    for k, (_, _, optional) in enumerate(graph["blocks"]):
        ts = np.nonzero(blk == k)[0]
        if not len(ts):
            continue
        assert np.array_equal(ts, np.arange(ts[0], ts[0] + len(ts)))      # a block's frames are consecutive
        phone = class_phone[cls[ts[0]]]                                    # the phone of the block: that of any of its classes
        a = g = h = 0.0
        for t in ts:                                                       # ascending t
            a += own[t]
            g += own[t] - best[t]
            h += float(class_phone[arg[t]] == phone)
        blocks[k] = (a / len(ts), g / len(ts), h / len(ts))
    for t in range(T):
        ll += own[t]
        if not graph["blocks"][blk[t]][2]:
            tot[1] += own[t] - best[t]
            tot[2] += float(class_phone[arg[t]] == class_phone[cls[t]])
            tot[3] += 1
    return {"frames": T, "viterbi": viterbi / T, "loglik": ll / T, "gop": tot[1] / tot[3], "match": tot[2] / tot[3], "blocks": blocks}


def score(f, graph, w, mu, var, class_phone, decode):
    """One utterance end to end: F, the emissions E[t, j] = F[t, sid[j]], `decode(E, graph)` -> (backpointers, end state, frames per
    block, Viterbi score), the path, the reductions -> (frames per block, reductions dict, (state, own, best, arg, margin))."""
    F = class_scores(f, w, mu, var)
    bp, end, frames, vit = decode(F[:, graph["sid"]], graph)
    state = path_states(bp, end, graph)
    assert np.array_equal(run_lengths(graph, state), frames)
    cls = np.asarray(graph["sid"])[state]
    own, best, arg, margin = frame_scores(F, cls)
    return frames, reductions(graph, state, cls, own, best, arg, class_phone, vit), (state, own, best, arg, margin)


def plain_decode(E, graph):
    """`align_ref.viterbi` with the path's score (all arcs cost 0)"""
    from tests import align_ref as R
    bp, end, frames = R.viterbi(E, graph)
    states = path_states(bp, end, graph)
    vit = float(np.sum(E[np.arange(len(states)), states]))
    return bp, end, frames, vit


def block_mean(red, frames, blocks, col=1):
    """the frame-weighted mean of column `col` (1 = gop) of the reductions over the listed blocks that have frames"""
    ks = [k for k in blocks if frames[k] > 0]
    return sum(red["blocks"][k, col] * frames[k] for k in ks) / sum(frames[k] for k in ks)
