"""fp64 numpy oracle of probabilistic YIN, written from the specification in the docstring of fastspeech2_amd/pyin.py, stage by stage:
`cmnd`, `observe`, `viterbi`, `pyin`.  It shares no code with fastspeech2_amd/pyin.py; the defaults below are read off that
docstring.  Besides the results it reports what the GPU tests need to know about their own inputs: which frames sit on a rounding
boundary (`observe`) and by how much the best path wins (`viterbi`)."""
import math

import numpy as np

FMIN, FMAX, FRAME_LENGTH, N_THRESHOLDS, BETA_AB, NO_TROUGH_PROB = 71.0, 800.0, 2048, 100, (2, 18), 0.01
BINS_PER_SEMITONE, MAX_TRANSITION_RATE, SWITCH_PROB = 20, 35.92, 0.01


def half_up(v):
    return int(np.floor(v + 0.5))


def frame_count(n, fs, frame_period):
    return 1 + int(n / fs / (frame_period / 1000))


def geometry(fs, frame_period, fmin=FMIN, fmax=FMAX, frame_length=FRAME_LENGTH, bins_per_semitone=BINS_PER_SEMITONE,
             max_transition_rate=MAX_TRANSITION_RATE):
    hop = half_up(frame_period / 1000.0 * fs)
    W = frame_length // 2
    bo = 12 * bins_per_semitone
    return dict(hop=hop, L=frame_length, W=W, tmin=int(np.floor(fs / fmax)), tmax=min(int(np.ceil(fs / fmin)), frame_length - W - 1),
                bo=bo, nb=int(np.floor(bo * np.log2(fmax / fmin))) + 1,
                h=half_up(max_transition_rate * 12 * hop / fs) * (bins_per_semitone // 2))


# ------------------------------------------------------------------------------------------------ stage 1
def cmnd(x, fs, frame_period, fmin=FMIN, fmax=FMAX, frame_length=FRAME_LENGTH):
    """x float32 (N,) -> d' (F, tau_max + 1) float64"""
    g = geometry(fs, frame_period, fmin, fmax, frame_length)
    hop, L, W, tmax = g["hop"], g["L"], g["W"], g["tmax"]
    N = len(x)
    F = frame_count(N, fs, frame_period)
    xp = np.zeros((F - 1) * hop + L, np.float64)
    lo = L // 2                                                              # xp[n + L/2] = x[n]
    n = min(N, len(xp) - lo)
    xp[lo:lo + n] = np.asarray(x[:n], np.float64)
    X = np.lib.stride_tricks.sliding_window_view(xp, L)[::hop][:F]          # frame f: samples f hop - L/2 .. + L - 1
    d = np.empty((F, tmax + 1))
    for tau in range(tmax + 1):
        d[:, tau] = ((X[:, :W] - X[:, tau:tau + W]) ** 2).sum(axis=1)
    out = np.ones_like(d)
    csum = np.cumsum(d[:, 1:], axis=1)
    taus = np.arange(1, tmax + 1, dtype=np.float64)
    ok = csum != 0
    out[:, 1:][ok] = (d[:, 1:] * taus[None, :])[ok] / csum[ok]
    return out


# ------------------------------------------------------------------------------------------------ stage 2
def beta_weights(K=N_THRESHOLDS, ab=BETA_AB):
    a, b = ab
    n = a + b - 1

    def cdf(x):                                                              # 1 - P(fewer than a successes in n trials)
        return 1.0 - sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a))
    c = np.array([cdf(k / K) for k in range(K + 1)])
    return c[1:] - c[:-1]


def troughs(row, tmin, tmax):
    out = []
    for tau in range(tmin, tmax + 1):
        if tau == tmin:
            is_trough = row[tau] < row[tau + 1]
        elif tau == tmax:
            is_trough = row[tau] < row[tau - 1]
        else:
            is_trough = row[tau] < row[tau - 1] and row[tau] <= row[tau + 1]
        if is_trough:
            out.append(tau)
    return out


def refine(row, tau, tmin, tmax):
    if tau <= tmin or tau >= tmax:
        return 0.0
    a, b, c = row[tau - 1], row[tau], row[tau + 1]
    den = a - 2.0 * b + c
    return (a - c) / (2.0 * den) if den > 0 else 0.0


def observe_frame(row, fs, tmin, tmax, nb, bo, fmin, beta, no_trough_prob):
    """one d' row -> (obs row (2 nb,), p_v, boundary flag)"""
    K = len(beta)
    tr = troughs(row, tmin, tmax)
    gmin = tmin + int(np.argmin(row[tmin:tmax + 1]))                         # the first of equal minima
    voiced = np.zeros(nb)
    boundary = False
    if np.all(row[tmin:tmax + 1] == row[tmin]):                              # flat (digital silence): no minimum, no candidate
        return np.concatenate([voiced, np.full(nb, 1.0 / nb)]), 0.0, False

    def bin_of(tau):
        v = bo * np.log2(fs / (tau + refine(row, tau, tmin, tmax)) / fmin)
        near = abs((v - np.floor(v)) - 0.5) < 1e-9
        return min(max(half_up(v), 0), nb - 1), near
    used = {}
    for k in range(1, K + 1):
        s = k / K
        first = next((tau for tau in tr if row[tau] < s), None)
        tau, mass = (first, beta[k - 1]) if first is not None else (gmin, no_trough_prob * beta[k - 1])
        if tau not in used:
            used[tau] = bin_of(tau)
        b, near = used[tau]
        boundary |= near
        voiced[b] += mass
    for tau in tr:
        boundary |= bool(np.min(np.abs(row[tau] - np.arange(1, K + 1) / K)) < 1e-12)
    pv = min(voiced.sum(), 1.0)
    return np.concatenate([voiced, np.full(nb, (1.0 - pv) / nb)]), pv, boundary


def observe(dprime, fs, fmin=FMIN, fmax=FMAX, n_thresholds=N_THRESHOLDS, ab=BETA_AB, no_trough_prob=NO_TROUGH_PROB,
            bins_per_semitone=BINS_PER_SEMITONE):
    """d' (F, tau_max + 1) -> (obs (F, 2 nb), p_v (F,), boundary (F,) bool)"""
    tmax = dprime.shape[1] - 1
    tmin = int(np.floor(fs / fmax))
    bo = 12 * bins_per_semitone
    nb = int(np.floor(bo * np.log2(fmax / fmin))) + 1
    beta = beta_weights(n_thresholds, ab)
    rows = [observe_frame(r, fs, tmin, tmax, nb, bo, fmin, beta, no_trough_prob) for r in dprime]
    if not rows:
        return np.zeros((0, 2 * nb)), np.zeros(0), np.zeros(0, bool)
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], bool)


# ------------------------------------------------------------------------------------------------ stage 3
def log_transition(nb, h):
    """(log w(delta), delta = -h..h; log Z_i)"""
    w = np.array([h + 1.0 - abs(dl) for dl in range(-h, h + 1)])
    Z = np.array([sum(w[j - i + h] for j in range(max(0, i - h), min(nb - 1, i + h) + 1)) for i in range(nb)])
    return np.log(w), np.log(Z)


def _log(p):
    with np.errstate(divide="ignore"):
        return np.log(p)


def viterbi(obs, h, switch_prob=SWITCH_PROB):
    """obs (F, 2 nb) -> (states (F,) int, optimum log-likelihood, margin): margin = the least amount by which a choice on the way won,
    over the best final state against the second best and the chosen predecessor against the runner-up at every frame of the path."""
    F, S = obs.shape
    nb = S // 2
    logw, logz = log_transition(nb, h)
    lsw = np.array([_log(1.0 - switch_prob), _log(switch_prob)])
    lo = _log(obs)
    delta = -np.log(S) + lo[0]
    back = np.zeros((F, S), np.int64)
    gaps = np.full((F, S), np.inf)
    valid = np.zeros((nb, 2 * h + 1), bool)                                  # predecessor bin j - h + o inside [0, nb)
    for j in range(nb):
        valid[j, max(0, h - j):min(2 * h, nb - 1 - j + h) + 1] = True
    pred_bin = np.arange(nb)[:, None] - h + np.arange(2 * h + 1)[None, :]
    for t in range(1, F):
        pad = np.full((2, nb + 2 * h), -np.inf)
        pad[:, h:h + nb] = (delta - np.concatenate([logz, logz])).reshape(2, nb)
        win = np.lib.stride_tricks.sliding_window_view(pad, 2 * h + 1, axis=1) + logw[None, None, :]       # (v, j, o)
        new = np.empty(S)
        for v1 in (0, 1):
            cand = np.concatenate([win[0] + lsw[int(v1 != 0)], win[1] + lsw[int(v1 != 1)]], axis=1)                    # (j, [v = 0 offsets, v = 1 offsets])
            ok = np.concatenate([valid, valid], axis=1)
            cand = np.where(ok, cand, -np.inf)
            first_ok = np.argmax(ok, axis=1)
            best = np.argmax(cand, axis=1)                                   # the first of equal maxima
            val = cand[np.arange(nb), best]
            best = np.where(np.isneginf(val), first_ok, best)
            srt = np.sort(cand, axis=1)
            with np.errstate(invalid="ignore"):
                gap = srt[:, -1] - srt[:, -2]
            gaps[t, v1 * nb:(v1 + 1) * nb] = np.where(np.isnan(gap), 0.0, gap)
            v0 = best // (2 * h + 1)
            back[t, v1 * nb:(v1 + 1) * nb] = v0 * nb + pred_bin[np.arange(nb), best % (2 * h + 1)]
            new[v1 * nb:(v1 + 1) * nb] = lo[t, v1 * nb:(v1 + 1) * nb] + val
        delta = new
    s = int(np.argmax(delta))
    top = np.sort(delta)
    with np.errstate(invalid="ignore"):
        margin = top[-1] - top[-2] if S > 1 else np.inf
    margin = 0.0 if np.isnan(margin) else margin
    states = np.empty(F, np.int64)
    for t in range(F - 1, -1, -1):
        states[t] = s
        if t:
            margin = min(margin, gaps[t, s])
            s = int(back[t, s])
    return states, float(np.max(delta)), float(margin)


def log_likelihood(states, obs, h, switch_prob=SWITCH_PROB):
    """log P(path, observations) of any state path under the model, term by term"""
    F, S = obs.shape
    nb = S // 2
    logw, logz = log_transition(nb, h)
    total = -math.log(S) + float(_log(obs[0, states[0]]))
    for t in range(1, F):
        (v0, i), (v1, j) = divmod(int(states[t - 1]), nb), divmod(int(states[t]), nb)
        if abs(j - i) > h:
            return -math.inf
        total += logw[j - i + h] - logz[i] + float(_log(switch_prob if v0 != v1 else 1.0 - switch_prob)) + float(_log(obs[t, states[t]]))
    return total


def states_to_f0(states, nb, bo, fmin=FMIN):
    states = np.asarray(states)
    return np.where(states < nb, fmin * 2.0 ** ((states % nb) / bo), 0.0)


# ------------------------------------------------------------------------------------------------ all of it
def pyin(x, fs, frame_period, fmin=FMIN, fmax=FMAX, frame_length=FRAME_LENGTH, full=False):
    """x float32 (N,) -> (f0 (F,), voiced probability (F,), t (F,)); with `full` a dict of every stage's output as well"""
    g = geometry(fs, frame_period, fmin, fmax, frame_length)
    d = cmnd(x, fs, frame_period, fmin, fmax, frame_length)
    obs, pv, boundary = observe(d, fs, fmin, fmax)
    states, ll, margin = viterbi(obs, g["h"])
    f0 = states_to_f0(states, g["nb"], g["bo"], fmin)
    t = np.arange(len(f0)) * frame_period / 1000.0
    if full:
        return f0, pv, t, dict(dprime=d, obs=obs, boundary=boundary, states=states, loglik=ll, margin=margin, **g)
    return f0, pv, t
