"""A seeded multi-speaker corpus for the speaker-similarity tests, in the manner of tests/align_fmllr_corpus.py.

`corpus(seed)`: N_SPEAKERS speakers, N_TRAIN training and N_HELD held-out utterances each, of about 100 frames.  A frame is the
mean of one of 6 sound classes (smooth over the 80 channels: 12 low DCT components, so that the few cepstra the features keep see
them) plus white noise, in segments of 1 to 3 frames (short, so that
the statistics of an utterance of 100 frames are steady); 3 to 6 frames of silence (every channel 5 lower: under the energy floor)
open and close an utterance.  Every frame of speaker s then passes through that speaker's fixed dense matrix M_s = I + EPSILON R_s
(R_s has N(0, 1 / N_MEL) entries, one fixed seed for every corpus seed): a constant shift per speaker would not do, the
per-utterance normalisation of the feature step cancels it.  The 80-channel matrix stands where the log-mel spectrogram stands in
the product.  EPSILON was chosen on the host with the numpy oracle (tests/golden/make_spk_bars.py): the smallest of 0.5, 1, 2, 3
at which the oracle identifies every held-out utterance on the seeds 4321, 17 and 99.

`wav_corpus(root, seed)`: the same idea as audio for the command-line test: a sound is a mixture of four sinusoids, a speaker a fixed
set of gains on them and a pitch factor; 16-bit PCM at 22050 Hz under `{root}/raw/{speaker}/{name}.wav`."""
import os

import numpy as np

N_MEL, N_SPEAKERS, N_TRAIN, N_HELD, N_CLASSES = 80, 6, 8, 3, 6
EPSILON, NOISE, SILENCE = 2.0, 0.1, 5.0
M, N_CEP, ITERS = 8, 5, 2
DUR = (1, 3)                                                               # frames per segment
SEEDS = (4321, 17, 99)
SR, HOP = 22050, 256


def distortions(epsilon=EPSILON):
    """(N_SPEAKERS, N_MEL, N_MEL): the same for every corpus seed"""
    rng = np.random.RandomState(2424)
    return np.eye(N_MEL)[None] + epsilon * rng.randn(N_SPEAKERS, N_MEL, N_MEL) / np.sqrt(N_MEL)


def _basis():
    k = np.arange(12)[:, None]
    m = np.arange(N_MEL)[None, :]
    return np.cos(np.pi * k * (2 * m + 1) / (2 * N_MEL))


def _base(rng, means):
    """one undistorted utterance (T, N_MEL) of about 100 frames"""
    rows = [np.full((rng.randint(3, 7), N_MEL), -SILENCE)]
    n = 0
    while n < 90:
        d = rng.randint(DUR[0], DUR[1] + 1)
        rows.append(np.tile(means[rng.randint(N_CLASSES)], (d, 1)))
        n += d
    rows.append(np.full((rng.randint(3, 7), N_MEL), -SILENCE))
    x = np.concatenate(rows)
    return x + NOISE * rng.randn(*x.shape)


def corpus(seed, epsilon=None):
    """-> (train, held): lists of dict(speaker, base (T, 80) float64, mel (80, T) float32), speakers in turn"""
    D = distortions(EPSILON if epsilon is None else epsilon)
    rng = np.random.RandomState(seed)
    means = 1.5 + (rng.randn(N_CLASSES, 12) / np.sqrt(1 + np.arange(12))) @ _basis()
    sets = []
    for n in (N_TRAIN, N_HELD):
        utts = []
        for _ in range(n):
            for s in range(N_SPEAKERS):
                base = _base(rng, means)
                utts.append({"speaker": s, "base": base, "mel": distort(base, D[s])})
        sets.append(utts)
    return sets


def distort(base, matrix):
    return (base @ matrix.T).T.astype(np.float32)


def wav_corpus(root, seed, speakers=("spa", "spb", "spc"), n_train=4, n_held=2):
    """Writes {root}/raw/{speaker}/{name}.wav -> (train [(name, speaker)], held [(name, speaker)])"""
    from scipy.io import wavfile
    rng = np.random.RandomState(seed)
    sounds = [(np.sort(rng.uniform(150, 3500, 4)), rng.uniform(0.3, 1.0, 4)) for _ in range(8)]
    voices = {s: (rng.uniform(0.85, 1.2), np.exp(1.2 * rng.randn(4))) for s in speakers}
    out = []
    for kind, n in (("tr", n_train), ("he", n_held)):
        names = []
        for s in speakers:
            os.makedirs(os.path.join(root, "raw", s), exist_ok=True)
            pitch, gains = voices[s]
            for u in range(n):
                parts = [1e-3 * rng.randn(4 * HOP)]
                for _ in range(10):
                    fr, am = sounds[rng.randint(len(sounds))]
                    k = np.arange(rng.randint(6, 14) * HOP)
                    tone = sum(a * g * np.sin(2 * np.pi * f * pitch * k / SR) for f, a, g in zip(fr, am, gains))
                    parts.append(0.2 * tone / (am * gains).sum() + 2e-3 * rng.randn(len(k)))
                parts.append(1e-3 * rng.randn(4 * HOP))
                name = f"{s}_{kind}{u:02d}"
                wavfile.write(os.path.join(root, "raw", s, name + ".wav"), SR, np.round(np.concatenate(parts) * 32767).astype(np.int16))
                names.append((name, s))
        out.append(names)
    return out
