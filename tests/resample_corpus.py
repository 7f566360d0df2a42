"""Tiny synthetic corpus trees in the three layouts `fastspeech2_amd.prepare_align` walks (tests/test_resample_cpu.py,
tests/test_resample_gpu.py), synthesised from tests/f0_signals.py and seeded noise; plus the reference pipeline as an `audio_fn`."""
import os

import numpy as np
from scipy.io import wavfile

from tests import f0_signals as S
from tests.resample_ref import peaknorm_ref, resample_ref


def config(dataset, corpus, raw, sampling_rate=22050, cleaners=("english_cleaners",)):
    return {"dataset": dataset, "path": {"corpus_path": corpus, "raw_path": raw},
            "preprocessing": {"audio": {"sampling_rate": sampling_rate, "max_wav_value": 32768.0},
                              "text": {"text_cleaners": list(cleaners)}}}


def _signal(kind, sr, dur, seed):
    rng = np.random.default_rng(seed)
    if kind == "tone":
        x = S.tone(150.0 + 10 * seed, dur=dur, fs=sr)
    elif kind == "glide":
        x = S.glide(dur=dur, fs=sr)[0]
    else:
        x = 0.2 * rng.standard_normal(int(dur * sr)).astype(np.float32)
    return np.asarray(x, dtype=np.float32) + 0.01 * rng.standard_normal(len(x)).astype(np.float32)


def _write(path, sr, x):
    """int16 PCM file; returns what load_wav reads back from it (float32 in [-1, 1))"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    pcm = (np.clip(x, -1, 1) * 32767).astype(np.int16)
    wavfile.write(path, sr, pcm)
    return pcm.astype(np.float32) / 32768.0


def ref_audio_fn(wavs, sr_in, sr_out, max_wav_value):
    """the reference pipeline: float32(resample_ref(x)) -> numpy float32 y / max|y| * max_wav_value -> astype(int16)"""
    return [peaknorm_ref(resample_ref(w, sr_in, sr_out).astype(np.float32), max_wav_value) for w in wavs]


def make_ljspeech(root, sr=22050):
    """-> (config, {out_wav: (source float32, source rate)}, {out_lab: text}); LJ001-0003 has no wav"""
    corpus, raw = os.path.join(root, "LJSpeech-1.1"), os.path.join(root, "raw_lj")
    os.makedirs(corpus, exist_ok=True)
    lines = [("LJ001-0001", "Printing, in the only sense", "Printing, in the   only sense"),
             ("LJ001-0002", "raw two", "In Being Comparatively Modern."),
             ("LJ001-0003", "raw three", "this one has no audio")]
    with open(os.path.join(corpus, "metadata.csv"), "w", encoding="utf-8") as f:
        for ln in lines:
            f.write("|".join(ln) + "\n")
    wavs, labs = {}, {}
    for k, (name, _, norm) in enumerate(lines[:2]):
        x = _write(os.path.join(corpus, "wavs", name + ".wav"), sr, _signal(("tone", "noise")[k], sr, 0.21 + 0.1 * k, k))
        wavs[os.path.join(raw, "LJSpeech", name + ".wav")] = (x, sr)
        labs[os.path.join(raw, "LJSpeech", name + ".lab")] = " ".join(norm.lower().split())
    return config("LJSpeech", corpus, raw), wavs, labs


def make_libritts(root, sr=24000, other_sr=16000, dur=0.3):
    """two speakers, three chapters, four utterances (one at `other_sr`: batches must not mix it with the rest), a stray file"""
    corpus, raw = os.path.join(root, "LibriTTS", "train-clean-100"), os.path.join(root, "raw_libri")
    plan = [("19", "198", "19_198_000000_000000", "tone", sr, "Northanger Abbey"),
            ("19", "198", "19_198_000001_000002", "glide", sr, "This little work was finished."),
            ("19", "227", "19_227_000003_000001", "noise", other_sr, "a  SECOND chapter"),
            ("26", "495", "26_495_000004_000000", "tone", sr, "Another speaker")]
    wavs, labs = {}, {}
    for k, (spk, chap, name, kind, rate, text) in enumerate(plan):
        folder = os.path.join(corpus, spk, chap)
        x = _write(os.path.join(folder, name + ".wav"), rate, _signal(kind, rate, dur + 0.07 * k, 10 + k))
        with open(os.path.join(folder, name + ".normalized.txt"), "w") as f:
            f.write(text + "\n")
        with open(os.path.join(folder, name + ".original.txt"), "w") as f:
            f.write("not read\n")
        wavs[os.path.join(raw, spk, name + ".wav")] = (x, rate)
        labs[os.path.join(raw, spk, name + ".lab")] = " ".join(text.lower().split())
    with open(os.path.join(corpus, "19", "198", "19_198.trans.tsv"), "w") as f:
        f.write("stray\n")
    return config("LibriTTS", corpus, raw), wavs, labs


def make_aishell3(root, sr=44100):
    """train and test splits, two speakers; SSB00050003.wav is listed but absent"""
    corpus, raw = os.path.join(root, "AISHELL-3"), os.path.join(root, "raw_aishell")
    plan = {"train": [("SSB00050001.wav", "广 guang3 州 zhou1 女 nv3", True), ("SSB00050003.wav", "大 da4 学 xue2", False)],
            "test": [("SSB00090002.wav", "生 sheng1 登 deng1 上 shang4", True)]}
    wavs, labs = {}, {}
    k = 0
    for split, rows in plan.items():
        os.makedirs(os.path.join(corpus, split), exist_ok=True)
        with open(os.path.join(corpus, split, "content.txt"), "w", encoding="utf-8") as f:
            for wav_name, text, present in rows:
                f.write(wav_name + "\t" + text + "\n")
                if not present:
                    continue
                spk = wav_name[:7]
                x = _write(os.path.join(corpus, split, "wav", spk, wav_name), sr, _signal(("tone", "noise")[k % 2], sr, 0.2 + 0.05 * k, 20 + k))
                wavs[os.path.join(raw, spk, wav_name)] = (x, sr)
                labs[os.path.join(raw, spk, wav_name[:11] + ".lab")] = " ".join(text.split(" ")[1::2])
                k += 1
    return config("AISHELL3", corpus, raw, cleaners=[]), wavs, labs


def listing(root):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs)
