"""Corpus feature extraction around the HIP STFT (reference preprocessor/preprocessor.py:15-310, preprocess.py).

`Preprocessor(config).build_from_path()` reads `{raw_path}/{speaker}/{basename}.wav|.lab` and the MFA alignments under
`{preprocessed_path}/TextGrid/{speaker}/{basename}.TextGrid`, and writes what `dataset.py` reads:
`{mel,pitch,energy,duration}/{speaker}-{kind}-{basename}.npy`, `stats.json`, `speakers.json`, `train.txt`, `val.txt`.

The reference runs one utterance at a time through a CPU conv1d STFT (`preprocessor.py:194`).  Here the corpus is
processed in two stages so that the GPU sees few, large launches:

  host stage    per utterance: TextGrid -> phones / frame durations / trim window (`get_alignment`), wav read + trim,
                F0 (pyworld DIO + StoneMask when importable, or a caller-supplied `pitch_fn`); thread pool.
                With `pitch="gpu"` F0 moves to the device stage instead: `pitch.dio_stonemask` on each ragged batch of the
                unclipped trimmed audio (csrc/fs2_f0.hip).
                With `resample="gpu"` a file whose rate differs from the config's is no longer resampled here: the wav stays at
                its own rate, the trim window is computed in OUTPUT samples exactly as above, and only the input span that
                window depends on goes to the device stage.
  device stage  utterances are packed into ragged batches of up to `batch_seconds` of padded audio (`ragged.greedy_batches`);
                per batch: `ragged.Staging` -> one H2D copy -> reflect pad per row -> framed-DFT GEMM -> fused
                |.| / mel / log / energy epilogue -> one D2H copy, `audio.TacotronSTFT.mel_spectrogram_ragged`.
                With `resample="gpu"` batches hold one source rate and start with `resample.resample_poly` of each row's trim
                window (csrc/fs2_resample.hip): its unclipped output feeds `pitch.dio_stonemask`, its clamped output the STFT,
                without a round trip through the host.

Everything after the device stage (trim to sum(duration), phoneme-level averaging, outlier removal for the statistics,
normalisation, file formats, metadata lines, the train/val split) follows the reference line by line, including
its quirk that a wav WITHOUT a TextGrid re-feeds the previous utterance's pitch/energy values into the running
statistics (`preprocessor.py:70-89`: `pitch`, `energy`, `n` keep their last values).

Third-party pieces of the reference that are absent from this image and what stands in for them:
  tgt==1.4.4 `io.read_textgrid`  -> `read_textgrid` below (long and short Praat text formats; empty-text intervals
                                    are dropped, as tgt does by default with include_empty_intervals=False)
  librosa==0.7.2 `load`          -> `load_wav`: scipy.io.wavfile, mono, float32 in [-1, 1); polyphase resampling to
                                    22050 Hz only if the file's rate differs (librosa.load's default sr; the files
                                    `prepare_align.py` writes are already at that rate)
  pyworld==0.2.10 dio/stonemask  -> imported when present; otherwise `pitch_fn` or `pitch="gpu"` (DIO + StoneMask as HIP
                                    kernels, fastspeech2_amd/pitch.py) must be given (no silent substitute)
  sklearn StandardScaler         -> `RunningMoments` (the same incremental mean/variance update, Chan et al.)
"""
import json
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import audio as Audio, ragged

SIL_PHONES = ("sil", "sp", "spn")


# ------------------------------------------------------------------------------------------------ TextGrid
_TOKEN = re.compile(r'"((?:[^"]|"")*)"|(-?\d+(?:\.\d+)?(?:[eE][-+]?\d+)?)|(<exists>|<absent>)')


def read_textgrid(path, include_empty_intervals=False):
    """Praat TextGrid (long "key = value" or short value-only text format) -> {tier name: [(start, end, text), ...]}.
    Point tiers yield (time, time, mark).  Replaces tgt.io.read_textgrid for `preprocessor.py:162-165`."""
    raw = open(path, "rb").read()
    for enc in ("utf-8-sig", "utf-16"):
        try:
            src = raw.decode(enc)
            break
        except UnicodeError:
            continue
    else:
        raise ValueError(f"{path}: not a UTF-8/UTF-16 TextGrid")
    lines = []
    for line in src.splitlines():
        s = line.strip()
        if s.startswith("!"):                                   # Praat comment line
            continue
        # long format: drop everything up to '=' (key names, "[n]" indices) unless the '=' sits inside a quoted string
        if "=" in s:
            q = s.find('"')
            e = s.find("=")
            if q < 0 or e < q:
                s = s[e + 1:]
        elif re.match(r"^(item|intervals|points)\s*\[\d*\]\s*:?$", s) or s in ("item []:", "item []"):
            continue
        lines.append(s)
    toks = []
    for m in _TOKEN.finditer("\n".join(lines)):
        if m.group(1) is not None:
            toks.append(m.group(1).replace('""', '"'))
        elif m.group(2) is not None:
            toks.append(float(m.group(2)))
        else:
            toks.append(m.group(3) == "<exists>")
    if len(toks) < 6 or toks[0] != "ooTextFile" or toks[1] != "TextGrid":
        raise ValueError(f"{path}: not a Praat TextGrid text file")
    pos = 4                                                     # file type, object class, xmin, xmax
    if toks[pos] is not True:
        return {}
    n_tiers = int(toks[pos + 1])
    pos += 2
    tiers = {}
    for _ in range(n_tiers):
        cls, name = toks[pos], toks[pos + 1]
        n = int(toks[pos + 4])
        pos += 5
        items = []
        if cls == "IntervalTier":
            for _ in range(n):
                s, e, text = float(toks[pos]), float(toks[pos + 1]), toks[pos + 2]
                pos += 3
                if include_empty_intervals or text.strip() != "":
                    items.append((s, e, text))
        elif cls == "TextTier":
            for _ in range(n):
                t, text = float(toks[pos]), toks[pos + 1]
                pos += 2
                items.append((t, t, text))
        else:
            raise ValueError(f"{path}: unknown tier class {cls!r}")
        tiers.setdefault(name, items)
    return tiers


# ------------------------------------------------------------------------------------------------ small host pieces
def load_wav(path, target_sr=22050, resample=True):
    """float32 mono waveform at `target_sr` (what `librosa.load(path)` returns for the reference, preprocessor.py:172).
    `resample=False` leaves the file at its own rate and returns (waveform, rate) for a caller that resamples on the GPU."""
    from scipy.io import wavfile

    sr, w = wavfile.read(path)
    if w.dtype.kind == "i":
        w = w.astype(np.float32) / float(1 << (8 * w.dtype.itemsize - 1))
    elif w.dtype.kind == "u":                                   # 8-bit PCM
        w = (w.astype(np.float32) - 128.0) / 128.0
    else:
        w = w.astype(np.float32)
    if w.ndim == 2:
        w = w.mean(axis=1)
    if not resample:
        return w, int(sr)
    if sr != target_sr:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(sr), int(target_sr))
        w = resample_poly(w, target_sr // g, sr // g).astype(np.float32)
    return w


class RunningMoments:
    """Incremental mean / population variance (sklearn StandardScaler.partial_fit's update, preprocessor.py:61-62,86-89)."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, 0.0, 0.0

    def partial_fit(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if x.size == 0:
            return self
        new_sum = x.sum()
        n_new, n_old = x.size, self.n
        n_tot = n_old + n_new
        new_m2 = x.var() * n_new
        if n_old == 0:
            m2 = new_m2
        else:
            last_sum = self.mean * n_old
            ratio = n_old / n_new
            m2 = self.m2 + new_m2 + ratio / n_tot * (last_sum / ratio - new_sum) ** 2
        self.mean = (self.mean * n_old + new_sum) / n_tot
        self.m2, self.n = m2, n_tot
        return self

    @property
    def scale(self):
        s = float(np.sqrt(self.m2 / max(self.n, 1)))
        return s if s != 0.0 else 1.0                           # sklearn's _handle_zeros_in_scale


def remove_outlier(values):
    """preprocessor.py:283-291: Tukey fence - keep what lies strictly inside (Q1 - 1.5 IQR, Q3 + 1.5 IQR)."""
    v = np.asarray(values)
    q1, q3 = np.percentile(v, [25, 75])
    fence = 1.5 * (q3 - q1)
    return v[(v > q1 - fence) & (v < q3 + fence)]


def phoneme_average(values, durations):
    """preprocessor.py:210-218,222-229: mean over each phoneme's frames (0 for zero-length phonemes); returns len(durations)
    values.  Slices past the end of `values` behave as numpy's do (mean of an empty slice is NaN), like the reference."""
    out = np.array(values, copy=True)
    pos = 0
    for i, d in enumerate(durations):
        out[i] = np.mean(out[pos:pos + d]) if d > 0 else 0
        pos += d
    return out[:len(durations)]


def _pyworld_pitch():
    try:
        import pyworld as pw
    except ImportError:
        return None

    def pitch_fn(wav, sampling_rate, hop_length):
        x = wav.astype(np.float64)
        f0, t = pw.dio(x, sampling_rate, frame_period=hop_length / sampling_rate * 1000)
        return pw.stonemask(x, f0, t, sampling_rate)
    return pitch_fn


def resolve_pitch(choice):
    """preprocess.py --pitch: "pyworld" -> None (the host pyworld path), "gpu" -> "gpu", "pyin" -> "pyin", "auto" -> pyworld when
    importable, else "gpu".  The result is Preprocessor's `pitch` keyword."""
    if choice not in ("auto", "pyworld", "gpu", "pyin"):
        raise ValueError(f"--pitch must be auto, pyworld, gpu or pyin, got {choice!r}")
    if choice == "auto":
        return None if _pyworld_pitch() is not None else "gpu"
    return None if choice == "pyworld" else choice


# ------------------------------------------------------------------------------------------------ the preprocessor
class Preprocessor:
    def __init__(self, config, device="cuda", pitch_fn=None, batch_seconds=1800.0, num_workers=8, seed=None, pitch=None,
                 resample=None):
        """`config` = preprocess.yaml (preprocessor.py:16-51).  `pitch_fn(wav float32, sampling_rate, hop_length) -> f0 per
        frame (0 = unvoiced)` replaces pyworld when that package is absent; `pitch="gpu"` computes F0 on the GPU per ragged
        batch instead (fastspeech2_amd.pitch), `pitch="pyin"` does the same with probabilistic YIN (fastspeech2_amd.pyin);
        `seed` fixes the train/val shuffle (the reference uses the unseeded global `random`); `resample="gpu"` converts files at another rate than the config's on the GPU, per ragged batch, instead of
        per file in `load_wav` (needs `pitch="gpu"` or "pyin": a host pitch backend would need the audio back on the host)."""
        if resample not in (None, "gpu"):
            raise ValueError(f"resample must be None or 'gpu', got {resample!r}")
        if resample == "gpu" and pitch not in ("gpu", "pyin"):
            raise ValueError("resample='gpu' needs pitch='gpu' or 'pyin': with a host pitch backend the resampled audio would have to "
                             "come back to the host")
        if pitch not in (None, "gpu", "pyin"):
            raise ValueError(f"pitch must be None, 'gpu' or 'pyin', got {pitch!r}")
        if pitch is not None and pitch_fn is not None:
            raise ValueError(f"pass either pitch_fn or pitch={pitch!r}, not both")
        if pitch is not None:
            ragged.require_device(torch.device(device),
                                  f"Preprocessor(pitch={pitch!r}): " + ("DIO + StoneMask" if pitch == "gpu" else "pYIN"))
        self.config = config
        self.in_dir = config["path"]["raw_path"]
        self.out_dir = config["path"]["preprocessed_path"]
        self.val_size = config["preprocessing"]["val_size"]
        self.sampling_rate = config["preprocessing"]["audio"]["sampling_rate"]
        self.hop_length = config["preprocessing"]["stft"]["hop_length"]
        assert config["preprocessing"]["pitch"]["feature"] in ["phoneme_level", "frame_level"]
        assert config["preprocessing"]["energy"]["feature"] in ["phoneme_level", "frame_level"]
        self.pitch_phoneme_averaging = config["preprocessing"]["pitch"]["feature"] == "phoneme_level"
        self.energy_phoneme_averaging = config["preprocessing"]["energy"]["feature"] == "phoneme_level"
        self.pitch_normalization = config["preprocessing"]["pitch"]["normalization"]
        self.energy_normalization = config["preprocessing"]["energy"]["normalization"]
        self.STFT = Audio.TacotronSTFT(
            config["preprocessing"]["stft"]["filter_length"], config["preprocessing"]["stft"]["hop_length"],
            config["preprocessing"]["stft"]["win_length"], config["preprocessing"]["mel"]["n_mel_channels"],
            config["preprocessing"]["audio"]["sampling_rate"], config["preprocessing"]["mel"]["mel_fmin"],
            config["preprocessing"]["mel"]["mel_fmax"])
        self.device = torch.device(device)
        self.pitch_fn = pitch_fn
        self.pitch = pitch
        self.resample = resample
        self.batch_samples = int(batch_seconds * self.sampling_rate)
        self.num_workers = num_workers
        self.host_chunk = max(64, 8 * num_workers)          # utterances handed to the host thread pool at a time
        self.seed = seed
        self._staging = ragged.Staging()

    # ---------------------------------------------------------------- host stage
    def get_alignment(self, intervals):
        """preprocessor.py:243-281 on [(start, end, phone), ...]: trim leading / trailing silences, durations in frames as the
        difference of the ROUNDED boundary positions (so they telescope), trim window in seconds."""
        phones, durations = [], []
        start_time = end_time = 0
        end_idx = 0
        for s, e, p in intervals:
            if phones == []:
                if p in SIL_PHONES:
                    continue
                start_time = s
            phones.append(p)
            if p not in SIL_PHONES:
                end_time = e
                end_idx = len(phones)
            durations.append(int(np.round(e * self.sampling_rate / self.hop_length)
                                 - np.round(s * self.sampling_rate / self.hop_length)))
        return phones[:end_idx], durations[:end_idx], start_time, end_time

    def _tg_path(self, speaker, basename):
        return os.path.join(self.out_dir, "TextGrid", speaker, "{}.TextGrid".format(basename))

    def _host_stage(self, speaker, basename):
        """preprocessor.py:154-191 up to (not including) the STFT.  Returns None where the reference returns None."""
        tiers = read_textgrid(self._tg_path(speaker, basename))
        if "phones" not in tiers:
            raise KeyError("{}: no tier named 'phones'".format(self._tg_path(speaker, basename)))
        phone, duration, start, end = self.get_alignment(tiers["phones"])
        if start >= end:
            return None
        window = {}
        if self.resample == "gpu":                                          # the same window, in samples of the resampled file
            from . import resample as R
            full, sr = load_wav(os.path.join(self.in_dir, speaker, "{}.wav".format(basename)), resample=False)
            up, down = R.ratio(sr, self.sampling_rate)
            n_out = R.out_length(len(full), up, down)
            a, e = min(int(self.sampling_rate * start), n_out), min(int(self.sampling_rate * end), n_out)
            lo, hi = R.input_span(a, e - a, len(full), up, down)
            wav = full[lo:hi].astype(np.float32)
            window = {"sr": sr, "in_begin": lo, "out_begin": a, "out_len": max(e - a, 0)}
        else:
            wav = load_wav(os.path.join(self.in_dir, speaker, "{}.wav".format(basename)))
            wav = wav[int(self.sampling_rate * start):int(self.sampling_rate * end)].astype(np.float32)
        with open(os.path.join(self.in_dir, speaker, "{}.lab".format(basename)), "r") as f:
            raw_text = f.readline().strip("\n")
        pitch = None                                                        # pitch="gpu" / "pyin": set by the device stage
        if self.pitch is None:
            pitch = np.asarray(self.pitch_fn(wav, self.sampling_rate, self.hop_length), dtype=np.float64)[:sum(duration)]
            if np.sum(pitch != 0) <= 1:
                return None
        return {"speaker": speaker, "basename": basename, "text": "{" + " ".join(phone) + "}", "raw_text": raw_text,
                "duration": duration, "wav": wav, "pitch": pitch, **window}

    # ---------------------------------------------------------------- device stage
    def _stage(self, wavs, clip=False):
        """[float32 1-D] -> ((B, N) float32 on the device, lengths); one H2D copy (ragged.Staging)."""
        ragged.require_device(self.device, "fastspeech2_amd.preprocess")
        self._staging.pack(wavs, clip)
        return self._staging.to(self.device), [len(w) for w in wavs]

    def _features(self, mel, energy, frames):
        mel, energy = mel.cpu().numpy(), energy.cpu().numpy()               # one D2H each; the copy orders after the kernels
        return [(mel[b, :, :f].astype(np.float32), energy[b, :f].astype(np.float32)) for b, f in enumerate(frames.tolist())]

    def _extract_mels(self, wavs):
        """[float32 1-D] -> [(mel (n_mel, frames), energy (frames,))] float32 numpy; one ragged launch set on the GPU
        (audio/tools.py:8-15 `get_mel_from_wav` per utterance in the reference: clip to [-1, 1], STFT, squeeze)."""
        return self._features(*self.STFT.mel_spectrogram_ragged(*self._stage(wavs, clip=True)))

    def _f0_batch(self, y, lens):
        """The chosen device estimator on one ragged batch -> (f0 (B, Fmax) float64 numpy, frames (B,) numpy); one D2H copy."""
        frame_period = self.hop_length / self.sampling_rate * 1000
        if self.pitch == "pyin":
            from . import pyin as Pyin
            f0, _, _, frames = Pyin.pyin_numpy(y, lens, self.sampling_rate, frame_period)
        else:
            from . import pitch as Pitch
            f0, _, frames = Pitch.dio_stonemask(y, lens, self.sampling_rate, frame_period)
        return f0, frames

    def _extract_pitch(self, wavs):
        """pitch="gpu": [float32 1-D] -> [f0 per DIO frame, float64], DIO + StoneMask on the GPU over the UNCLIPPED audio (the
        reference's pitch_fn sees the wav before get_mel_from_wav clips it); one H2D and one D2H copy.  pitch="pyin": the same
        with pYIN, on the same frame grid."""
        f0, frames = self._f0_batch(*self._stage(wavs))
        return [f0[b, :f] for b, f in enumerate(frames.tolist())]

    def _extract_resampled(self, its):
        """resample="gpu": host-stage items of ONE source rate -> ([f0 per DIO frame], [(mel, energy)]).  One H2D copy of the input
        spans, `resample_poly` of each row's trim window, then F0 on its unclipped and the STFT on its clamped output."""
        from . import resample as R
        x, lens = self._stage([it["wav"] for it in its])
        y, yc, out_lens = R.resample_poly(x, lens, its[0]["sr"], self.sampling_rate,
                                          out_begin=[it["out_begin"] for it in its], out_len=[it["out_len"] for it in its],
                                          clip=True, in_begin=[it["in_begin"] for it in its])
        f0, f0_frames = self._f0_batch(y, out_lens)
        return ([f0[b, :f] for b, f in enumerate(f0_frames.tolist())],
                self._features(*self.STFT.mel_spectrogram_ragged(yc, out_lens)))

    # ---------------------------------------------------------------- per utterance, after the STFT
    def _finish_utterance(self, it, mel_spectrogram, energy):
        """preprocessor.py:194-241."""
        duration, pitch = it["duration"], it["pitch"]
        speaker, basename = it["speaker"], it["basename"]
        mel_spectrogram = mel_spectrogram[:, :sum(duration)]
        energy = energy[:sum(duration)]
        if self.pitch_phoneme_averaging:
            from scipy.interpolate import interp1d
            nonzero_ids = np.where(pitch != 0)[0]
            interp_fn = interp1d(nonzero_ids, pitch[nonzero_ids],
                                 fill_value=(pitch[nonzero_ids[0]], pitch[nonzero_ids[-1]]), bounds_error=False)
            pitch = phoneme_average(interp_fn(np.arange(0, len(pitch))), duration)
        if self.energy_phoneme_averaging:
            energy = phoneme_average(energy, duration)
        np.save(os.path.join(self.out_dir, "duration", "{}-duration-{}.npy".format(speaker, basename)), duration)
        np.save(os.path.join(self.out_dir, "pitch", "{}-pitch-{}.npy".format(speaker, basename)), pitch)
        np.save(os.path.join(self.out_dir, "energy", "{}-energy-{}.npy".format(speaker, basename)), energy)
        np.save(os.path.join(self.out_dir, "mel", "{}-mel-{}.npy".format(speaker, basename)), mel_spectrogram.T)
        return ("|".join([basename, speaker, it["text"], it["raw_text"]]), remove_outlier(pitch), remove_outlier(energy),
                mel_spectrogram.shape[1])

    def normalize(self, in_dir, mean, std):
        """preprocessor.py:293-305: standardise every .npy of `in_dir` in place; returns the (min, max) over the whole corpus
        (float64 extremes when the directory is empty, as the reference's running min / max start there)."""
        lo, hi = np.finfo(np.float64).max, np.finfo(np.float64).min
        for name in os.listdir(in_dir):
            path = os.path.join(in_dir, name)
            z = (np.load(path) - mean) / std
            np.save(path, z)
            if z.size:
                lo, hi = min(lo, z.min()), max(hi, z.max())
        return lo, hi

    # ---------------------------------------------------------------- the corpus pass
    def build_from_path(self):
        if self.pitch_fn is None and self.pitch is None:
            self.pitch_fn = _pyworld_pitch()
        if self.pitch_fn is None and self.pitch is None:
            raise RuntimeError("pyworld is not installed: pass pitch_fn=(wav, sampling_rate, hop_length) -> f0 per frame, "
                               "or pitch=\"gpu\" for DIO + StoneMask on the GPU")
        for d in ("mel", "pitch", "energy", "duration"):
            os.makedirs(os.path.join(self.out_dir, d), exist_ok=True)
        print("Processing Data ...")

        # corpus walk in the reference's order (preprocessor.py:66-73); entries without a TextGrid are kept as markers
        speakers, entries = {}, []
        for i, speaker in enumerate(os.listdir(self.in_dir)):
            speakers[speaker] = i
            for wav_name in os.listdir(os.path.join(self.in_dir, speaker)):
                if ".wav" not in wav_name:
                    continue
                basename = wav_name.split(".")[0]
                entries.append((speaker, basename, os.path.exists(self._tg_path(speaker, basename))))

        # the corpus streams through in windows of a few device batches of audio, so host memory holds one window of waveforms
        # (not the corpus: LibriTTS is ~185 GB of float32 samples); per-utterance results kept for the statistics are tiny
        todo = [k for k, e in enumerate(entries) if e[2]]
        results = {}                                                        # entry index -> _finish_utterance tuple, or None
        window, window_samples = [], 0

        def flush():
            items = [it for _, it in window]
            # resample="gpu": a batch holds one source rate
            for _, batch in ragged.keyed_batches([it.get("sr") for it in items], [(len(it["wav"]),) for it in items],
                                                 lambda sr: self.batch_samples, ragged.padded_samples):
                if self.resample == "gpu":
                    pitches, mels = self._extract_resampled([items[i] for i in batch])
                else:
                    wavs = [items[i]["wav"] for i in batch]
                    pitches = self._extract_pitch(wavs) if self.pitch is not None else None
                    mels = self._extract_mels(wavs)
                for j, (i, (mel, energy)) in enumerate(zip(batch, mels)):
                    items[i]["wav"] = None                                  # release the audio once its features exist
                    if pitches is not None:                                 # _host_stage's trim and voiced-frame rule
                        items[i]["pitch"] = pitches[j][:sum(items[i]["duration"])]
                        if np.sum(items[i]["pitch"] != 0) <= 1:
                            results[window[i][0]] = None
                            continue
                    results[window[i][0]] = self._finish_utterance(items[i], mel, energy)
            window.clear()

        with ThreadPoolExecutor(max_workers=max(1, self.num_workers)) as pool:
            chunk = self.host_chunk
            for c0 in range(0, len(todo), chunk):
                ks = todo[c0:c0 + chunk]
                for k, it in zip(ks, pool.map(lambda k: self._host_stage(entries[k][0], entries[k][1]), ks)):
                    if it is None:
                        results[k] = None
                        continue
                    window.append((k, it))
                    window_samples += len(it["wav"])
                if window_samples >= 4 * self.batch_samples:
                    flush()
                    window_samples = 0
            flush()

        # running statistics in corpus order, with the reference's stale-value behaviour for wavs that have no TextGrid
        out, n_frames = [], 0
        pitch_scaler, energy_scaler = RunningMoments(), RunningMoments()
        last = None
        for k, (speaker, basename, has_tg) in enumerate(entries):
            if has_tg:
                if results[k] is None:
                    continue                                                # preprocessor.py:80-81
                last = results[k]
                out.append(last[0])
            if last is None:
                raise NameError("first wav of the corpus has no TextGrid (the reference fails here too: "
                                "preprocessor.py:86 reads `pitch` before assignment)")
            _, pitch, energy, n = last
            if len(pitch) > 0:
                pitch_scaler.partial_fit(pitch)
            if len(energy) > 0:
                energy_scaler.partial_fit(energy)
            n_frames += n

        print("Computing statistic quantities ...")
        pitch_mean, pitch_std = (pitch_scaler.mean, pitch_scaler.scale) if self.pitch_normalization else (0, 1)
        energy_mean, energy_std = (energy_scaler.mean, energy_scaler.scale) if self.energy_normalization else (0, 1)
        pitch_min, pitch_max = self.normalize(os.path.join(self.out_dir, "pitch"), pitch_mean, pitch_std)
        energy_min, energy_max = self.normalize(os.path.join(self.out_dir, "energy"), energy_mean, energy_std)

        with open(os.path.join(self.out_dir, "speakers.json"), "w") as f:
            f.write(json.dumps(speakers))
        with open(os.path.join(self.out_dir, "stats.json"), "w") as f:
            f.write(json.dumps({"pitch": [float(pitch_min), float(pitch_max), float(pitch_mean), float(pitch_std)],
                                "energy": [float(energy_min), float(energy_max), float(energy_mean), float(energy_std)]}))
        print("Total time: {} hours".format(n_frames * self.hop_length / self.sampling_rate / 3600))

        (random.Random(self.seed) if self.seed is not None else random).shuffle(out)
        out = [r for r in out if r is not None]
        with open(os.path.join(self.out_dir, "train.txt"), "w", encoding="utf-8") as f:
            for m in out[self.val_size:]:
                f.write(m + "\n")
        with open(os.path.join(self.out_dir, "val.txt"), "w", encoding="utf-8") as f:
            for m in out[:self.val_size]:
                f.write(m + "\n")
        return out
