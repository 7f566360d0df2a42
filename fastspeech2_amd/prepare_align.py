"""Corpus -> `raw_path` for MFA and `Preprocessor` (reference prepare_align.py:1-21, preprocessor/{ljspeech,libritts,aishell3}.py):
`{raw_path}/{speaker}/{basename}.wav` at the configured rate, peak-normalised int16, beside `{basename}.lab` with the cleaned text.

`prepare_align(config)` dispatches on the corpus name in `config["dataset"]` and reads `path.corpus_path`, `path.raw_path`,
`preprocessing.audio.{sampling_rate, max_wav_value}` and `preprocessing.text.text_cleaners`.  The walkers restate the reference's
directory conventions:

  LJSpeech   `metadata.csv`, one `name|text|normalised text` line per utterance; audio `wavs/{name}.wav`; column 3 is cleaned and
             written; the single speaker is called `LJSpeech`.  A line whose wav is missing is skipped.
  LibriTTS   `{speaker}/{chapter}/{name}.wav` beside `{name}.normalized.txt`, whose first line is cleaned and written.
  AISHELL-3  `{train,test}/content.txt`, one `{wav name}<TAB>{hanzi pinyin hanzi pinyin ...}` line per utterance; the speaker is the
             first 7 characters of the wav name, the audio `{split}/wav/{speaker}/{wav name}`, the text every second token (the
             pinyin) joined by blanks, uncleaned; the .lab is named after the first 11 characters.  Missing wavs are skipped.

Text goes through `text._clean` (its `english_cleaners` warning says what is not built).

Audio.  The reference resamples one file at a time on the host (`librosa.load(path, sampling_rate)`) and then writes
`(wav / max|wav| * max_wav_value).astype(int16)`.  Here a host thread pool reads files as mono float32 at their own rate
(`preprocess.load_wav(resample=False)`); utterances are grouped by source rate and packed into ragged batches of up to
`batch_seconds` of padded audio (`ragged.keyed_batches`); per batch: `ragged.Staging` -> one H2D copy -> `resample.resample_poly` -> `peak_abs` -> `peaknorm_pcm` -> one
D2H copy of the int16 rows -> `scipy.io.wavfile.write`.  A file already at the target rate skips the resampler and is still
normalised, as the reference does to LJSpeech.  The filter, the cast (a positive peak sample times 32768 wraps to -32768, as in the
reference) and the one deviation (an all-zero file yields zeros, with a warning, where the reference divides by zero) are specified
in fastspeech2_amd/resample.py.

Loudness.  `normalize="loudness"` replaces the last two steps of the device stage by `peak_abs` -> `loudness.block_energy` ->
`integrated` -> `gain` -> `gain_pcm`: every utterance goes to `target_lufs` (ITU-R BS.1770-4 integrated loudness), the gain bounded by
the `ceiling_db` sample-peak ceiling, with a rounding, saturating cast (fastspeech2_amd/loudness.py).  The default stays `"peak"`, with
which nothing above changes.

`audio_fn(wavs, sr_in, sr_out, max_wav_value) -> [int16 arrays]` replaces the device stage (the seam `Preprocessor` has in
`pitch_fn`), so walkers, text and file layout can be exercised without a GPU.
"""
import json
import math
import os
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ragged
from .preprocess import load_wav
from .text import _clean


# ------------------------------------------------------------------------------------------------ corpus walkers
# each yields (wav_path, out_wav, out_lab, text): source file, the two files to write under raw_path, the .lab contents
def walk_ljspeech(in_dir, out_dir, cleaners):
    with open(os.path.join(in_dir, "metadata.csv"), encoding="utf-8") as f:
        for line in f:
            parts = line.strip().split("|")
            name = parts[0]
            yield (os.path.join(in_dir, "wavs", name + ".wav"), os.path.join(out_dir, "LJSpeech", name + ".wav"),
                   os.path.join(out_dir, "LJSpeech", name + ".lab"), _clean(parts[2], cleaners))


def walk_libritts(in_dir, out_dir, cleaners):
    for speaker in os.listdir(in_dir):
        for chapter in os.listdir(os.path.join(in_dir, speaker)):
            folder = os.path.join(in_dir, speaker, chapter)
            for file_name in os.listdir(folder):
                if file_name[-4:] != ".wav":
                    continue
                name = file_name[:-4]
                with open(os.path.join(folder, name + ".normalized.txt")) as f:
                    text = f.readline().strip("\n")
                yield (os.path.join(folder, file_name), os.path.join(out_dir, speaker, name + ".wav"),
                       os.path.join(out_dir, speaker, name + ".lab"), _clean(text, cleaners))


def walk_aishell3(in_dir, out_dir, cleaners=None):
    for split in ("train", "test"):
        with open(os.path.join(in_dir, split, "content.txt"), encoding="utf-8") as f:
            for line in f:
                wav_name, text = line.strip("\n").split("\t")
                speaker = wav_name[:7]
                yield (os.path.join(in_dir, split, "wav", speaker, wav_name), os.path.join(out_dir, speaker, wav_name),
                       os.path.join(out_dir, speaker, wav_name[:11] + ".lab"), " ".join(text.split(" ")[1::2]))


WALKERS = (("LJSpeech", walk_ljspeech), ("AISHELL3", walk_aishell3), ("LibriTTS", walk_libritts))


def _walker(config):
    for key, fn in WALKERS:                                                 # prepare_align.py:9-14, in its order
        if key in config["dataset"]:
            return fn
    raise ValueError(f"prepare_align knows LJSpeech, AISHELL3 and LibriTTS, not dataset {config['dataset']!r}")


# ------------------------------------------------------------------------------------------------ device stage
class _DeviceAudio:
    """audio_fn on the GPU: [float32 1-D] at sr_in -> [int16 1-D] at sr_out, peak-normalised or (normalize="loudness") brought to
    `target_lufs` under the `ceiling_db` sample-peak ceiling; one H2D and one D2H copy of audio per call.  After a loudness call
    `measurements` holds one dict per utterance of that call (the keys of `--report`, without `wav`)."""

    def __init__(self, device, normalize="peak", target_lufs=-23.0, ceiling_db=-1.0):
        self.device = ragged.require_device(torch.device(device), "fastspeech2_amd.prepare_align (without an audio_fn)")
        self._staging = ragged.Staging()
        self.normalize, self.target_lufs, self.ceiling_db = normalize, target_lufs, ceiling_db
        self.measurements = None

    def __call__(self, wavs, sr_in, sr_out, max_wav_value):
        from . import resample as R
        self._staging.pack(wavs)
        y, out_lens = R.resample_poly(self._staging.to(self.device), [len(w) for w in wavs], sr_in, sr_out)
        if self.normalize == "loudness":
            return self._loudness(y, out_lens, sr_out)
        pcm = R.peaknorm_pcm(y, out_lens, R.peak_abs(y, out_lens), max_wav_value).cpu().numpy()   # orders after the kernels
        return [pcm[b, :n].copy() for b, n in enumerate(out_lens.tolist())]

    def _loudness(self, y, out_lens, sr):
        """peak_abs -> block_energy -> integrated -> gain -> gain_pcm; the int16 rows and the per-utterance numbers (fp64: loudness,
        gain, flags, saturated count) leave the device in one buffer."""
        from . import loudness as L, resample as R
        B, N = y.shape
        peak = R.peak_abs(y, out_lens)
        loud = L.integrated(*L.block_energy(y, out_lens, sr))
        g, flags = L.gain(loud, peak, self.target_lufs, self.ceiling_db)
        buf = torch.empty(B * 4 * 8 + B * N * 2, dtype=torch.uint8, device=y.device)
        stats, pcm = buf[:B * 32].view(torch.float64).view(B, 4), buf[B * 32:].view(torch.int16).view(B, N)
        _, sat = L.gain_pcm(y, out_lens, g, out=pcm)
        stats.copy_(torch.stack([loud[:, 0], g, flags.double(), sat.double()], dim=1))
        host = buf.cpu()                                                     # orders after the kernels
        stats, pcm = host[:B * 32].view(torch.float64).view(B, 4).tolist(), host[B * 32:].view(torch.int16).view(B, N).numpy()
        out = [pcm[b, :n].copy() for b, n in enumerate(out_lens.tolist())]
        self.measurements = []
        for (lufs, gain, flag, clipped), row in zip(stats, out):
            gain_db = 20.0 * math.log10(gain) if gain > 0 else None
            fallback = bool(int(flag) & 2)
            peak_out = int(np.abs(row.astype(np.int32)).max()) if len(row) else 0
            self.measurements.append({
                "lufs_in": lufs if math.isfinite(lufs) else None,
                "lufs_out": lufs + gain_db if not fallback and gain_db is not None else None,
                "gain_db": gain_db, "limited": bool(int(flag) & 1), "fallback": fallback, "clipped": int(clipped),
                "sample_peak_dbfs_out": 20.0 * math.log10(peak_out / 32768.0) if peak_out else None})
        return out


# ------------------------------------------------------------------------------------------------ the corpus pass
NORMALIZE = ("peak", "loudness")
REPORT_KEYS = ("wav", "lufs_in", "lufs_out", "gain_db", "limited", "fallback", "clipped", "sample_peak_dbfs_out")


def _summary(rows, out_dir):
    """lines for stdout: mean and spread of the input loudness per speaker directory, then the limited and fallback counts"""
    by_spk = {}
    for r in rows:
        by_spk.setdefault(os.path.relpath(os.path.dirname(r["wav"]), out_dir), []).append(r["lufs_in"])
    lines = []
    for spk in sorted(by_spk):
        v = np.array([x for x in by_spk[spk] if x is not None], dtype=np.float64)
        if len(v):
            lines.append(f"{spk}: {len(by_spk[spk])} files, input loudness mean {v.mean():.2f} LUFS, std {v.std():.2f}, "
                         f"range {v.min():.2f} .. {v.max():.2f}")
        else:
            lines.append(f"{spk}: {len(by_spk[spk])} files, none long and loud enough to measure")
    lines.append(f"{sum(r['limited'] for r in rows)} of {len(rows)} files limited by the peak ceiling, "
                 f"{sum(r['fallback'] for r in rows)} without a loudness (shorter than 400 ms or silent: set to the ceiling)")
    return lines


def prepare_align(config, device="cuda", audio_fn=None, batch_seconds=1500.0, num_workers=8, normalize="peak", target_lufs=-23.0,
                  ceiling_db=-1.0, report=None):
    """Write `raw_path` from `corpus_path`; returns the number of utterances written.

    normalize="peak" (the default) is the reference's `wav / max|wav| * max_wav_value`.  normalize="loudness" brings every utterance
    to `target_lufs` (integrated loudness, ITU-R BS.1770-4: fastspeech2_amd/loudness.py) unless that would take its sample peak above
    `ceiling_db` dBFS, in which case the ceiling sets the gain; an utterance without a loudness (shorter than 400 ms, or silent) is
    set to the ceiling.  `report`: a file that receives one JSON object per written wav (REPORT_KEYS), one per line; a summary goes
    to stdout.  Loudness normalisation belongs to the device stage and cannot be combined with an `audio_fn`."""
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
    if normalize == "loudness":
        from .loudness import check_options
        check_options(target_lufs, ceiling_db)
        if audio_fn is not None:
            raise ValueError('normalize="loudness" runs in the device stage: it cannot be combined with an audio_fn')
    elif report is not None:
        raise ValueError('report is written by normalize="loudness" only')
    in_dir, out_dir = config["path"]["corpus_path"], config["path"]["raw_path"]
    sampling_rate = config["preprocessing"]["audio"]["sampling_rate"]
    max_wav_value = config["preprocessing"]["audio"]["max_wav_value"]
    cleaners = config["preprocessing"]["text"]["text_cleaners"]
    walk = _walker(config)
    if audio_fn is None:
        audio_fn = _DeviceAudio(device, normalize, target_lufs, ceiling_db)
    rows = []
    batch_samples = int(batch_seconds * sampling_rate)
    written = 0
    window, window_samples = [], 0                                          # (out_wav, source rate, float32 waveform)

    def flush():
        nonlocal written
        # a batch never mixes source rates (one filter per launch); its budget is `batch_seconds` at the source rate
        for sr, ks in ragged.keyed_batches([w[1] for w in window], [(len(w[2]),) for w in window],
                                           lambda sr: batch_samples * sr // sampling_rate, ragged.padded_samples):
            pcms = audio_fn([window[k][2] for k in ks], sr, sampling_rate, max_wav_value)
            if normalize == "loudness":
                rows.extend(dict(wav=window[k][0], **m) for k, m in zip(ks, audio_fn.measurements))
            for k, pcm in zip(ks, pcms):
                from scipy.io import wavfile
                pcm = np.asarray(pcm)
                assert pcm.dtype == np.int16 and pcm.ndim == 1, (pcm.dtype, pcm.shape)
                if not pcm.any():
                    warnings.warn(f"{window[k][0]}: silent file written as zeros (the reference divides by a zero peak here)")
                wavfile.write(window[k][0], sampling_rate, pcm)
                written += 1
        window.clear()

    def read(entry):
        wav_path, out_wav, out_lab, text = entry
        os.makedirs(os.path.dirname(out_wav), exist_ok=True)
        wav, sr = load_wav(wav_path, resample=False)
        with open(out_lab, "w") as f:
            f.write(text)
        return out_wav, sr, wav

    with ThreadPoolExecutor(max_workers=max(1, num_workers)) as pool:
        chunk, todo = max(64, 8 * num_workers), []

        def drain():
            nonlocal window_samples
            for item in pool.map(read, todo):
                window.append(item)
                window_samples += len(item[2])
            todo.clear()
            if window_samples >= 4 * batch_samples:                         # host memory holds a few device batches of audio
                flush()
                window_samples = 0

        for entry in walk(in_dir, out_dir, cleaners):
            if not os.path.exists(entry[0]):                                # the reference skips utterances without audio
                continue
            todo.append(entry)
            if len(todo) >= chunk:
                drain()
        drain()
        flush()
    if normalize == "loudness":
        if report is not None:
            with open(report, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")
        print("\n".join(_summary(rows, out_dir)))
    return written
