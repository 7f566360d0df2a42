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

`audio_fn(wavs, sr_in, sr_out, max_wav_value) -> [int16 arrays]` replaces the device stage (the seam `Preprocessor` has in
`pitch_fn`), so walkers, text and file layout can be exercised without a GPU.
"""
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
    """audio_fn on the GPU: [float32 1-D] at sr_in -> [int16 1-D] at sr_out, peak-normalised; one H2D and one D2H copy per call."""

    def __init__(self, device):
        self.device = ragged.require_device(torch.device(device), "fastspeech2_amd.prepare_align (without an audio_fn)")
        self._staging = ragged.Staging()

    def __call__(self, wavs, sr_in, sr_out, max_wav_value):
        from . import resample as R
        self._staging.pack(wavs)
        y, out_lens = R.resample_poly(self._staging.to(self.device), [len(w) for w in wavs], sr_in, sr_out)
        pcm = R.peaknorm_pcm(y, out_lens, R.peak_abs(y, out_lens), max_wav_value).cpu().numpy()   # orders after the kernels
        return [pcm[b, :n].copy() for b, n in enumerate(out_lens.tolist())]


# ------------------------------------------------------------------------------------------------ the corpus pass
def prepare_align(config, device="cuda", audio_fn=None, batch_seconds=1500.0, num_workers=8):
    """Write `raw_path` from `corpus_path`; returns the number of utterances written."""
    in_dir, out_dir = config["path"]["corpus_path"], config["path"]["raw_path"]
    sampling_rate = config["preprocessing"]["audio"]["sampling_rate"]
    max_wav_value = config["preprocessing"]["audio"]["max_wav_value"]
    cleaners = config["preprocessing"]["text"]["text_cleaners"]
    walk = _walker(config)
    if audio_fn is None:
        audio_fn = _DeviceAudio(device)
    batch_samples = int(batch_seconds * sampling_rate)
    written = 0
    window, window_samples = [], 0                                          # (out_wav, source rate, float32 waveform)

    def flush():
        nonlocal written
        # a batch never mixes source rates (one filter per launch); its budget is `batch_seconds` at the source rate
        for sr, ks in ragged.keyed_batches([w[1] for w in window], [(len(w[2]),) for w in window],
                                           lambda sr: batch_samples * sr // sampling_rate, ragged.padded_samples):
            pcms = audio_fn([window[k][2] for k in ks], sr, sampling_rate, max_wav_value)
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
    return written
