#!/usr/bin/env python
"""score.py — objective scores of synthesized against recorded speech on the GPU (fastspeech2_amd/metrics.py):

    python score.py -p preprocess.yaml -t train.yaml --source val.txt [--syn_dir DIR] [--ref_dir DIR] [--no_trim] [--no_f0]
                    [--cepstra {mel,world}] [--alpha A] [--n_mcep K] [--prosody] [--f0 {dio,pyin}] [--aligned] [--max_len_diff N]
                    [--smoothing] [--wavelet] [--hnr] [--out scores.jsonl]

For every `basename|speaker|...` line of `--source` the recorded `{raw_path}/{speaker}/{basename}.wav` (or `{ref_dir}/{basename}.wav`)
is compared with `{result_path}/{basename}.wav` (or `{syn_dir}/...`), where `synthesize.py --mode batch` writes: mel-cepstral
distortion along a dynamic-time-warping path, F0 RMSE in cents and voiced / unvoiced error on that path.  The recorded file is cut
to its TextGrid's speech window, the window the training mel came from, unless `--no_trim` is given or there is no TextGrid; every
output row says which was used.  One JSON object per utterance goes to `--out`, one summary line to stdout.  With `--cepstra mel`
(the default, 13 coefficients) the cepstra are a DCT of this project's own log-mel: the dB values compare runs of this tool, not
published MCD figures.  With `--cepstra world` (24 coefficients) they are mel-cepstra of the CheapTrick spectral envelope, the
published definition (fastspeech2_amd/envelope.py); the all-pass constant comes from the sampling rate unless `--alpha` gives it, and
rows and summary also carry `cepstra`, `alpha` and `fft_size`.  Agreement with the pyworld / pysptk binaries is unmeasured.
With `--prosody` (not with `--no_f0`) every row and the summary also carry the numbers FastSpeech 2 evaluates its variance adaptor by:
gross pitch error, F0 frame error and log-F0 correlation on the path, the DTW distance between the voiced pitch contours in Hz, the
mean absolute error of the frame energy, and the standard deviation, skewness and excess kurtosis of the voiced F0 of both sides.
The paper does not say how it treats unvoiced frames or in which unit its DTW distance is: these compare runs of this tool.
With `--f0 pyin` both sides of every F0 and prosody number come from probabilistic YIN (fastspeech2_amd/pyin.py) instead of DIO +
StoneMask, an independent estimator to cross-check the pitch scores with; rows and summary then carry `f0_estimator`.
With `--aligned` the synthesized wavs are taken to share the recording's time axis, as copysynth.py's do (a recorded mel through the
vocoder): a pair whose lengths differ by more than `--max_len_diff` samples (default 2 hop_length) is skipped as not time-aligned,
every other pair is cut to its shorter side and also gets STOI and ESTOI (fastspeech2_amd/stoi.py: the published algorithms on this
project's own resampler; agreement with pystoi or the authors' MATLAB code is unmeasured), and the summary their corpus means.
With `--smoothing` every row and the summary also carry the two published measures of over-smoothed spectra, taken of both sides'
cepstra (fastspeech2_amd/modspec.py): the global variance per coefficient and its ratio in dB, and the modulation spectrum in bands
from 0 to the frame-rate Nyquist with the distance between the two sides.  A ratio or a band difference below 0 says the synthesized
trajectories vary too little; the numbers compare runs of this tool, and a value near 0 is not a claim of naturalness.
With `--wavelet` (not with `--no_f0`; it goes with either `--f0` and either `--cepstra`, and does not need `--prosody`) every row and
the summary also say at which time scale the pitch contour departs from the recording (fastspeech2_amd/cwt.py): both sides' F0 is
interpolated over the unvoiced frames, taken as ln F0 and normalised per utterance, transformed by a Mexican-hat wavelet at ten
scales from 20 ms to 10.24 s, and the two transforms are correlated along the DTW path, per scale and per level of two adjacent
scales, with the power per scale of each side and the mean and deviation of ln F0.  The constants are FastSpeech 2's pitch
spectrogram's as remembered, not checked against the papers; the numbers compare runs of this tool.
With `--hnr` (not with `--no_f0`; it goes with either `--f0` and either `--cepstra`) every row and the summary also say how clean
the voiced speech of both sides is (fastspeech2_amd/hnr.py): the harmonics-to-noise ratio of Boersma (1993) in dB per voiced frame,
from the window-corrected autocorrelation at the lags around the scored F0, its mean and deviation per side, and its difference
(synthesized minus reference), RMSE and correlation along the DTW path.  A periodic signal in white noise at S dB SNR scores S dB.
Agreement with Praat is unmeasured, and a higher value is not claimed to be better: the numbers compare the two sides and runs of
this tool."""
import argparse
import json
import sys

import yaml

from fastspeech2_amd import metrics


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-p", "--preprocess_config", type=str, required=True, help="path to preprocess.yaml")
    parser.add_argument("-t", "--train_config", type=str, required=True, help="path to train.yaml (path.result_path)")
    parser.add_argument("--source", type=str, required=True, help="metadata file of `basename|speaker|...` lines (val.txt)")
    parser.add_argument("--syn_dir", type=str, default=None, help="folder of the synthesized wavs (default: train.yaml's result_path)")
    parser.add_argument("--ref_dir", type=str, default=None, help="folder of the recorded wavs (default: raw_path/speaker)")
    parser.add_argument("--no_trim", action="store_true", help="use the whole recorded file, not its TextGrid's speech window")
    parser.add_argument("--no_f0", action="store_true", help="mel-cepstral distortion only")
    parser.add_argument("--cepstra", choices=("mel", "world"), default="mel",
                        help="mel: DCT of the log-mel (tool-internal); world: mel-cepstra of the CheapTrick spectral envelope")
    parser.add_argument("--alpha", type=float, default=None, help="all-pass constant of --cepstra world (default: by sampling rate)")
    parser.add_argument("--n_mcep", type=int, default=None, help="cepstral coefficients 1..n_mcep (at most 40; default 13 mel, 24 world)")
    parser.add_argument("--prosody", action="store_true",
                        help="also GPE, FFE, log-F0 correlation, pitch-contour DTW, energy MAE and the pitch moments (needs F0)")
    parser.add_argument("--f0", choices=("dio", "pyin"), default="dio",
                        help="estimator of both sides of every F0 and prosody score: DIO + StoneMask or probabilistic YIN; with --cepstra "
                             "world CheapTrick keeps its own DIO + StoneMask F0 whatever this says")
    parser.add_argument("--aligned", action="store_true",
                        help="the wavs are sample-aligned with the recordings (copysynth.py): also STOI and ESTOI per pair")
    parser.add_argument("--max_len_diff", type=int, default=None,
                        help="--aligned: skip a pair whose lengths differ by more samples than this (default 2 hop_length)")
    parser.add_argument("--smoothing", action="store_true",
                        help="also the global variance and the modulation spectrum of both sides' cepstra: how over-smoothed the "
                             "synthesized spectra are")
    parser.add_argument("--wavelet", action="store_true",
                        help="also the wavelet prosody scores: correlation, RMSE and power of the continuous ln F0 at ten time scales "
                             "(needs F0)")
    parser.add_argument("--hnr", action="store_true",
                        help="also the harmonics-to-noise ratio of both sides' voiced frames, per side and along the path (needs F0)")
    parser.add_argument("--out", type=str, default="scores.jsonl")
    parser.add_argument("--device", type=str, default="cuda")
    return parser.parse_args(argv)


def main(argv=None, score_fn=None, aligned_fn=None):
    args = parse_args(argv)
    config = yaml.load(open(args.preprocess_config, "r"), Loader=yaml.FullLoader)
    train = yaml.load(open(args.train_config, "r"), Loader=yaml.FullLoader)
    try:
        rows, skipped, summary = metrics.run(config, train["path"]["result_path"], args.source, out_path=args.out, syn_dir=args.syn_dir,
                                             ref_dir=args.ref_dir, trim=not args.no_trim, f0=not args.no_f0, n_mcep=args.n_mcep,
                                             score_fn=score_fn, device=args.device, cepstra=args.cepstra, alpha=args.alpha,
                                             prosody=args.prosody, f0_estimator=args.f0, aligned=args.aligned,
                                             max_len_diff=args.max_len_diff, aligned_fn=aligned_fn, smoothing=args.smoothing,
                                             wavelet=args.wavelet, hnr=args.hnr)
    except ValueError as e:
        sys.exit(str(e))
    for name, reason in skipped:
        print("skipped {}: {}".format(name, reason))
    print(json.dumps(summary))
    return rows, skipped, summary


if __name__ == "__main__":
    main()
