"""`python prepare_align.py config/LibriTTS/preprocess.yaml` — the reference's prepare_align.py:1-21: corpus_path -> raw_path
(wavs at the configured rate, peak-normalised int16, plus .lab transcripts) for MFA and preprocess.py, with the sample-rate
conversion and normalisation on the GPU in ragged batches (fastspeech2_amd/prepare_align.py)."""
import argparse

import yaml

from fastspeech2_amd.prepare_align import prepare_align

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("config", type=str, help="path to preprocess.yaml")
    parser.add_argument("--batch_seconds", type=float, default=1500.0, help="audio per ragged batch on the GPU")
    parser.add_argument("--num_workers", type=int, default=8, help="host threads reading wav files")
    parser.add_argument("--normalize", choices=("peak", "loudness"), default="peak",
                        help="peak: the reference's wav / max|wav|; loudness: integrated loudness (ITU-R BS.1770-4) to --target_lufs")
    parser.add_argument("--target_lufs", type=float, default=-23.0, help="loudness target in LUFS (--normalize loudness)")
    parser.add_argument("--ceiling_db", type=float, default=-1.0, help="sample-peak ceiling in dBFS that bounds the gain")
    parser.add_argument("--report", type=str, default=None, help="write one JSON object per wav (loudness in / out, gain, flags)")
    args = parser.parse_args()

    config = yaml.load(open(args.config, "r"), Loader=yaml.FullLoader)
    n = prepare_align(config, batch_seconds=args.batch_seconds, num_workers=args.num_workers, normalize=args.normalize,
                      target_lufs=args.target_lufs, ceiling_db=args.ceiling_db, report=args.report)
    print("{} utterances written to {}".format(n, config["path"]["raw_path"]))
