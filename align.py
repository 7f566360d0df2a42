"""`python align.py config/LJSpeech/preprocess.yaml` — forced alignment on the GPU in place of the Montreal Forced Aligner run the
reference's README asks for: trains a monophone HMM on `raw_path`'s wav + .lab pairs with `path.lexicon_path` and writes
`{preprocessed_path}/TextGrid/{speaker}/{basename}.TextGrid` for preprocess.py (fastspeech2_amd/align.py)."""
import argparse
import sys

import yaml

from fastspeech2_amd.align import build, scores_summary

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("config", type=str, help="path to preprocess.yaml")
    parser.add_argument("--states", type=int, default=2, help="HMM states per phone (1..3)")
    parser.add_argument("--iters", type=int, default=12, help="Baum-Welch passes after the flat start")
    parser.add_argument("--mixtures", type=int, default=1, help="Gaussian mixture components per state, grown by splitting (1..8)")
    parser.add_argument("--mix_iters", type=int, default=4, help="Baum-Welch passes after every split")
    parser.add_argument("--lda", type=int, default=0, help="output dimensions of an LDA over spliced frames before the Gaussian stages (0: none)")
    parser.add_argument("--splice", type=int, default=3, help="frames of context on either side that --lda splices (0..4)")
    parser.add_argument("--lda_iters", type=int, default=4, help="Baum-Welch passes after the LDA transform")
    parser.add_argument("--fmllr", type=int, default=0, choices=(0, 1),
                        help="1: per-speaker fMLLR transforms after the LDA stage (needs at most 64 feature dimensions: --lda k, k <= 64)")
    parser.add_argument("--fmllr_rounds", type=int, default=2, help="rounds of statistics, transform update and retraining")
    parser.add_argument("--fmllr_iters", type=int, default=2, help="Baum-Welch passes after every transform update")
    parser.add_argument("--fmllr_sweeps", type=int, default=20, help="row sweeps of every transform update")
    parser.add_argument("--fmllr_min_frames", type=float, default=500, help="a speaker with fewer frames keeps its transform")
    parser.add_argument("--triphones", type=int, default=0,
                        help="leaves of a decision tree over word-internal triphone states, trained after the single-Gaussian stages (0: none)")
    parser.add_argument("--tri_iters", type=int, default=4, help="Baum-Welch passes on the tied triphone states")
    parser.add_argument("--tri_min_occ", type=float, default=100, help="frames either side of a tree split must keep")
    parser.add_argument("--tri_min_gain", type=float, default=0.0, help="log-likelihood gain a tree split must exceed")
    parser.add_argument("--questions", type=str, default=None,
                        help="file of question sets, `name phone phone ...` per line (# is the word boundary); default: clustered from the data")
    parser.add_argument("--transitions", type=int, default=0, choices=(0, 1),
                        help="1: every Baum-Welch pass also trains the self-loop probability of every state and the probabilities of the "
                             "optional silences, and decoding uses them")
    parser.add_argument("--scores", type=str, default=None,
                        help="also write per-utterance and per-phone confidence scores (loglik, gop, match) to this JSONL file; no "
                             "threshold is applied and no TextGrid is dropped")
    parser.add_argument("--seg_scores", type=int, default=0, choices=(0, 1),
                        help="1 (needs --scores): also score every interval as a whole HMM of every phone and add gop_seg (Witt and "
                             "Young's definition), the best rival phone and the margin to every phone entry")
    parser.add_argument("--g2p_model", type=str, default=None,
                        help="a model trained by `python g2p.py train`: an out-of-lexicon word gets its pronunciation instead of spn")
    parser.add_argument("--save_model", type=str, default=None,
                        help="write the trained model to this .npz file (tables, options, phone table, feature settings, speaker names, "
                             "phone bigram counts) for --model and for recognize.py")
    parser.add_argument("--model", type=str, default=None,
                        help="align with this model file instead of training one (`mfa align`); training options beside it are an error, "
                             "and so are a lexicon or feature settings that are not the model's")
    parser.add_argument("--overwrite", action="store_true", help="replace TextGrids that exist already")
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--batch_gib", type=float, default=8.0, help="device buffers per ragged batch")
    parser.add_argument("--num_workers", type=int, default=8, help="host threads reading wav and .lab files")
    args = parser.parse_args()

    if args.seg_scores and args.scores is None:
        parser.error("--seg_scores 1 needs --scores FILE")
    config = yaml.load(open(args.config, "r"), Loader=yaml.FullLoader)
    try:
        written, skipped, history = build(config, device=args.device, states=args.states, iters=args.iters, overwrite=args.overwrite,
                                          batch_bytes=int(args.batch_gib * (1 << 30)), num_workers=args.num_workers, mixtures=args.mixtures,
                                          mix_iters=args.mix_iters, lda=args.lda, splice=args.splice, lda_iters=args.lda_iters,
                                          fmllr=args.fmllr, fmllr_rounds=args.fmllr_rounds, fmllr_iters=args.fmllr_iters,
                                          fmllr_sweeps=args.fmllr_sweeps, fmllr_min_frames=args.fmllr_min_frames,
                                          triphones=args.triphones, tri_iters=args.tri_iters, tri_min_occ=args.tri_min_occ,
                                          tri_min_gain=args.tri_min_gain, questions=args.questions, transitions=args.transitions, scores=args.scores,
                                          g2p=args.g2p_model, seg_scores=args.seg_scores, save_model=args.save_model, model=args.model)
    except FileExistsError as e:
        sys.exit(str(e))
    except ValueError as e:
        if args.model is None:
            raise
        sys.exit(str(e))
    print("log-likelihood per frame: " + " ".join("{:.4f}".format(h) for h in history))
    print("{} TextGrids written, {} utterances skipped".format(written, len(skipped)))
    if args.scores is not None:
        print(scores_summary(args.scores))
