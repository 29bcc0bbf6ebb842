"""DAVIS J&F of mask folders that already exist -- a host-egress run, another method's output -- through the scorer of ``eval_vos --score``
(cutie_amd/inference/utils/davis_metrics.py: the counts come from the GPU stage PROB_TO_ID flags == 64, the arithmetic is davis2017's).

    python -m cutie_amd.score_masks --results OUT/Annotations --gt DIR/Annotations [--dataset NAME] [--output DIR] [--score-all-frames]

``--results`` and ``--gt`` hold one folder of palette PNGs per video, ``<video>/<frame>.png``; a video without ground truth is left out, a
frame without ground truth is skipped.  Writes global_results-<dataset>.csv, per-sequence_results-<dataset>.csv and scores.json into
``--output`` (default: ``--results``) and prints the global line."""
import argparse
import logging
import os
from os import path

import numpy as np
import torch

from .inference.utils.davis_metrics import SequenceScorer, global_line, load_ids, write_results

log = logging.getLogger()


def score_folders(results, gt, *, dataset='generic', output=None, score_all_frames=False, device='cuda'):
    """-> (global figures, {video: scores}); the files go to ``output`` (default: ``results``)."""
    videos = sorted(v for v in os.listdir(results) if path.isdir(path.join(results, v)))
    per_sequence = {}
    for vid in videos:
        if not path.isdir(path.join(gt, vid)):
            log.warning(f'score_masks: no ground truth for {vid}; it is left out')
            continue
        scorer = SequenceScorer(gt, vid, device, skip_first_last=not score_all_frames)
        for name in sorted(f for f in os.listdir(path.join(results, vid)) if f.lower().endswith('.png')):
            ids = load_ids(path.join(results, vid, name))
            scorer.add(name, torch.from_numpy(np.ascontiguousarray(ids)).to(scorer.device))
        per_sequence[vid] = scorer.finish()
    glob = write_results(output or results, dataset, per_sequence)
    return glob, per_sequence


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument('--results', required=True, help='the predicted masks: DIR/<video>/<frame>.png')
    ap.add_argument('--gt', required=True, help='the ground truth: DIR/<video>/<frame>.png')
    ap.add_argument('--dataset', default='generic', help='the name in the result files')
    ap.add_argument('--output', help='where the result files go (default: --results)')
    ap.add_argument('--score-all-frames', action='store_true', help='also score the first and the last ground-truth frame of a video')
    return ap


def main():
    args = arg_parser().parse_args()
    glob, per_sequence = score_folders(args.results, args.gt, dataset=args.dataset, output=args.output, score_all_frames=args.score_all_frames)
    print(f'{args.dataset}: {global_line(glob)}   ({sum(v is not None for v in per_sequence.values())} sequences)')


if __name__ == '__main__':
    main()
