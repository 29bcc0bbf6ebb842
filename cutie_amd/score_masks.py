"""DAVIS J&F of mask folders that already exist -- a host-egress run, another method's output -- through the scorer of ``eval_vos --score``
(cutie_amd/inference/utils/davis_metrics.py: the counts come from the GPU stage PROB_TO_ID flags == 64, the arithmetic is davis2017's).

    python -m cutie_amd.score_masks --results OUT/Annotations --gt DIR/Annotations [--dataset NAME] [--output DIR] [--score-all-frames]
        [--decode host|device]    (device: predictions AND ground truth are inflated and unfiltered on the GPU, a batch of frames per launch --
                                   inference/data/png_packet.py, device_ingest.png_to_device; the host only parses the containers.  Same
                                   result files.  Default host: PIL.)

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


DECODE_BATCH = 16            # frames per decode launch with decode='device' (two images each: prediction and ground truth)
decode_fallbacks = {}        # decode='device': files that went through PIL after all, by the parser's reason (summed over the process)


def _planes_on_device(files, device, staging):
    """decode='device': the uint8 [H, W] planes of ``files`` on the device -- every file the parser takes in ONE upload and one launch per
    decode stage, the others through PIL -- and the deferred check of the launch (or None)."""
    from .inference.data import device_ingest as DI, png_packet as P
    planes, packets, where = [None] * len(files), [], []
    for k, f in enumerate(files):
        pkt, why = P.parse_file(f)
        if pkt is not None and len(pkt.shape) != 2:
            pkt, why = None, 'not a palette or grey mask'
        if pkt is None:
            decode_fallbacks[why] = decode_fallbacks.get(why, 0) + 1
            P.count_fallback(why)
            planes[k] = torch.from_numpy(np.ascontiguousarray(load_ids(f))).to(device)
        else:
            packets.append(pkt)
            where.append(k)
    chk = None
    if packets:
        decoded, chk = DI.png_to_device(packets, device, check=False, staging=staging)
        for k, plane in zip(where, decoded):
            planes[k] = plane
    return planes, chk


def score_folders(results, gt, *, dataset='generic', output=None, score_all_frames=False, device='cuda', decode='host'):
    """-> (global figures, {video: scores}); the files go to ``output`` (default: ``results``).  decode='device': the PNGs of both folders
    are decoded on the GPU, DECODE_BATCH frames per launch; the result files equal the host mode's."""
    if decode not in ('host', 'device'):
        raise ValueError(f"score_masks: decode is 'host' or 'device', not {decode!r}")
    videos = sorted(v for v in os.listdir(results) if path.isdir(path.join(results, v)))
    per_sequence = {}
    staging = None
    if decode == 'device':
        from .inference.data.device_ingest import PngStaging
        staging = PngStaging(2)
    for vid in videos:
        if not path.isdir(path.join(gt, vid)):
            log.warning(f'score_masks: no ground truth for {vid}; it is left out')
            continue
        scorer = SequenceScorer(gt, vid, device, skip_first_last=not score_all_frames)
        names = sorted(f for f in os.listdir(path.join(results, vid)) if f.lower().endswith('.png'))
        if decode == 'device':
            names = [n for n in names if scorer.gt_path(n) is not None and scorer.objects]      # (the others are skipped by `add` too)
            for o in range(0, len(names), DECODE_BATCH):
                part = names[o:o + DECODE_BATCH]
                files = [path.join(results, vid, n) for n in part] + [scorer.gt_path(n) for n in part]
                planes, _ = _planes_on_device(files, scorer.device, staging)
                for k, n in enumerate(part):
                    scorer.add(n, planes[k], gt_dev=planes[len(part) + k])
            staging.finish()                                  # a corrupt file raises ValueError with its name
        else:
            for name in names:
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
    ap.add_argument('--decode', choices=('host', 'device'), default='host',
                    help='device: the PNGs of both folders are inflated and unfiltered on the GPU, a batch of frames per launch (default host: PIL)')
    return ap


def main():
    args = arg_parser().parse_args()
    glob, per_sequence = score_folders(args.results, args.gt, dataset=args.dataset, output=args.output, score_all_frames=args.score_all_frames,
                                        decode=args.decode)
    print(f'{args.dataset}: {global_line(glob)}   ({sum(v is not None for v in per_sequence.values())} sequences)')


if __name__ == '__main__':
    main()
