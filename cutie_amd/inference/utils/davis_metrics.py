"""DAVIS J&F from the integers of the device stage (PROB_TO_ID flags == 64, csrc/score.hip; ``OpList.jf_counts``): the float arithmetic of
davis2017-evaluation (metrics.py db_eval_iou / db_eval_boundary / db_statistics, evaluation.py, evaluation_method.py) on eight counts per
(frame, object), the scorer that gathers them while a video runs, and the result files.  Host side, numpy only.

Not in the reference: its docs/EVALUATION.md sends the PNG folder to davis2017-evaluation or vos-benchmark.  Those packages (and cv2 /
skimage, which they need) are not available to this project's tests, so the agreement with davis2017 is derived from its published
source, not run against it.  Two known differences from the package: ``statistics`` does not wrap its bin
edges at 256 frames; and the void label 255 of the ground truth is background for every object in the ground truth ONLY -- davis2017 also
hands the void mask to db_eval_iou / db_eval_boundary, which take the void pixels out of the prediction as well, so a prediction that
covers a void region loses J and F here and not there (DAVIS 2017 val / test-dev have no void pixels; DAVIS 2016-style masks can).

Columns of a counts row: 0 |pred & gt|, 1 |pred | gt|, 2 pred boundary pixels, 3 gt boundary pixels, 4 pred boundary pixels within the
radius of a gt boundary pixel, 5 gt boundary pixels within the radius of a pred boundary pixel, 6 pred area, 7 gt area."""
import json
import logging
import math
import os
from os import path

import numpy as np
import torch
from PIL import Image

log = logging.getLogger()

BOUND_TH = 0.008            # db_eval_boundary's bound_th: the match radius as a share of the image diagonal
GLOBAL_COLUMNS = ('J&F-Mean', 'J-Mean', 'J-Recall', 'J-Decay', 'F-Mean', 'F-Recall', 'F-Decay')


def bound_pix(H, W):
    """The match radius of F in pixels: ceil(0.008 * |(H, W)|) in float64 -- 8 at 480 x 854, 18 at 1080 x 1920, 36 at 2160 x 3840."""
    return int(math.ceil(BOUND_TH * math.sqrt(float(H) * float(H) + float(W) * float(W))))


def j_from_counts(counts):
    """counts int [..., 8] -> J float64 [...]: intersection over union, 1 where the union is empty."""
    c = np.asarray(counts, dtype=np.int64)
    inter, union = c[..., 0].astype(np.float64), c[..., 1].astype(np.float64)
    return np.where(union == 0, 1.0, inter / np.where(union == 0, 1.0, union))


def f_from_counts(counts):
    """counts int [..., 8] -> F float64 [...]: 2 p r / (p + r) of the boundary precision and recall; no boundary in the prediction
    with one in the ground truth is (p, r) = (1, 0), the other way round (0, 1), none in either (1, 1); F = 0 when p + r == 0."""
    c = np.asarray(counts, dtype=np.int64)
    n_p, n_g = c[..., 2], c[..., 3]
    mp, mg = c[..., 4].astype(np.float64), c[..., 5].astype(np.float64)
    p = np.where(n_p > 0, mp / np.maximum(n_p, 1), 1.0)
    r = np.where(n_g > 0, mg / np.maximum(n_g, 1), 1.0)
    p = np.where((n_p == 0) & (n_g > 0), 1.0, np.where((n_p > 0) & (n_g == 0), 0.0, p))
    r = np.where((n_p == 0) & (n_g > 0), 0.0, np.where((n_p > 0) & (n_g == 0), 1.0, r))
    s = p + r
    return np.where(s == 0, 0.0, 2 * p * r / np.where(s == 0, 1.0, s))


def statistics(values):
    """(mean, recall, decay) of one object's per-frame values, as db_statistics: recall = the share of values above 0.5; decay = the
    mean of the first of four bins minus the mean of the last, the bins' edges being round(linspace(1, N, 5) + 1e-10) - 1.  The edges
    are Python ints here: davis2017 casts them to uint8, which wraps for sequences of more than 256 frames -- that is not reproduced."""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    if n == 0:
        raise ValueError('statistics of no values')
    edges = [int(e) for e in (np.round(np.linspace(1, n, 5) + 1e-10) - 1)]
    bins = [v[edges[i]:edges[i + 1] + 1] for i in range(4)]
    return float(v.mean()), float((v > 0.5).mean()), float(bins[0].mean() - bins[3].mean())


def _stem(name):
    return path.splitext(path.basename(name))[0]


def load_ids(png_path):
    """A mask PNG as its palette indices (mode P) or grey values (mode L), uint8 [H, W]."""
    arr = np.array(Image.open(png_path))
    if arr.ndim != 2 or arr.dtype != np.uint8:
        raise ValueError(f'{png_path}: J&F scores palette or grey masks (ids below 256), not mode {Image.open(png_path).mode}')
    return arr


class SequenceScorer:
    """The counts of one sequence, gathered on the device while it runs.  The ground truth is ``gt_dir/video_name/<frame>.png``; the
    objects are 1 .. max id of the FIRST ground-truth frame (255, the void label, aside), as in davis2017.  ``add`` loads the frame's
    ground truth, uploads it and enqueues the stage into row t of an int32 [T, K, 8] device table on the caller's stream -- no
    synchronisation, nothing comes back; ``finish`` makes the one copy of the table.  ``skip_first_last``: the first and the last
    ground-truth frame of the sequence are not scored (the DAVIS semi-supervised protocol: the first is given, the last is left out).
    ``gt_decode='device'`` (default 'host': PIL): ``add`` parses the ground-truth file (inference/data/png_packet.py), uploads the few KB of
    its compressed bytes and enqueues the two PNG decode stages (RESIZE flags 64 / 128) in front of the J&F stage on the caller's stream.
    ``add`` itself adds no synchronisation for the frame it enqueues, but the decode's error word is looked at when its staging slot comes
    round again, four frames later: that is a WAIT on the status copy behind that frame's decode launch (about 7 ms of GPU work for a 480p
    mask alone in a launch), so from the fifth frame on ``add`` can block the issuing thread where the host route only waits for an upload.
    The check, there or in ``finish``, raises ValueError naming a corrupt file.  A file the parser declines is decoded by PIL as before and counted in ``gt_fallbacks`` by reason.
    The first ground-truth frame, which fixes the objects, is read on the host either way."""

    def __init__(self, gt_dir, video_name, device, *, skip_first_last=True, gt_decode='host'):
        from ... import ops as O
        if gt_decode not in ('host', 'device'):
            raise ValueError(f"score: gt_decode is 'host' or 'device', not {gt_decode!r}")
        self.video_name, self.device, self.skip_first_last = video_name, torch.device(device), skip_first_last
        self.gt_decode, self.gt_fallbacks, self.gt_device_frames, self._png_staging = gt_decode, {}, 0, None
        self.dir = path.join(gt_dir, video_name) if video_name else gt_dir
        if not path.isdir(self.dir):
            raise ValueError(f'score: no ground-truth folder {self.dir}')
        self.names = sorted(f for f in os.listdir(self.dir) if f.lower().endswith('.png'))
        if not self.names:
            raise ValueError(f'score: no ground-truth PNG in {self.dir}')
        self.index = {_stem(f): t for t, f in enumerate(self.names)}
        first = load_ids(path.join(self.dir, self.names[0]))
        first = first[first != 255]
        K = int(first.max()) if first.size else 0
        if K > O.OpList.JF_MAX_OBJECTS - 1:
            raise ValueError(f'score: {K} objects in {self.names[0]}, at most 254')
        self.objects = list(range(1, K + 1))
        self.table = torch.zeros((len(self.names), max(K, 1), 8), dtype=torch.int32, device=self.device)
        self.objs_dev = torch.tensor(self.objects or [1], dtype=torch.int32).to(self.device)
        self.seen = set()
        self._scratch = None
        self._staging, self._turn = [], 0          # pinned ground-truth buffers in turn, each with the event behind its upload

    STAGING = 4

    def _upload(self, gt):
        """The ground-truth plane on the device.  On a GPU it goes through one of a few pinned buffers with a non-blocking copy, so the
        stream is not waited for; a buffer is taken again only once its own upload has run (its event, four frames back)."""
        if self.device.type != 'cuda':
            return torch.from_numpy(np.ascontiguousarray(gt)).to(self.device)
        if self._staging and tuple(self._staging[0][0].shape) != gt.shape:
            for _, ev in self._staging:
                ev.synchronize()
            self._staging = []
        if len(self._staging) < self.STAGING:
            self._staging.append((torch.empty(gt.shape, dtype=torch.uint8).pin_memory(), torch.cuda.Event()))
            host, ev = self._staging[-1]
        else:
            host, ev = self._staging[self._turn % self.STAGING]
            ev.synchronize()
        self._turn += 1
        host.numpy()[...] = gt
        dev = host.to(self.device, non_blocking=True)
        ev.record()
        return dev

    def _parse(self, gt_path):
        """gt_decode='device': the file's packet, or None -- counted by reason -- when it goes the host way (a format the parser declines,
        or a mode that load_ids refuses: its error is PIL's route's to raise)."""
        from ..data import png_packet as P
        pkt, why = P.parse_file(gt_path)
        if pkt is not None and len(pkt.shape) != 2:
            pkt, why = None, 'not a palette or grey mask'
        if pkt is None:
            self.gt_fallbacks[why] = self.gt_fallbacks.get(why, 0) + 1
            P.count_fallback(why)
        return pkt

    def _decode(self, pkt):
        """The ground-truth plane decoded on the device, on the caller's stream (device_ingest.png_to_device: one upload through a pinned
        slot, two launches); the check stays with the slot."""
        from ..data import device_ingest as DI
        if self._png_staging is None:
            self._png_staging = DI.PngStaging(self.STAGING)
        (gt_dev,), _ = DI.png_to_device([pkt], self.device, check=False, staging=self._png_staging)
        self.gt_device_frames += 1
        return gt_dev

    def gt_path(self, frame_name):
        """The ground-truth file of a frame, or None."""
        t = self.index.get(_stem(frame_name))
        return None if t is None else path.join(self.dir, self.names[t])

    def add(self, frame_name, ids_dev, gt_dev=None):
        """One frame: ``ids_dev`` = its predicted ids, uint8 [H, W] on the scorer's device.  A frame without ground truth is skipped.
        ``gt_dev``: the frame's ground truth, already a uint8 [H, W] plane on the device (score_masks decodes whole batches) -- nothing
        is loaded then."""
        from ... import ops as O
        t = self.index.get(_stem(frame_name))
        if t is None or not self.objects:
            return
        gt_path = path.join(self.dir, self.names[t])
        pkt = self._parse(gt_path) if (self.gt_decode == 'device' and gt_dev is None) else None
        gt = load_ids(gt_path) if (pkt is None and gt_dev is None) else None
        H, W = int(ids_dev.shape[-2]), int(ids_dev.shape[-1])
        gt_shape = tuple(gt_dev.shape) if gt_dev is not None else (tuple(gt.shape) if pkt is None else pkt.shape)
        if gt_shape != (H, W):
            raise ValueError(f'score: {self.video_name}/{self.names[t]} is {gt_shape[0]} x {gt_shape[1]}, the prediction {H} x {W}')
        if ids_dev.dtype != torch.uint8:
            raise ValueError(f'score: predicted ids are uint8, not {ids_dev.dtype}')
        pred = ids_dev.reshape(H, W)
        if not pred.is_contiguous():
            pred = pred.contiguous()
        if gt_dev is None:
            gt_dev = self._upload(gt) if pkt is None else self._decode(pkt)
        elif gt_dev.dtype != torch.uint8 or not gt_dev.is_contiguous():
            raise ValueError('score: the ground-truth plane is a contiguous uint8 [H, W]')
        K = len(self.objects)
        if self._scratch is None or self._scratch[0] != (H, W):
            self._scratch = ((H, W), torch.empty(O.OpList.jf_scratch_words(H, W, K), dtype=torch.int32, device=self.device))
        ol = O.OpList()
        ol.jf_counts(pred, gt_dev, self.objs_dev, self.table[t], self._scratch[1], H=H, W=W, radius=bound_pix(H, W))
        ol.run()
        self.seen.add(t)

    def finish(self):
        """-> {'objects': [ids], 'frames': [names], 'counts': [t][k][8] ints, 'J': [t][k], 'F': [t][k]} of the scored frames, or None
        (reported) when there is none."""
        T = len(self.names)
        if self._png_staging is not None:
            self._png_staging.finish()                           # a corrupt ground-truth file raises here at the latest
        scored = [t for t in sorted(self.seen) if not (self.skip_first_last and t in (0, T - 1))]
        if not scored or not self.objects:
            log.warning(f'score: {self.video_name or self.dir} has no scored frame ({len(self.objects)} objects, {len(self.seen)} frames with '
                        f'ground truth); it is left out')
            return None
        want = [t for t in range(T) if not (self.skip_first_last and t in (0, T - 1))]
        if len(scored) != len(want):
            log.warning(f'score: {self.video_name or self.dir}: {len(want) - len(scored)} ground-truth frames have no prediction and are not scored')
        counts = self.table.cpu().numpy()[scored]                  # the one copy
        return {'objects': list(self.objects), 'frames': [self.names[t] for t in scored], 'counts': counts.tolist(),
                'J': j_from_counts(counts).tolist(), 'F': f_from_counts(counts).tolist()}


def summarize(per_sequence):
    """{sequence: scores of SequenceScorer.finish} -> (global {column: value}, rows [(name '<seq>_<id>', J-Mean, F-Mean)]): every global
    figure is the mean over all (sequence, object) pairs of the per-object statistic; J&F-Mean = (J-Mean + F-Mean) / 2."""
    rows, stats = [], []
    for seq in sorted(per_sequence):
        sc = per_sequence[seq]
        if sc is None:
            continue
        J, F = np.asarray(sc['J'], dtype=np.float64), np.asarray(sc['F'], dtype=np.float64)
        for k, oid in enumerate(sc['objects']):
            sj, sf = statistics(J[:, k]), statistics(F[:, k])
            rows.append((f'{seq}_{oid}', sj[0], sf[0]))
            stats.append(sj + sf)
    if not stats:
        raise ValueError('score: no sequence was scored')
    m = np.mean(np.asarray(stats, dtype=np.float64), axis=0)
    glob = dict(zip(GLOBAL_COLUMNS, [float((m[0] + m[3]) / 2)] + [float(v) for v in m]))
    return glob, rows


def write_results(out_dir, dataset, per_sequence):
    """global_results-<dataset>.csv, per-sequence_results-<dataset>.csv (both '%.3f', as davis2017's evaluation_method.py writes them)
    and scores.json (full precision and the integer counts) into ``out_dir`` -> the global figures."""
    glob, rows = summarize(per_sequence)
    os.makedirs(out_dir, exist_ok=True)
    with open(path.join(out_dir, f'global_results-{dataset}.csv'), 'w') as f:
        f.write(','.join(GLOBAL_COLUMNS) + '\n' + ','.join('%.3f' % glob[c] for c in GLOBAL_COLUMNS) + '\n')
    with open(path.join(out_dir, f'per-sequence_results-{dataset}.csv'), 'w') as f:
        f.write('Sequence,J-Mean,F-Mean\n' + ''.join('%s,%.3f,%.3f\n' % r for r in rows))
    with open(path.join(out_dir, 'scores.json'), 'w') as f:
        json.dump({'dataset': dataset, 'global': glob, 'per_object': {n: {'J-Mean': j, 'F-Mean': fm} for n, j, fm in rows},
                   'sequences': {s: v for s, v in sorted(per_sequence.items()) if v is not None}}, f)
    return glob


def global_line(glob):
    return '  '.join(f'{c} {glob[c]:.3f}' for c in GLOBAL_COLUMNS)
