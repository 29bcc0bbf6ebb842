"""Dataset-level driver: the loop of the reference cutie/eval_vos.py:85-171 without hydra (one InferenceCore per video,
first-mask alignment, ``end`` on the last frame, FPS = frames / sum of device-event time around ``step``), on top of
``VOSTestDataset`` / ``VideoReader`` / ``ResultSaver``.

Three drivers -- ``process_video``, ``process_video_multiscale``, ``process_videos_lockstep`` -- over one copy of each piece: ``_feed``
(decode threads -> the device look-ahead window, inference/data/prefetch.py ``Window``) and ``_take`` (a frame's record, mask, valid
labels and hints), ``timed_step`` (the FPS protocol), ``_saver`` / ``_save``, and ``_run_video``: the frames of one video on its
member cores -- the whole of the first two drivers and the tail of a lock-step group.

    python -m cutie_amd.eval_vos --images DIR/JPEGImages --masks DIR/Annotations --output OUT [--weights ckpt.pth]
        [--size 480] [--use-all-masks] [--long-term] [--dataset d17-val] [--visualize] [--clips-in-flight 2] [--lockstep 4]
        [--model small] [--flip-aug] [--save-scores] [--ingest device|device-decode [--decode-batch 8]] [--egress device] [--overlay device]      (multi-scale testing: one run per --size with --save-scores, then
                                           python -m cutie_amd.merge_multi_scale --list OUT_a OUT_b --output MERGED)
        [--sizes 480 600 720]              (multi-scale testing in ONE run: the scales of a video advance side by side and are merged on the GPU,
                                            no score files -- process_video_multiscale; excludes --size, --save-scores and --lockstep > 1)
        [--score [--gt DIR] [--score-all-frames] [--gt-decode host|device]]      (DAVIS J&F of the run against the palette PNGs of DIR/<video>/ -- default: --masks --,
                                            counted on the GPU from the id planes while the videos run (inference/utils/davis_metrics.py); writes
                                            global_results-<dataset>.csv, per-sequence_results-<dataset>.csv and scores.json into --output;
                                            the first and last ground-truth frame of a video are left out unless --score-all-frames)
        [--min-region N] [--fill-holes N] [--region-connectivity 4|8]
                                           (the region filter, on the GPU, on the id plane before anything reads it: object components
                                            below N pixels become background, then enclosed background components below N pixels get
                                            the id left of their first pixel (csrc/regions.hip); masks, RLE strings, overlays, --tracks
                                            and --score see the filtered plane, the model does not; not for long-id (RGB) masks)
        [--trimap R_IN R_OUT] [--trimap-objects] [--dilate-mask R]
                                           (what matting and inpainting models take: OUT/<video>/trimap/*.png (0 | 128 | 255: the band
                                            of R_IN pixels inside and R_OUT pixels outside the edge of all objects is unknown), one
                                            trimap per object in trimap_objects/<id>/, and all objects dilated by the disk of R pixels in
                                            dilated/*.png; exact Euclidean distances, measured on the GPU on the plane of the mask that is
                                            written (csrc/edt.hip); not for long-id (RGB) masks)
        [--tracks]                         (one row per object and saved frame -- area, box, centroid, confidence -- counted on the GPU from the id
                                            plane and the probabilities (inference/utils/track_report.py): OUT/tracks/<video>/tracks.json and
                                            tracks_mot.txt; with --sizes the confidence is null; not for long-id (RGB) masks)
        [--polygons]                       (every object of every saved frame as exact rings of lattice corners, traced on the GPU on the plane of
                                            the written mask (csrc/polygons.hip, inference/utils/polygons.py): OUT/polygons/<video>/polygons.json;
                                            --region-connectivity 8 joins diagonal pixels into one ring; not for long-id (RGB) masks)

BURST (a --dataset name containing "burst", e.g. burst-val | burst-test; eval_vos.py:42-54,108,156-157,171-172 of the reference):
    python -m cutie_amd.eval_vos --dataset burst-val --images DIR/frames/val --json DIR/val/first_frame_annotations.json --output OUT
        [--skip-frames N] [--size 600] [--egress device] [--lockstep 4] ...      (no --masks: the first masks are the json's RLE strings; no --sizes)
    masks are written on the annotated frames only, and OUT/predictions.json holds every sequence's RLE strings (BURSTResultHandler).

With several GPUs launch it under torch.distributed.run: videos are sharded over the ranks (cutie_amd/parallel.py)."""
import argparse
import logging
import os
import time
from contextlib import nullcontext
from os import path
from typing import Dict, List

import torch

from .config import default_config
from .inference.data.device_ingest import PngStaging, finish, to_device, to_device_many
from .inference.data.burst_test_dataset import BURSTTestDataset
from .inference.data.prefetch import ReadAhead, Window, fill_together, pop_together
from .inference.data.video_reader import INGEST_MODES
from .inference.data.vos_test_dataset import VOSTestDataset
from .inference.inference_core import InferenceCore
from .inference.utils.burst_utils import BURSTResultHandler
from .inference.utils.davis_metrics import SequenceScorer, global_line, write_results
from .inference.utils.results_utils import EGRESS_MODES, OVERLAY_MODES, ResultSaver, make_zip
from .inference.utils.polygons import PolygonReport
from .inference.utils.track_report import TrackReport

log = logging.getLogger()


def timed_step(fn, on_gpu):
    """-> (fn(), seconds): the reference's FPS protocol around one ``step`` (eval_vos.py:126-145: synchronize, event, step, event,
    synchronize); wall seconds on a CPU device."""
    if not on_gpu:
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0
    torch.cuda.synchronize()
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / 1000


def _check_ingest(ingest):
    if ingest is not None and ingest not in INGEST_MODES:
        raise ValueError(f'ingest must be one of {INGEST_MODES}, not {ingest!r}')


def _read_ahead(vid_reader, workers, ingest):
    """ReadAhead over the reader's records in the given ingest mode (None: the reader's own)."""
    if ingest is None:
        return ReadAhead(vid_reader, workers=workers)
    return ReadAhead(vid_reader, workers=workers, getitem=lambda i: vid_reader.get(i, ingest=ingest))


def _check_decode_batch(decode_batch, ingest_modes):
    """decode_batch > 1 is the batch JPEG decode of 'device-decode'; in every other mode it is ignored (-> 1; the command line says so once)."""
    decode_batch = int(decode_batch)
    if decode_batch < 1:
        raise ValueError(f'decode_batch must be at least 1, not {decode_batch}')
    return decode_batch if all(m == 'device-decode' for m in ingest_modes) else 1


def _feeds(vid_readers, dev, depth, read_workers, ingest, keep_u8s, decode_batch=1) -> List[Window]:
    """The records of each reader: decoded ahead on threads (eval_vos.py:92), then up to ``depth`` of them on the device ahead of the
    step that takes them (uploaded as they enter the window, their deferred decode check made as they leave it).  keep_u8s[k]: the
    device-ingest records of reader k keep their uint8 frame on the device (``info['image_u8']``: the device overlay of ``--visualize``
    reads it).  decode_batch = B > 1 ('device-decode'): the windows take B records at a time and fill TOGETHER -- one
    ``to_device_many`` call, i.e. one upload and one chain of decode launches, for the B frames of every feed that is due."""
    B = _check_decode_batch(decode_batch, [(ingest or rd.ingest) for rd in vid_readers])
    if B == 1:
        return [Window(_read_ahead(rd, read_workers, ingest), lambda d, k=k: to_device(d, dev, defer_check=True, keep_u8=k), finish, depth)
                for rd, k in zip(vid_readers, keep_u8s)]
    staging = PngStaging() if dev.type == 'cuda' else None            # pinned upload buffers of these feeds (one driver, one thread)

    def upload_many(records, owners):
        return to_device_many(records, dev, defer_check=True, keep_u8=[w.tag for w in owners], staging=staging)

    feeds = [Window(_read_ahead(rd, read_workers, ingest), None, finish, depth, upload_many=upload_many, batch=B, tag=k, fill=False)
             for rd, k in zip(vid_readers, keep_u8s)]
    fill_together(feeds)
    return feeds


def _take(windows, dev, lookahead):
    """The next frame of every feed -> per feed (record, its mask on the device or None, its valid labels or None, hints or None).  The
    hints are the frames of the following steps, already on the device: step(next_images=...) runs the image encoder over a window of
    them (InferenceCore.prefetch_window); the SAME tensors come with the later records (the look-ahead matches frames by storage)."""
    taken = []
    for window, d in zip(windows, pop_together(windows)):
        mask, valid = d.get('mask'), d.get('valid_labels')
        hints = [x['rgb'] for x in window.queued] if (lookahead and window.queued) else None
        taken.append((d, (mask.to(dev) if mask is not None else None), (valid.tolist() if valid is not None else None), hints))
    return taken


def _saver(core, vid_reader, mask_output_root, *, dataset, visualize, visualize_output_root, egress, save_scores=False,
           score_output_root=None, score_gt=None, score_all_frames=False, overlay='host', gt_decode='host', tracks=False,
           tracks_output_root=None, regions=None, bands=None, polygons=False, polygons_output_root=None) -> ResultSaver:
    """score_gt: the ground-truth root of a scored run (--score): the saver gets the video's SequenceScorer.
    tracks (--tracks): the saver gets the video's own TrackReport and writes it into tracks_output_root/<video>/ when it ends.
    regions (--min-region / --fill-holes / --region-connectivity): (min_region, fill_holes, connectivity) of the saver's region filter.
    bands (--trimap / --trimap-objects / --dilate-mask): (trimap, trimap_objects, dilate_mask) of the saver, over all objects.
    polygons (--polygons): the saver gets the video's own PolygonReport and writes it into polygons_output_root/<video>/ when it ends."""
    outlines = None
    if polygons:
        if vid_reader.use_long_id:
            raise ValueError(f'{vid_reader.vid_name}: long ids (RGB masks) have no uint8 id plane: no polygons')
        outlines = PolygonReport(vid_reader.vid_name)
    trimap, trimap_objects, dilate_mask = bands if bands is not None else (None, False, 0.0)
    if bands is not None and vid_reader.use_long_id:
        raise ValueError(f'{vid_reader.vid_name}: long ids (RGB masks) have no uint8 id plane: no trimap, no dilated mask')
    min_region, fill_holes, connectivity = regions if regions is not None else (0, 0, 8)
    if max(min_region, fill_holes) >= 2 and vid_reader.use_long_id:
        raise ValueError(f'{vid_reader.vid_name}: long ids (RGB masks) have no uint8 id plane: no region filter')
    report = None
    if tracks:
        if vid_reader.use_long_id:
            raise ValueError(f'{vid_reader.vid_name}: long ids (RGB masks) have no uint8 id plane: no track report')
        report = TrackReport(vid_reader.vid_name)
    scorer = None
    if score_gt is not None:
        if vid_reader.use_long_id:
            raise ValueError(f'{vid_reader.vid_name}: long ids (RGB masks) cannot be scored')
        scorer = SequenceScorer(score_gt, vid_reader.vid_name, core.network.device, skip_first_last=not score_all_frames, gt_decode=gt_decode)
    return ResultSaver(mask_output_root, vid_reader.vid_name, dataset=dataset, object_manager=core.object_manager,
                       use_long_id=vid_reader.use_long_id, palette=vid_reader.get_palette(), visualize=visualize,
                       visualize_output_root=visualize_output_root, processor=core, save_scores=save_scores,
                       score_output_root=score_output_root, egress=egress, scorer=scorer, overlay=overlay,
                       tracks=report, tracks_output_root=tracks_output_root,
                       min_region=min_region, fill_holes=fill_holes, region_connectivity=connectivity,
                       trimap=trimap, trimap_objects=trimap_objects, dilate_mask=dilate_mask,
                       polygons=outlines, polygons_output_root=polygons_output_root,
                       init_json=vid_reader.sequence_json if is_burst(dataset) else None)       # (eval_vos.py:108)


def is_burst(dataset: str) -> bool:
    return 'burst' in dataset.lower()


def _with_json(stats, saver):
    """BURST: the sequence's json with the predicted segmentations (complete once the saver has ended) joins the video's stats; so do the
    scores of a scored run."""
    if saver.json_style == 'burst':
        stats['video_json'] = saver.video_json
    if saver.scorer is not None:                 # a scored run: the video's counts and J / F per frame and object (None: nothing was scored)
        stats['scores'] = saver.scores
    if saver.tracks is not None:                 # --tracks: the video's report (what tracks.json holds), so that sharded ranks can gather them
        stats['tracks'] = saver.tracks.as_dict()
    if saver.polygons is not None:               # --polygons: the video's report (what polygons.json holds)
        stats['polygons'] = saver.polygons.as_dict()
    if saver.regions is not None:                # --min-region / --fill-holes: what the filter changed in the video
        stats['regions'] = saver.regions
    return stats


def _save(saver, prob, info, last_frame, save_all):
    if save_all or info['save']:
        saver.process(prob, info['frame'], resize_needed=info['resize_needed'], shape=info['shape'], last_frame=last_frame,
                      path_to_image=info['path_to_image'], **_frame_kw(saver, info))


def _frame_kw(saver, info) -> Dict:
    """overlay='device': the frame's uint8 original on the device, when the ingest kept it (``_feeds(keep_u8s=...)``).
    tracks: the frame's 1-based position in the video as the reader orders it."""
    kw = {'image_u8': info.get('image_u8')} if saver.overlay == 'device' else {}
    if (saver.tracks is not None or saver.polygons is not None) and info.get('time_index') is not None:
        kw['frame_index'] = int(info['time_index']) + 1
    return kw


def _run_video(members, feeds, n, start, stats, save, *, dev, lookahead):
    """Frames start .. n-1 of ONE video (eval_vos.py:97-151) on its member cores, stepped one after another per frame: one member for
    process_video and for a video that outlives its lock-step group, the S scales for process_video_multiscale.  members[s]() enters
    what member s runs in and gives its InferenceCore; feeds[s] is its window of records.  Frames before the first mask of a video
    that starts here are not stepped; ``end`` comes with the last frame; save(probs, info, last_frame) receives the members'
    probabilities of every stepped frame, which stay referenced until it returns.  stats: 'frames' += 1 per stepped frame, 'seconds'
    += the time around every member's step."""
    on_gpu = dev.type == 'cuda'
    first_mask_loaded = start > 0
    for ti in range(start, n):
        taken = _take(feeds, dev, lookahead)
        info = taken[0][0]['info']
        if any(d['info']['frame'] != info['frame'] or tuple(d['info']['shape']) != tuple(info['shape']) for d, *_ in taken):
            raise ValueError(f"process_video_multiscale: the readers disagree on frame {ti} ({[d['info']['frame'] for d, *_ in taken]})")
        if not first_mask_loaded:
            if taken[0][1] is None:
                continue                                  # nothing to do before the first mask
            first_mask_loaded = True
        probs = []
        for enter, (d, mask, valid, hints) in zip(members, taken):
            with enter() as core:
                prob, secs = timed_step(lambda: core.step(d['rgb'], mask, valid, end=(ti == n - 1), next_images=hints), on_gpu)
            probs.append(prob)
            stats['seconds'] += secs
        stats['frames'] += 1
        save(probs, info, ti == n - 1)


def process_video(network, cfg, vid_reader, mask_output_root, *, dataset='generic', save_all=True, visualize=False,
                  visualize_output_root=None, lookahead=True, save_scores=False, score_output_root=None,
                  read_workers=4, ingest=None, egress='host', score_gt=None, score_all_frames=False, overlay='host', gt_decode='host', decode_batch=1,
                  tracks=False, tracks_output_root=None, regions=None, bands=None, polygons=False, polygons_output_root=None) -> Dict:
    """One video through a fresh InferenceCore (eval_vos.py:97-151).  Returns {'frames', 'seconds'} (time around step).
    ingest: 'host' | 'device' | 'device-decode' (VideoReader(ingest=...); default: the reader's own mode).
    egress: 'host' | 'device' (``ResultSaver``'s ``egress``: the GPU writes the masks' PNG streams).
    overlay: 'host' | 'device' (``ResultSaver``'s ``overlay``: with ``visualize`` the GPU blends and writes the JPEGs' entropy-coded segments).
    score_gt: the root of the ground-truth PNGs -- the video is scored (J&F counts on the device, ``_saver``) and 'scores' joins the stats."""
    _check_ingest(ingest)
    from .inference import inference_core as IC
    processor = InferenceCore(network, cfg=cfg)
    saver = _saver(processor, vid_reader, mask_output_root, dataset=dataset, visualize=visualize, visualize_output_root=visualize_output_root,
                   egress=egress, save_scores=save_scores, score_output_root=score_output_root, score_gt=score_gt, score_all_frames=score_all_frames, gt_decode=gt_decode,
                   overlay=overlay, tracks=tracks, tracks_output_root=tracks_output_root, regions=regions, bands=bands,
                   polygons=polygons, polygons_output_root=polygons_output_root)
    stats = {'frames': 0, 'seconds': 0.0}
    try:
        feeds = _feeds([vid_reader], network.device, (IC.WINDOW + IC.WINDOW_LEAD + 1) if lookahead else 1, read_workers, ingest,
                       [saver.overlay == 'device'], decode_batch)
        _run_video([lambda: nullcontext(processor)], feeds, len(vid_reader), 0, stats,
                   lambda probs, info, last: _save(saver, probs[0], info, last, save_all), dev=network.device, lookahead=lookahead)
    finally:
        saver.end()
    return _with_json(stats, saver)


def process_video_multiscale(network, cfg, vid_readers, mask_output_root, *, dataset='generic', save_all=True, visualize=False,
                             visualize_output_root=None, lookahead=True, save_scores=False, score_output_root=None,
                             read_workers=4, ingest=None, egress='host', score_gt=None, score_all_frames=False, overlay='host', gt_decode='host', decode_batch=1,
                             tracks=False, tracks_output_root=None, regions=None, bands=None, polygons=False, polygons_output_root=None) -> Dict:
    """Multi-scale testing of ONE video in one pass (the reference: one eval_vos run per size with save_scores, then
    scripts/merge_multi_scale.py over the score dumps).  ``vid_readers``: S readers of the SAME video from S ``VOSTestDataset(size=s)``.
    One InferenceCore per member on the one network, stepped one after another per frame -- each with its own look-ahead window, memory
    and frame context (``ClipCores``); per member exactly ``process_video``'s handling (``_run_video``) -- and after the S steps of a frame
    ``ResultSaver.process_merged`` sums the members' quantised probabilities at the original size and writes the mask (one kernel; no
    score files, no full-size plane).
    The members' probabilities stay referenced until the merge has been issued: a pooled plan output that somebody holds is not recycled
    (plans.SlotPool), and everything runs on the caller's stream.  Returns {'frames', 'seconds'}; seconds = the sum over the members."""
    _check_ingest(ingest)
    if is_burst(dataset):
        raise ValueError('process_video_multiscale: BURST has no multi-scale protocol')
    if save_scores:
        raise ValueError('process_video_multiscale merges on the device and writes no scores: save_scores is not supported')
    from .inference import inference_core as IC
    from .inference.lockstep import ClipCores
    S = len(vid_readers)
    if S < 1:
        raise ValueError('process_video_multiscale needs at least one reader')
    rd0 = vid_readers[0]
    n = len(rd0)
    if any(rd.vid_name != rd0.vid_name or len(rd) != n for rd in vid_readers):
        raise ValueError('process_video_multiscale: the readers must be of the same video (name and length)')
    members = ClipCores(network, cfg, S)
    saver = _saver(members.cores[0], rd0, mask_output_root, dataset=dataset, visualize=visualize, visualize_output_root=visualize_output_root,
                   egress=egress, score_gt=score_gt, score_all_frames=score_all_frames, gt_decode=gt_decode, overlay=overlay,
                   tracks=tracks, tracks_output_root=tracks_output_root, regions=regions, bands=bands,
                   polygons=polygons, polygons_output_root=polygons_output_root)

    def save(probs, info, last_frame):
        if save_all or info['save']:
            saver.process_merged(probs, info['frame'], info['shape'], last_frame=last_frame, path_to_image=info['path_to_image'],
                                 id_maps=[{t: o.id for t, o in c.object_manager.tmp_id_to_obj.items()} for c in members.cores],
                                 **_frame_kw(saver, info))

    stats = {'frames': 0, 'seconds': 0.0}
    try:
        depth = (IC.WINDOW + IC.WINDOW_LEAD + 1) if lookahead else 1
        # (the first member's records carry the frame for the overlay: `save` gets its info)
        feeds = _feeds(vid_readers, network.device, depth, read_workers, ingest, [s == 0 and saver.overlay == 'device' for s in range(S)], decode_batch)
        _run_video([lambda s=s: members.clip(s) for s in range(S)], feeds, n, 0, stats, save, dev=network.device, lookahead=lookahead)
    finally:
        saver.end()
    return _with_json(stats, saver)


def lockstep_key(vid_reader):
    """What the videos of a lock-step group must share (cutie_amd/inference/lockstep.py): frame size as the model sees it, the number of
    objects of the first mask, the mask schedule.  None: the video cannot join a group (no mask on its first frame)."""
    d0 = vid_reader[0]
    if d0.get('mask') is None:
        return None
    hw = d0['rgb'].shape[-2:] if 'rgb' in d0 else d0['info']['rgb_shape']      # a device-ingest record: the shape it will have
    return (tuple(int(v) for v in hw), int(len(d0['valid_labels'])), bool(vid_reader.use_all_mask))


def lockstep_key_mixed(vid_reader):
    """``lockstep_key`` without the number of objects -- what the videos of a group share under --lockstep-mixed
    (``LockstepCores(mixed_objects=True)``): frame size and mask schedule.  None: no group for this video (no mask on its first frame, or
    more objects than a batched plan holds per clip)."""
    k = lockstep_key(vid_reader)
    if k is None or not 1 <= k[1] <= 7:
        return None
    return (k[0], k[2])


def lockstep_groups(mine, readers, lockstep, mixed=False):
    """The lock-step groups of the videos `mine` (indices into `readers`): videos that can advance together, longest first so that the videos
    of a group have similar lengths; groups of one video are left out (they run one by one).  mixed: grouped by frame size and mask
    schedule only, and the videos INSIDE a group sorted by object count -- the counts tuple keys the plans, so the fewer orders the fewer
    plans (and neighbours of one count share their conv launches, plans.Plan.conv)."""
    key = lockstep_key_mixed if mixed else lockstep_key
    by_key = {}
    for c in mine:
        k = key(readers[c])
        if k is not None:
            by_key.setdefault(k, []).append(c)
    grouped = []
    for k, cs in by_key.items():
        cs.sort(key=lambda c: -len(readers[c]))
        for g0 in range(0, len(cs) - 1, lockstep):
            grp = cs[g0:g0 + lockstep]
            if len(grp) >= 2:
                if mixed:
                    grp.sort(key=lambda c: lockstep_key(readers[c])[1])
                grouped.append(grp)
    return grouped


def process_videos_lockstep(network, cfg, vid_readers, mask_output_root, *, dataset='generic', save_all=True, visualize=False,
                            visualize_output_root=None, lookahead=True, save_scores=False, score_output_root=None, read_workers=4,
                            ingest=None, egress='host', score_gt=None, score_all_frames=False, overlay='host', gt_decode='host', decode_batch=1,
                            mixed_objects=False, tracks=False, tracks_output_root=None, regions=None, bands=None, polygons=False,
                            polygons_output_root=None) -> Dict[int, Dict]:
    """``process_video`` for a GROUP of videos advanced in lock step (``LockstepCores``: one launch plan per stage for the objects of all
    videos; per video the results of its own ``InferenceCore``).  The videos should share ``lockstep_key`` (mixed_objects: ``lockstep_key_mixed``
    -- their object counts may differ); they may differ in length -- the
    group runs as long as its shortest video, the others finish on their own cores.  Returns {index in vid_readers: {'frames', 'seconds'}}
    (the seconds of a lock-step frame are split evenly over its videos)."""
    _check_ingest(ingest)
    from .inference.lockstep import LockstepCores
    C = len(vid_readers)
    ls = LockstepCores(network, cfg, C, mixed_objects=mixed_objects)
    dev = network.device
    savers = [_saver(ls.cores[c], rd, mask_output_root, dataset=dataset, visualize=visualize, visualize_output_root=visualize_output_root,
                     egress=egress, save_scores=save_scores, score_output_root=score_output_root, score_gt=score_gt,
                     score_all_frames=score_all_frames, gt_decode=gt_decode, overlay=overlay, tracks=tracks,
                     tracks_output_root=tracks_output_root, regions=regions, bands=bands, polygons=polygons,
                     polygons_output_root=polygons_output_root) for c, rd in enumerate(vid_readers)]
    lens = [len(rd) for rd in vid_readers]
    T = min(lens)
    stats = {c: {'frames': 0, 'seconds': 0.0} for c in range(C)}
    try:
        feeds = _feeds(vid_readers, dev, 16 if lookahead else 1, read_workers, ingest, [sv.overlay == 'device' for sv in savers], decode_batch)
        for ti in range(T):
            data, masks, valid, hints = (list(v) for v in zip(*_take(feeds, dev, lookahead)))
            any_mask = any(m is not None for m in masks)
            hint = None
            if all(h is not None for h in hints) and not any_mask and ti < T - 1:
                n = min(min(len(h) for h in hints), T - 1 - ti)
                hint = [h[:n] for h in hints]
            end = all(ti == n_ - 1 for n_ in lens)          # (open, ADVICE.md: a shorter video of an unequal group never gets end=True)
            probs, secs = timed_step(lambda: ls.step([d['rgb'] for d in data], masks if any_mask else None, valid if any_mask else None,
                                                     end=end, next_images=hint), dev.type == 'cuda')
            for c in range(C):
                stats[c]['frames'] += 1
                stats[c]['seconds'] += secs / C
                _save(savers[c], probs[c], data[c]['info'], ti == lens[c] - 1, save_all)
        for c in range(C):                                   # the videos longer than the shortest one: on their own cores
            _run_video([lambda: ls.clip(c)], [feeds[c]], lens[c], T, stats[c],
                       lambda probs, info, last: _save(savers[c], probs[0], info, last, save_all), dev=dev, lookahead=lookahead)
    finally:
        for s in savers:
            s.end()
    for c in range(C):
        _with_json(stats[c], savers[c])
    return stats


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', required=True)
    ap.add_argument('--masks', help='the folder of first-frame masks (every dataset but BURST)')
    ap.add_argument('--json', help='BURST: the first-frame annotation json (its RLE strings are the first masks)')
    ap.add_argument('--skip-frames', type=int, default=-1, help='BURST: run on every N-th frame and the annotated ones (-1: on all)')
    ap.add_argument('--output', required=True)
    ap.add_argument('--weights')
    ap.add_argument('--dataset', default='generic')
    ap.add_argument('--size', type=int, default=-1)
    ap.add_argument('--sizes', type=int, nargs='+', default=None,
                    help='multi-scale testing in one run: at least two distinct --size values (-1: the original size); the scales of a video '
                         'advance side by side and their quantised scores are summed and argmaxed on the GPU (process_video_multiscale), '
                         'no score files.  Excludes --size, --save-scores and --lockstep > 1')
    ap.add_argument('--subset')
    ap.add_argument('--use-all-masks', action='store_true')
    ap.add_argument('--long-term', action='store_true')
    ap.add_argument('--visualize', action='store_true')
    ap.add_argument('--clips-in-flight', type=int, default=1)
    ap.add_argument('--lockstep-mixed', action='store_true',
                    help='--lockstep groups by frame size and mask schedule only: videos with different numbers of objects (1 .. 7) share the '
                         'batched plans (LockstepCores(mixed_objects=True); same results per video)')
    ap.add_argument('--lockstep', type=int, default=1, help='advance up to this many videos of one frame size / object count in LOCK STEP through one launch plan '
                                                            'per stage (cutie_amd/inference/lockstep.py; same results per video); the others run as --clips-in-flight says')
    ap.add_argument('--read-workers', type=int, default=4, help='decode threads per clip (0 = inline)')
    ap.add_argument('--flip-aug', action='store_true')
    ap.add_argument('--model', default='base', choices=['base', 'small'], help='cutie/config/model/{base,small}.yaml')
    ap.add_argument('--save-scores', action='store_true')
    ap.add_argument('--ingest', default='host', choices=list(INGEST_MODES),
                    help="device: upload the decoded uint8 frames, ToTensor + antialiased resize on the GPU (cutie_amd/inference/data/device_ingest.py); "
                         "device-decode: upload the JPEG bytes and decode them on the GPU as well (baseline JPEG; other frames as 'device')")
    ap.add_argument('--decode-batch', type=int, default=1,
                    help='--ingest device-decode: decode this many frames of a clip (of every clip of a --lockstep group, of every scale '
                         'of --sizes) through ONE chain of launches (RESIZE flags 256); the look-ahead windows grow by N - 1 frames.  '
                         'Same results.  Default 1: a launch chain per frame.  Ignored in the other ingest modes')
    ap.add_argument('--egress', default='host', choices=list(EGRESS_MODES),
                    help='device: the GPU resamples + argmaxes the result in one kernel and writes the PNG zlib stream; the host copies a few '
                         'KB per frame without blocking and only wraps them in PNG chunks (cutie_amd/inference/utils/results_utils.py)')
    ap.add_argument('--overlay', default='host', choices=list(OVERLAY_MODES),
                    help='--visualize: device = the GPU blends the object colours over the frame and writes the JPEG entropy-coded segment '
                         '(the same files as the host overlay; keeps --egress device; best with --ingest device | device-decode, which '
                         'leave the uint8 frame on the GPU -- with --ingest host every frame is decoded again and uploaded)')
    ap.add_argument('--score', action='store_true',
                    help='DAVIS J&F of the run, counted on the GPU while the videos run (cutie_amd/inference/utils/davis_metrics.py): writes '
                         'global_results-<dataset>.csv, per-sequence_results-<dataset>.csv and scores.json into --output.  Not for BURST or long-id (RGB) masks: '
                         'the first mask under --masks / --gt is peeked at for an early error, every video is checked when it starts')
    ap.add_argument('--gt', help='--score: the root of the ground-truth palette PNGs, DIR/<video>/<frame>.png (default: --masks)')
    ap.add_argument('--gt-decode', choices=('host', 'device'), default='host',
                    help='--score: device = the ground-truth PNGs are inflated and unfiltered on the GPU in front of the J&F stage '
                         '(inference/data/png_packet.py; a file the parser declines is decoded by PIL); default host: PIL on the issuing thread')
    ap.add_argument('--score-all-frames', action='store_true',
                    help='--score: also score the first and the last ground-truth frame of a video (the DAVIS protocol leaves them out)')
    ap.add_argument('--tracks', action='store_true',
                    help='per video OUT/tracks/<video>/tracks.json and tracks_mot.txt: area, box, centroid and confidence of every object on every '
                         'saved frame, counted on the GPU (cutie_amd/inference/utils/track_report.py).  With --sizes the confidence is null.  '
                         'Not for long-id (RGB) masks')
    ap.add_argument('--polygons', action='store_true',
                    help='per video OUT/polygons/<video>/polygons.json: every object of every saved frame as exact rings of lattice corners '
                         '(outer rings and holes), traced on the GPU on the plane of the written mask (csrc/polygons.hip; '
                         'cutie_amd/inference/utils/polygons.py); diagonal pixels join under --region-connectivity 8.  Not for long-id (RGB) masks')
    ap.add_argument('--min-region', type=int, default=0, metavar='N',
                    help='drop object components of fewer than N pixels from every result mask (on the GPU, before the mask is written, encoded, '
                         'overlaid, tracked or scored; csrc/regions.hip).  0 or 1: off.  Not for long-id (RGB) masks')
    ap.add_argument('--fill-holes', type=int, default=0, metavar='N',
                    help='fill enclosed background components of fewer than N pixels with the id left of their first pixel, after --min-region '
                         '(so a speck of one object inside another becomes the other).  0 or 1: off.  Not for long-id (RGB) masks')
    ap.add_argument('--trimap', nargs=2, type=float, metavar=('R_IN', 'R_OUT'),
                    help='per frame OUT/<video>/trimap/<frame>.png, an 8-bit grey PNG: 255 sure foreground (all objects), 0 sure background, 128 '
                         'the unknown band of R_IN pixels inside and R_OUT pixels outside the edge; exact Euclidean distances, measured on '
                         'the GPU on the plane of the written mask (csrc/edt.hip); radii 0 .. 255.  Not for long-id (RGB) masks')
    ap.add_argument('--trimap-objects', action='store_true', help='with --trimap: one trimap per object as well, OUT/<video>/trimap_objects/<object id>/<frame>.png')
    ap.add_argument('--dilate-mask', type=float, default=0.0, metavar='R',
                    help='per frame OUT/<video>/dilated/<frame>.png (0 | 255): all objects dilated by the disk of R pixels (what inpainting and '
                         'object-removal models take); 0 .. 255.  Not for long-id (RGB) masks')
    ap.add_argument('--region-connectivity', type=int, choices=(4, 8), default=8,
                    help='neighbours that connect the pixels of a component for --min-region and --fill-holes: 4 (edges) or 8 (edges and corners; default)')
    return ap


def _long_id_masks(masks_dir) -> bool:
    """Does the first mask of the first video under ``masks_dir`` hold long ids (an RGB PNG)?  A best-effort peek for an early
    ``ap.error`` -- one file is looked at, False when nothing can be read; the guard that holds for every video is ``_saver``'s ValueError."""
    from PIL import Image
    try:
        for vid in sorted(os.listdir(masks_dir)):
            pngs = sorted(f for f in os.listdir(path.join(masks_dir, vid)) if f.lower().endswith('.png'))
            if pngs:
                return Image.open(path.join(masks_dir, vid, pngs[0])).mode == 'RGB'
    except OSError:
        pass
    return False


def check_args(ap: argparse.ArgumentParser, args) -> None:
    """The rules between switches that argparse cannot state (ap.error: usage + exit status 2)."""
    if is_burst(args.dataset):
        if args.json is None:
            ap.error('a BURST dataset needs --json (the first-frame annotation file)')
        if args.sizes is not None:
            ap.error('--sizes: BURST has no multi-scale protocol')
    elif args.masks is None:
        ap.error('the following arguments are required: --masks')
    if args.score:
        if is_burst(args.dataset):
            ap.error('--score: BURST is not scored with J&F (its predictions.json goes to the BURST benchmark tools)')
        if args.gt is None:
            args.gt = args.masks
        if _long_id_masks(args.masks) or _long_id_masks(args.gt):
            ap.error('--score: long-id datasets (RGB masks) cannot be scored: J&F is counted on uint8 id planes')
    elif args.gt is not None or args.score_all_frames:
        ap.error('--gt and --score-all-frames belong to --score')
    if getattr(args, 'tracks', False) and args.masks is not None and _long_id_masks(args.masks):
        ap.error('--tracks: long-id datasets (RGB masks) have no uint8 id plane to count on')
    if getattr(args, 'polygons', False) and args.masks is not None and _long_id_masks(args.masks):
        ap.error('--polygons: long-id datasets (RGB masks) have no uint8 id plane to trace')
    if getattr(args, 'min_region', 0) < 0 or getattr(args, 'fill_holes', 0) < 0:
        ap.error('--min-region and --fill-holes are not negative')
    if max(getattr(args, 'min_region', 0), getattr(args, 'fill_holes', 0)) >= 2 and args.masks is not None and _long_id_masks(args.masks):
        ap.error('--min-region / --fill-holes: long-id datasets (RGB masks) have no uint8 id plane to label')
    radii = list(getattr(args, 'trimap', None) or ()) + [getattr(args, 'dilate_mask', 0.0)]
    if not all(0.0 <= r <= 255.0 for r in radii):
        ap.error('--trimap and --dilate-mask take radii of 0 .. 255 pixels')
    if getattr(args, 'trimap_objects', False) and max(getattr(args, 'trimap', None) or (0.0,)) <= 0.0:
        ap.error('--trimap-objects belongs to --trimap')
    if max(radii) > 0.0 and args.masks is not None and _long_id_masks(args.masks):
        ap.error('--trimap / --dilate-mask: long-id datasets (RGB masks) have no uint8 id plane to measure on')
    if getattr(args, 'decode_batch', 1) < 1:
        ap.error('--decode-batch is at least 1')
    if args.sizes is not None:
        if len(set(args.sizes)) != len(args.sizes) or len(args.sizes) < 2:
            ap.error('--sizes takes at least two distinct values')
        if any(v != -1 and v < 1 for v in args.sizes):
            ap.error('--sizes: a size is positive, or -1 for the original size')
        if len(args.sizes) > 8:
            ap.error('--sizes: at most 8 scales are merged in one launch')
        if args.size != -1:
            ap.error('--sizes and --size exclude each other')
        if args.save_scores:
            ap.error('--sizes merges on the GPU and writes no scores: it excludes --save-scores')
        if args.lockstep > 1:
            ap.error('--sizes does not run in lock step: it excludes --lockstep > 1 (use --clips-in-flight)')


def run_dataset(net, cfg, args, rank=0, world=1) -> Dict[int, Dict]:
    """The videos of this rank's shard through the drivers, as the switches say -> {index of the video: its stats}.  BURST: the
    sequences' predictions go to ``predictions.json`` in the output root (rank 0, the other ranks' sequences gathered)."""
    from .parallel import run_concurrent, shard_clips
    burst = is_burst(args.dataset)
    if burst:                                                 # (eval_vos.py:42-54; save_all is False there, eval_config.yaml)
        meta = BURSTTestDataset(args.images, args.json, size=args.size, skip_frames=args.skip_frames, ingest=args.ingest)
    else:
        meta = VOSTestDataset(args.images, args.masks, use_all_masks=args.use_all_masks, size=args.size, subset=args.subset,
                              ingest=args.ingest)
    readers = list(meta.get_datasets())
    mine = shard_clips(len(readers), rank, world)
    mask_root = path.join(args.output, 'Annotations')
    common = dict(dataset=args.dataset, visualize=args.visualize, visualize_output_root=path.join(args.output, 'Visualizations'),
                  save_scores=args.save_scores, score_output_root=path.join(args.output, 'Scores'), read_workers=args.read_workers,
                  egress=args.egress, save_all=not burst, overlay=getattr(args, 'overlay', 'host'))     # (no ingest=: the readers carry the mode)
    decode_batch = int(getattr(args, 'decode_batch', 1))
    if decode_batch > 1 and args.ingest != 'device-decode':
        log.warning('--decode-batch %d only matters with --ingest device-decode; ignored', decode_batch)
    elif decode_batch != 1:
        common.update(decode_batch=decode_batch)
    score = bool(getattr(args, 'score', False))
    if score:
        common.update(score_gt=args.gt or args.masks, score_all_frames=bool(args.score_all_frames), gt_decode=args.gt_decode)
    if getattr(args, 'tracks', False):                        # (off: no argument is passed and no launch is issued)
        common.update(tracks=True, tracks_output_root=path.join(args.output, 'tracks'))
    if getattr(args, 'polygons', False):                      # (off: no argument is passed and no launch is issued)
        common.update(polygons=True, polygons_output_root=path.join(args.output, 'polygons'),
                      regions=(0, 0, getattr(args, 'region_connectivity', 8)))             # (the connectivity of the rings; thresholds 0: no filter)
    filtered = max(getattr(args, 'min_region', 0), getattr(args, 'fill_holes', 0)) >= 2
    if filtered:                                              # (off: no argument is passed and no launch is issued)
        common.update(regions=(args.min_region, args.fill_holes, getattr(args, 'region_connectivity', 8)))
    trimap = tuple(getattr(args, 'trimap', None) or (0.0, 0.0))
    if max(trimap) > 0.0 or getattr(args, 'dilate_mask', 0.0) > 0.0:      # (off: no argument is passed and no launch is issued)
        common.update(bands=(trimap, bool(getattr(args, 'trimap_objects', False)), float(getattr(args, 'dilate_mask', 0.0))))
    run = lambda view, c: process_video(view, cfg, readers[c], mask_root, **common)
    if args.sizes is not None:
        # one dataset per scale over the same folders (`readers`, from --size -1, only counts the videos): member s of video c is
        # scales[s][c] -- every dataset lists the folder in the same sorted order
        scales = [list(VOSTestDataset(args.images, args.masks, use_all_masks=args.use_all_masks, size=sz, subset=args.subset,
                                      ingest=args.ingest).get_datasets()) for sz in args.sizes]
        run = lambda view, c: process_video_multiscale(view, cfg, [sc[c] for sc in scales], mask_root, **common)   # (check_args: no --save-scores here)
    res = {}
    with torch.inference_mode():
        if args.lockstep > 1 and not args.flip_aug:
            # groups of videos that can advance together (same frame size, object count and mask schedule), longest first so that the
            # videos of a group have similar lengths; what is left over runs one by one below
            # (--lockstep-mixed: same frame size and mask schedule only)
            grouped = lockstep_groups(mine, readers, args.lockstep, mixed=args.lockstep_mixed)
            for grp in grouped:
                st = process_videos_lockstep(net, cfg, [readers[c] for c in grp], mask_root, mixed_objects=args.lockstep_mixed, **common)
                for j, c in enumerate(grp):
                    res[c] = st[j]
            mine = [c for c in mine if c not in res]
        res.update(run_concurrent(net, mine, run, streams=max(1, args.clips_in_flight)))
    if burst:                                                 # (eval_vos.py:156-157,171-172)
        seqs = {c: r['video_json'] for c, r in res.items()}
        if world > 1:
            import torch.distributed as dist
            parts = [None] * world
            dist.all_gather_object(parts, seqs)
            seqs = {c: v for part in parts for c, v in part.items()}
        if rank == 0:
            handler = BURSTResultHandler(meta.json)
            for c in sorted(seqs):
                handler.add_sequence(seqs[c])
            os.makedirs(args.output, exist_ok=True)
            handler.dump(args.output)
    if score:                                                 # the videos' scores of all ranks -> the result files (rank 0)
        seqs = {readers[c].vid_name: r.get('scores') for c, r in res.items()}
        if world > 1:
            import torch.distributed as dist
            parts = [None] * world
            dist.all_gather_object(parts, seqs)
            seqs = {name: v for part in parts for name, v in part.items()}
        if rank == 0 and not any(v is not None for v in seqs.values()):
            log.warning('--score: no video had a scored frame; no result files are written')
        elif rank == 0:
            glob = write_results(args.output, args.dataset, seqs)
            print(f'{args.dataset}: {global_line(glob)}   ({sum(v is not None for v in seqs.values())} sequences)')
    if filtered:                                              # what the filter changed, with the run's summary (this rank's videos)
        print(f'rank {rank}: {region_line([r.get("regions") for r in res.values()])}')
    return res


def region_line(reports) -> str:
    """The totals of the videos' region-filter reports (``ResultSaver.regions``) as one line."""
    reports = [r for r in reports if r]
    t = {k: sum(r[k] for r in reports) for k in ('frames', 'islands_removed', 'pixels_cleared', 'holes_filled', 'pixels_filled')}
    return (f"region filter: {t['islands_removed']} islands removed ({t['pixels_cleared']} pixels), {t['holes_filled']} holes filled "
            f"({t['pixels_filled']} pixels) on {t['frames']} frames")


def main():
    ap = arg_parser()
    args = ap.parse_args()
    check_args(ap, args)
    from .model.cutie import CUTIE
    import torch.distributed as dist
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        dist.init_process_group(backend='nccl')
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    cfg = default_config(model=args.model, use_long_term=args.long_term, flip_aug=args.flip_aug, save_scores=args.save_scores)
    net = CUTIE(cfg).cuda().eval()
    if args.weights:
        net.load_weights(torch.load(args.weights, map_location='cpu'))
    res = run_dataset(net, cfg, args, rank, world)
    frames, secs = sum(r['frames'] for r in res.values()), sum(r['seconds'] for r in res.values())
    print(f'rank {rank}: {frames} frames, {secs:.2f} s in step, FPS {frames / max(secs, 1e-9):.1f}')
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        make_zip(args.dataset, args.output, 'cutie_amd', path.join(args.output, 'Annotations'))


if __name__ == '__main__':
    main()
