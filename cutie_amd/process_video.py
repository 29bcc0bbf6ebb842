"""Mask propagation through one video given a few annotated frames: the workflow of the reference scripts/process_video.py
(:22-211) on the HIP path.

1. every mask in ``--mask_dir`` (``<frame number, 7 digits>.png``; palette 'P', 'L' or RGB long ids) is committed to
   PERMANENT memory first: ``step(frame, one_hot[1:], idx_mask=False, force_permanent=True)`` (:94-120);
2. the video then runs from frame 0; frames that have a mask are stepped with it, the others propagate (:139-176); every
   output goes through ``ResultSaver`` (fused argmax + id remap on the device, PNG encoding on a writer thread); the next frame
   is uploaded one step ahead (``prefetch.Window``, depth 1) and the time is taken around ``step`` by ``eval_vos.timed_step``
   (device events on the GPU, wall seconds on a CPU device);
3. ``--mem_cleanup_ratio r``: when used / total device memory exceeds r the non-permanent memory is cleared (:214-228).

Frame source: a directory of images (sorted by name) or, when OpenCV is importable, a video file.  Differences from the
reference, on purpose: frames from a directory are RGB (the reference hands OpenCV's BGR arrays to the network unchanged,
:105,162); there is no CPU / MPS device switch -- the product has no CPU path; defaults are the reference's video_config.yaml
(long-term memory on, mem_every 10, max_internal_size 480).

    python -m cutie_amd.process_video -v FRAMES_DIR -m MASK_DIR -o OUT [--weights ckpt.pth] [--mem_every 10]
        [--max_internal_size 480] [--mem_cleanup_ratio 0.9] [--num_objects N] [--model small] [--ingest device] [--egress device]
        [--vis MODE [MODE ...]] [--soft-masks] [--alpha] [--target-objects ID [ID ...]] [--layer FILE]
        [--cutout] [--png-codes fixed|dynamic] [--refine-matte R [--refine-eps EPS]] [--trimap R_IN R_OUT] [--trimap-objects] [--dilate-mask R]
        [--redact blur|pixelate|fill [--redact-strength N] [--redact-color R G B] [--redact-grow R] [--redact-edge mask|matte] [--redact-background]]
        [--gt GT_DIR]      (prints the video's DAVIS J&F against GT_DIR/<frame number, 7 digits>.png, counted on the GPU: every frame that
                            has a ground-truth file is scored; cutie_amd/inference/utils/davis_metrics.py)

``--vis`` (davis | light | fade | popup | layer), ``--soft-masks``, ``--alpha``: the visualisations, per-object soft masks and the alpha
matte of the reference's interactive tool (gui/interactive_utils.py:79-229, gui/resource_manager.py:154-173), composed and encoded on
the GPU (ResultSaver vis_modes / soft_masks / alpha_matte) into OUT/visualization/<mode>/*.jpg, OUT/soft_masks/<object id>/*.png and
OUT/alpha/*.png.  ``--target-objects``: the objects that popup, layer and the matte keep (default all); ``--layer``: the RGBA image of
mode layer.  The uint8 frame the modes read is the one device ingest uploaded or decoded; with ``--ingest host`` it is made from the
float frame on the device, once per frame.

``--cutout``: the 'rgba' output of that tool (gui/interactive_utils.py:218-229) -- OUT/cutout/*.png, the frame as an RGBA PNG whose alpha is
the matte of the ``--target-objects``: the objects cut out, ready to composite.  Frame and matte are interleaved, filtered and coded with
dynamic Huffman codes on the GPU (csrc/png_photo.hip).  ``--png-codes dynamic`` sends the soft masks and the alpha matte through the same
encoder (the same pixels in fewer bytes); the default ``fixed`` keeps their bytes as they were.  The id masks never change encoder.

``--refine-matte R`` (with ``--refine-eps EPS``, default 1e-4): the matte of ``--alpha``, the alpha of ``--cutout`` and the planes of
``--soft-masks`` are probabilities computed at ``--max_internal_size`` and resampled to the frame: their edges are ramps on the coarse grid.
The colour guided filter (He, Sun, Tang) fits every plane, per window of radius R pixels, as an affine function of the frame's RGB and
averages the fits, which moves the planes' edges onto the frame's edges; it runs on the GPU between the planes and their PNG encoders
(ResultSaver matte_refine, csrc/guided.hip).  The id masks and the --vis JPEGs keep their bytes.

``--redact blur|pixelate|fill``: the footage itself, edited on the GPU -- OUT/redacted/*.jpg, every frame with the ``--target-objects`` (all
objects without it) blurred (three box passes of radius ``--redact-strength``, 1 .. 64, default 12), pixelated (cells of
``--redact-strength`` pixels, 2 .. 256, default 16) or painted with ``--redact-color R G B`` (default black).  ``--redact-grow R`` dilates
the objects' mask by the disk of R pixels first (0 .. 255: margins around faces and plates); ``--redact-edge matte`` blends under the soft
matte of the objects instead of the hard mask (the refined one with ``--refine-matte``); ``--redact-background`` inverts the weight:
everything but the objects takes the effect ("portrait mode").  ResultSaver redact, csrc/redact.hip, DESIGN.md section 26.

``--trimap R_IN R_OUT``, ``--trimap-objects``, ``--dilate-mask R``: what matting and inpainting models take next to the frame, as 8-bit
grey PNGs: OUT/trimap/*.png (255 sure foreground, 0 sure background, 128 the band of R_IN pixels inside and R_OUT pixels outside the edge
of the ``--target-objects``), one trimap per object in OUT/trimap_objects/<object id>/*.png, and the target objects dilated by the disk of
R pixels in OUT/dilated/*.png (0 | 255).  Exact Euclidean distances, measured on the GPU on the plane of the mask that is written
(ResultSaver trimap / trimap_objects / dilate_mask, csrc/edt.hip).

``--ingest device``: frames are read as uint8 and uploaded as such; ToTensor runs on the GPU (one RESIZE launch with flags 4,
cutie_amd/inference/data/device_ingest.py).  ``--ingest device-decode``: JPEG frames of a directory are parsed on the host and
decoded on the GPU (the other frames as with ``device``).  Any resize to max_internal_size stays InferenceCore's own."""
import os
import threading
from collections import Counter
from argparse import ArgumentParser
from os import path
from typing import Callable, Dict, Iterator, Optional, Tuple

import numpy as np
import torch
from PIL import Image

from .config import default_config
from .eval_vos import timed_step
from .inference.data import jpeg
from .inference.data.device_ingest import PngStaging, frame_to_device, jpeg_to_device, jpegs_to_device
from .inference.data.prefetch import ReadAhead, Window
from .inference.data.video_reader import INGEST_MODES
from .inference.inference_core import InferenceCore
from .inference.utils.results_utils import EGRESS_MODES, VIS_MODES, ResultSaver
from .inference.utils.polygons import PolygonReport
from .inference.utils.track_report import TrackReport

IMAGE_EXT = ('.jpg', '.jpeg', '.png', '.bmp')


def video_config(**overrides):
    """cutie/config/video_config.yaml: long-term memory on, mem_every 10, max_internal_size 480."""
    base = dict(use_long_term=True, mem_every=10, max_internal_size=480)
    base.update(overrides)
    return default_config(**base)


class FrameSource:
    """Random access + sequential reading of frames as float [3,H,W] in [0,1] (gui/interactive_utils.py:11-15), or with
    ``u8=True`` as the decoded uint8 [H,W,3] arrays (device ingest), with ``packets=True`` JPEG files of a directory as parsed
    packets (inference/data/jpeg.py; the others as uint8 arrays, counted by reason in ``decode_fallbacks``)."""

    def __init__(self, video: str, *, u8: bool = False, packets: bool = False):
        self.cap = None
        self.u8 = u8 or packets
        self.packets = packets
        self.decode_fallbacks = Counter()
        self._lock = threading.Lock()
        if path.isdir(video):
            self.names = sorted(n for n in os.listdir(video) if n.lower().endswith(IMAGE_EXT))
            self.root = video
            self.count = len(self.names)
        else:
            try:
                import cv2
            except ImportError as e:
                raise RuntimeError(f'{video} is not a directory of frames and OpenCV is not available to decode a video file') from e
            self.cv2 = cv2
            self.cap = cv2.VideoCapture(video)
            if not self.cap.isOpened():
                raise RuntimeError(f'Unable to open video {video}!')
            self.count = int(self.cap.get(cv2.CAP_PROP_FRAME_COUNT))

    def __len__(self):
        return self.count

    def read(self, index: int) -> Optional[torch.Tensor]:
        if self.cap is None:
            if not 0 <= index < self.count:
                return None
            if self.packets:
                pkt, why = jpeg.parse_file(path.join(self.root, self.names[index]))
                if pkt is not None:
                    return pkt
                with self._lock:
                    self.decode_fallbacks[why] += 1
            arr = np.array(Image.open(path.join(self.root, self.names[index])).convert('RGB'))
        else:
            self.cap.set(self.cv2.CAP_PROP_POS_FRAMES, index)
            ok, arr = self.cap.read()
            if arr is None:
                return None
            arr = arr[:, :, ::-1].copy()                          # BGR -> RGB
        if self.u8:
            return arr
        return torch.from_numpy(arr).permute(2, 0, 1).float() / 255

    def __iter__(self) -> Iterator[torch.Tensor]:
        # a directory decodes ahead on threads; a cv2.VideoCapture is a sequential, stateful decoder -> inline
        for f in ReadAhead(self, workers=4 if self.cap is None else 0, length=self.count, getitem=self.read):
            if f is None:
                return
            yield f

    def close(self):
        if self.cap is not None:
            self.cap.release()


def one_hot_planes(mask_np: np.ndarray, num_objects: int, device) -> torch.Tensor:
    """index mask -> float one-hot [num_objects, H, W] without the background plane
    (gui/interactive_utils.py:24-26 followed by ``[1:]``); ids above num_objects are an error there too."""
    m = torch.from_numpy(np.ascontiguousarray(mask_np)).long().to(device)
    if int(m.max()) > num_objects:
        raise RuntimeError(f'mask holds id {int(m.max())} but num_objects is {num_objects}')
    ids = torch.arange(1, num_objects + 1, device=device).view(-1, 1, 1)
    return (m.unsqueeze(0) == ids).float()


def check_to_clear_non_permanent_memory(processor: InferenceCore, mem_cleanup_ratio: float,
                                        mem_get_info: Callable[[], Tuple[int, int]] = None) -> bool:
    """scripts/process_video.py:214-228.  Returns True when a cleanup was triggered."""
    if not (0 < mem_cleanup_ratio <= 1):
        return False
    free, total = (mem_get_info or torch.cuda.mem_get_info)()
    ratio = (total - free) / total
    if ratio > mem_cleanup_ratio:
        print(f'GPU cleanup triggered: {ratio} > {mem_cleanup_ratio}')
        processor.clear_non_permanent_memory()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return True
    return False


def process_video(network, cfg, video: str, mask_dir: str, output_dir: str, *, num_objects: int = -1,
                  mem_cleanup_ratio: float = -1, mem_get_info=None, lookahead: bool = True, ingest: str = 'host', egress: str = 'host',
                  gt_dir: Optional[str] = None, gt_decode: str = 'host', vis_modes=(), soft_masks: bool = False, alpha_matte: bool = False, target_objects=None,
                  layer=None, decode_batch: int = 1, tracks: bool = False, min_region: int = 0, fill_holes: int = 0,
                  region_connectivity: int = 8, trimap=None, trimap_objects: bool = False, dilate_mask: float = 0.0, polygons: bool = False,
                  cutout: bool = False, png_codes: str = 'fixed', matte_refine=None, redact=None) -> Dict:
    """decode_batch = B > 1 (ingest='device-decode' only, ignored otherwise): B frames are decoded through one chain of launches
    (jpegs_to_device) and B frames wait on the device ahead of the step; the results are the same.
    gt_dir: ground-truth PNGs named like the outputs -- the video is scored on every frame that has one and 'scores' (SequenceScorer.finish)
    joins the result.  vis_modes / soft_masks / alpha_matte / target_objects / layer: ResultSaver's (the module docstring); 'folders' of
    the result names the folders they wrote.  tracks: area, box, centroid and confidence of every object on every frame, counted on the
    device (inference/utils/track_report.py): output_dir/tracks/tracks.json and tracks_mot.txt, and 'tracks' (the json's content) in the result.
    min_region / fill_holes / region_connectivity: ResultSaver's region filter -- small object components are dropped from every mask and
    small enclosed holes filled, on the device, before the mask is written, composed, tracked or scored; 'regions' (the totals) joins the
    result.  The model never sees the filtered plane.
    trimap = (r_in, r_out) / trimap_objects / dilate_mask = r: ResultSaver's -- output_dir/trimap/*.png (0 | 128 | 255) of the target objects
    (default all), one per object in trimap_objects/<id>/, and the target objects dilated by the disk of r pixels in dilated/*.png.
    polygons: every object's outline on every frame as exact rings of lattice corners, traced on the device (inference/utils/polygons.py):
    output_dir/polygons/polygons.json, and 'polygons' (the json's content) in the result.
    cutout: per frame output_dir/cutout/*.png, the frame as RGBA with the alpha matte of the target objects as its fourth channel (the
    'rgba' output of the reference's interactive tool), filtered and entropy-coded on the device.  png_codes = 'fixed' | 'dynamic':
    ResultSaver's -- 'dynamic' writes the soft masks and the alpha matte through that encoder too (the same pixels, fewer bytes).
    matte_refine = None | (r, eps): ResultSaver's -- the matte, the cut-out's alpha and the soft masks pass the colour guided filter with
    the frame as the guide (radius r pixels, eps on the [0, 1] scale) before they are encoded; the id masks and the JPEGs keep their bytes.
    redact = None | dict: ResultSaver's -- per frame output_dir/redacted/*.jpg, the frame with the target objects (or, with background=True,
    everything but them) blurred, pixelated or filled on the device."""
    if ingest not in INGEST_MODES:
        raise ValueError(f'ingest must be one of {INGEST_MODES}, not {ingest!r}')
    dev = network.device
    vis_modes = tuple(vis_modes)
    want_u8 = bool(vis_modes) or bool(cutout) or matte_refine is not None or redact is not None   # the modes, the cut-out, the guided filter and the redaction read the uint8 frame
    src = FrameSource(video, u8=(ingest == 'device'), packets=(ingest == 'device-decode'))

    def upload(f):
        """-> (frame on the device, its deferred decode check or None[, the uint8 frame on the device: with want_u8])"""
        if isinstance(f, jpeg.Packet):
            return jpeg_to_device(f, dev, check=False, keep_u8=want_u8)      # (a bad frame raises, naming its file, when it is checked)
        if ingest == 'host' or not want_u8:
            return (f.to(dev) if ingest == 'host' else frame_to_device(f, dev)), None
        frame, u8 = frame_to_device(f, dev, keep_u8=True)
        return frame, None, u8

    if decode_batch < 1:
        raise ValueError(f'decode_batch must be at least 1, not {decode_batch}')
    batch = decode_batch if ingest == 'device-decode' else 1
    staging = PngStaging() if (batch > 1 and dev.type == 'cuda') else None

    def upload_many(frames, owners):
        """``upload`` for the frames that enter the window together: the parsed JPEGs among them are decoded by ONE chain of launches"""
        items = [None] * len(frames)
        ks = [k for k, f in enumerate(frames) if isinstance(f, jpeg.Packet)]
        if ks:
            outs, chk, u8s = jpegs_to_device([frames[k] for k in ks], dev, check=False, keep_u8=True, staging=staging)
            for j, k in enumerate(ks):
                items[k] = (outs[j], chk.one(j), u8s[j]) if want_u8 else (outs[j], chk.one(j))
        return [upload(f) if item is None else item for f, item in zip(frames, items)]

    def checked(item):
        """-> (frame, its uint8 twin on the device or None)"""
        frame, chk = item[0], item[1]
        if chk is not None:
            chk()
        return frame, (item[2] if len(item) > 2 else None)

    def frame_u8(frame, u8):
        """The uint8 [H, W, 3] frame on the device: the one ingest kept, or -- host ingest -- the float frame quantised on the device
        (v * 255 + 0.5 truncated: the byte that ToTensor divided by 255)."""
        if u8 is None:
            u8 = (frame * 255 + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        return u8
    mask_names = sorted(n for n in os.listdir(mask_dir) if n.lower().endswith('.png'))
    if not mask_names:
        raise RuntimeError('No mask frames found!')
    first = Image.open(path.join(mask_dir, mask_names[0]))
    if first.mode == 'P':
        use_long_id, palette = False, first.getpalette()
    elif first.mode == 'RGB':
        use_long_id, palette = True, None
    elif first.mode == 'L':
        use_long_id, palette = False, None
    else:
        raise RuntimeError(f'Unknown mode {first.mode} in {mask_names[0]}.')

    def index_mask(name):
        arr = np.array(Image.open(path.join(mask_dir, name)))
        if use_long_id:
            arr = arr.astype(np.int64)
            arr = arr[..., 0] + 256 * arr[..., 1] + 65536 * arr[..., 2]
        return arr

    if num_objects is None or num_objects < 1:
        num_objects = len(np.unique(index_mask(mask_names[0]))) - 1
    processor = InferenceCore(network, cfg=cfg)
    with torch.inference_mode():
        # 1. commit the annotated frames to permanent memory
        for name in mask_names:
            frame = src.read(int(name[:-4]))
            if frame is None:
                break
            item = upload(frame) if batch == 1 else upload_many([frame], None)[0]
            processor.step(checked(item)[0], one_hot_planes(index_mask(name), num_objects, dev), idx_mask=False,
                           force_permanent=True)
        # 2. the whole video
        scorer = None
        if gt_dir is not None:
            from .inference.utils.davis_metrics import SequenceScorer
            scorer = SequenceScorer(gt_dir, '', dev, skip_first_last=False, gt_decode=gt_decode)
        saver = ResultSaver(output_dir, '', dataset='', object_manager=processor.object_manager, use_long_id=use_long_id,
                            palette=palette, processor=processor, egress=egress, scorer=scorer, vis_modes=vis_modes, soft_masks=soft_masks,
                            alpha_matte=alpha_matte, target_objects=target_objects, layer=layer,
                            tracks=TrackReport(path.basename(path.normpath(video))) if tracks else None,
                            min_region=min_region, fill_holes=fill_holes, region_connectivity=region_connectivity,
                            trimap=trimap, trimap_objects=trimap_objects, dilate_mask=dilate_mask,
                            polygons=PolygonReport(path.basename(path.normpath(video))) if polygons else None, cutout=cutout, png_codes=png_codes,
                            **({} if matte_refine is None else dict(matte_refine=matte_refine)), **({} if redact is None else dict(redact=redact)))
        total, n, cleanups = 0.0, 0, 0
        try:
            # the next frame is on the device while this one is stepped (decode_batch B: the next B frames, uploaded B at a time)
            ahead = Window(src, upload, checked, 1) if batch == 1 else Window(src, None, checked, 1, upload_many=upload_many, batch=batch)
            while ahead.queued:
                frame, u8 = ahead.pop()
                name = f'{n:07d}.png'
                mask = one_hot_planes(index_mask(name), num_objects, dev) if path.exists(path.join(mask_dir, name)) else None
                hint = ahead.queued[0][0] if (lookahead and ahead.queued) else None
                prob, secs = timed_step(lambda: processor.step(frame, mask, idx_mask=False, next_image=hint) if mask is not None
                                        else processor.step(frame, next_image=hint), dev.type == 'cuda')
                total += secs
                saver.process(prob, name, resize_needed=False, shape=None, last_frame=(n == len(src) - 1), path_to_image=None,
                              image_u8=frame_u8(frame, u8) if want_u8 else None, frame_index=n + 1)
                cleanups += check_to_clear_non_permanent_memory(processor, mem_cleanup_ratio, mem_get_info)
                n += 1
        finally:
            saver.end()
            src.close()
    out = {'frames': n, 'seconds': total, 'cleanups': cleanups, 'num_objects': num_objects, 'processor': processor}
    if scorer is not None:
        out['scores'] = saver.scores
    if tracks:
        out['tracks'] = saver.tracks.as_dict()
    if polygons:
        out['polygons'] = saver.polygons.as_dict()
    if saver.regions is not None:
        out['regions'] = saver.regions
    if vis_modes or soft_masks or alpha_matte or cutout or redact is not None:
        out['folders'] = ([path.join(output_dir, 'visualization', m) for m in vis_modes] + ([path.join(output_dir, 'soft_masks')] if soft_masks else []) +
                          ([path.join(output_dir, 'alpha')] if alpha_matte else []) + ([path.join(output_dir, 'cutout')] if cutout else []) +
                          ([path.join(output_dir, 'redacted')] if redact is not None else []))
    return out


def arg_parser() -> ArgumentParser:
    ap = ArgumentParser()
    ap.add_argument('-v', '--video', required=True, help='directory of frames (or a video file when OpenCV is available)')
    ap.add_argument('-m', '--mask_dir', required=True, help='masks named <frame number, 7 digits>.png')
    ap.add_argument('-o', '--output_dir', required=True)
    ap.add_argument('--weights')
    ap.add_argument('--num_objects', type=int, default=-1)
    ap.add_argument('--mem_every', type=int, default=10)
    ap.add_argument('--max_internal_size', type=int, default=480)
    ap.add_argument('--mem_cleanup_ratio', type=float, default=-1)
    ap.add_argument('--model', default='base', choices=['base', 'small'], help='cutie/config/model/{base,small}.yaml')
    ap.add_argument('--ingest', default='host', choices=list(INGEST_MODES), help='device: upload uint8 frames, ToTensor on the GPU; device-decode: decode JPEG frames on the GPU too')
    ap.add_argument('--decode-batch', type=int, default=1,
                    help='--ingest device-decode: decode this many frames through one chain of launches (default 1: one chain per frame; same results)')
    ap.add_argument('--egress', default='host', choices=list(EGRESS_MODES), help='device: the GPU writes the PNG streams of the masks (ResultSaver(egress=...))')
    ap.add_argument('--vis', nargs='+', default=[], choices=list(VIS_MODES), metavar='MODE',
                    help=f'visualisations written as OUT/visualization/MODE/*.jpg, composed and encoded on the GPU: {", ".join(VIS_MODES)}')
    ap.add_argument('--soft-masks', action='store_true', help='one 8-bit grey PNG per object and frame: OUT/soft_masks/<object id>/*.png')
    ap.add_argument('--alpha', action='store_true', help='the alpha matte of the target objects: OUT/alpha/*.png')
    ap.add_argument('--target-objects', nargs='+', type=int, metavar='ID', help='the objects popup, layer, the matte and the cut-out keep (default: all)')
    ap.add_argument('--cutout', action='store_true', help='the frame with the alpha matte of the target objects as its fourth channel: OUT/cutout/*.png (RGBA), encoded on the GPU')
    ap.add_argument('--png-codes', choices=('fixed', 'dynamic'), default='fixed',
                    help='the PNG encoder of the soft masks and the alpha matte: the id masks\' (fixed Huffman codes, default) or scanline filters + dynamic codes')
    ap.add_argument('--refine-matte', type=int, metavar='R', default=None,
                    help='refine the alpha matte, the cut-out\'s alpha and the soft masks with the colour guided filter under the frame: radius R, 1 .. 64 pixels')
    ap.add_argument('--refine-eps', type=float, metavar='EPS', default=None,
                    help='--refine-matte: the regulariser on the [0, 1] scale, 1e-6 .. 1 (default 1e-4); smaller follows the frame\'s edges more closely')
    ap.add_argument('--redact', choices=('blur', 'pixelate', 'fill'), default=None,
                    help='OUT/redacted/*.jpg: every frame with the --target-objects (all objects without it) blurred, pixelated or painted over, on the GPU')
    ap.add_argument('--redact-strength', type=int, metavar='N', default=None, help='--redact blur: the radius, 1 .. 64 (default 12); --redact pixelate: the cell size, 2 .. 256 (default 16)')
    ap.add_argument('--redact-color', type=int, nargs=3, metavar=('R', 'G', 'B'), default=None, help='--redact fill: the colour, three bytes (default 0 0 0)')
    ap.add_argument('--redact-grow', type=float, metavar='R', default=None, help='--redact: dilate the objects\' mask by the disk of R pixels first, 0 .. 255 (default 0)')
    ap.add_argument('--redact-edge', choices=('mask', 'matte'), default=None,
                    help='--redact: blend under the hard mask (default) or under the soft matte of the objects (the refined one with --refine-matte)')
    ap.add_argument('--redact-background', action='store_true', help='--redact: everything BUT the objects takes the effect (background blur)')
    ap.add_argument('--layer', metavar='FILE', help='the RGBA image of --vis layer (resized to the frames)')
    ap.add_argument('--gt-decode', choices=('host', 'device'), default='host',
                    help='--gt: device = the ground-truth PNGs are decoded on the GPU (default host: PIL)')
    ap.add_argument('--gt', help='ground-truth masks named like the outputs: prints the DAVIS J&F of the video (every frame that has one is scored)')
    ap.add_argument('--tracks', action='store_true',
                    help='OUT/tracks/tracks.json and tracks_mot.txt: area, box, centroid and confidence of every object on every frame, counted on the GPU')
    ap.add_argument('--polygons', action='store_true',
                    help='OUT/polygons/polygons.json: every object of every frame as exact rings of lattice corners (outer rings and holes), traced on the GPU')
    ap.add_argument('--min-region', type=int, default=0, metavar='N',
                    help='drop object components of fewer than N pixels from every mask, on the GPU, before it is written, composed, tracked or scored (0, 1: off)')
    ap.add_argument('--fill-holes', type=int, default=0, metavar='N',
                    help='then fill enclosed background components of fewer than N pixels with the id left of their first pixel (0, 1: off)')
    ap.add_argument('--region-connectivity', type=int, choices=(4, 8), default=8, help='neighbours that connect a component: 4 or 8 (default)')
    ap.add_argument('--trimap', nargs=2, type=float, metavar=('R_IN', 'R_OUT'),
                    help='OUT/trimap/*.png (0 | 128 | 255): the band of R_IN pixels inside and R_OUT pixels outside the edge of the --target-objects '
                         '(default all) is unknown; exact Euclidean distances, measured on the GPU; radii 0 .. 255')
    ap.add_argument('--trimap-objects', action='store_true', help='with --trimap: one trimap per object as well, OUT/trimap_objects/<object id>/*.png')
    ap.add_argument('--dilate-mask', type=float, default=0.0, metavar='R', help='OUT/dilated/*.png (0 | 255): the --target-objects (default all) dilated by the disk of R pixels; 0 .. 255')
    return ap


def refine_args(ap, args):
    """--refine-matte / --refine-eps -> ResultSaver's matte_refine (None | (r, eps)); a bad combination is the parser's error."""
    if args.refine_matte is None:
        if args.refine_eps is not None:
            ap.error('--refine-eps needs --refine-matte')
        return None
    eps = 1e-4 if args.refine_eps is None else args.refine_eps
    if not 1 <= args.refine_matte <= 64:
        ap.error(f'--refine-matte: a radius of {args.refine_matte}, 1 .. 64')
    if not 1e-6 <= eps <= 1.0:
        ap.error(f'--refine-eps: {eps}, 1e-6 .. 1')
    if not (args.alpha or args.cutout or args.soft_masks):
        ap.error('--refine-matte refines the planes of --alpha, --cutout and --soft-masks: none of them is set')
    return (args.refine_matte, eps)


def redact_args(ap, args):
    """--redact and its companions -> ResultSaver's redact (None | dict); a bad combination is the parser's error."""
    extras = [name for name, on in (('--redact-strength', args.redact_strength is not None), ('--redact-color', args.redact_color is not None),
                                    ('--redact-grow', args.redact_grow is not None), ('--redact-edge', args.redact_edge is not None),
                                    ('--redact-background', args.redact_background)) if on]
    if args.redact is None:
        if extras:
            ap.error(f'{extras[0]} needs --redact')
        return None
    mode = args.redact
    strength = {'blur': 12, 'pixelate': 16, 'fill': 0}[mode] if args.redact_strength is None else args.redact_strength
    if mode == 'blur' and not 1 <= strength <= 64:
        ap.error(f'--redact blur: a radius (--redact-strength) of {strength}, 1 .. 64')
    if mode == 'pixelate' and not 2 <= strength <= 256:
        ap.error(f'--redact pixelate: a cell (--redact-strength) of {strength}, 2 .. 256')
    if mode == 'fill' and args.redact_strength is not None:
        ap.error('--redact fill has no strength')
    if args.redact_color is not None and mode != 'fill':
        ap.error(f'--redact-color is the colour of --redact fill, not of {mode}')
    color = tuple(args.redact_color) if args.redact_color is not None else (0, 0, 0)
    if any(not 0 <= v <= 255 for v in color):
        ap.error(f'--redact-color: three bytes, not {list(color)}')
    grow = 0.0 if args.redact_grow is None else args.redact_grow
    if not 0.0 <= grow <= 255.0:
        ap.error(f'--redact-grow: {grow} pixels, 0 .. 255')
    edge = args.redact_edge or 'mask'
    if edge == 'matte' and grow != 0.0:
        ap.error('--redact-grow dilates the id mask: with --redact-edge matte it must be 0')
    return dict(mode=mode, strength=strength, color=color, grow=grow, edge=edge, background=bool(args.redact_background),
                targets=None if args.target_objects is None else list(args.target_objects))


def main():
    ap = arg_parser()
    args = ap.parse_args()
    matte_refine = refine_args(ap, args)                        # (a bad combination ends here, before the model is loaded)
    redact = redact_args(ap, args)
    if 'layer' in args.vis and not args.layer:
        ap.error('--vis layer needs --layer FILE')
    if args.decode_batch < 1:
        ap.error('--decode-batch is at least 1')
    if args.decode_batch > 1 and args.ingest != 'device-decode':
        print(f'--decode-batch {args.decode_batch} only matters with --ingest device-decode; ignored')
        args.decode_batch = 1
    from .model.cutie import CUTIE
    cfg = video_config(model=args.model, mem_every=args.mem_every, max_internal_size=args.max_internal_size)
    net = CUTIE(cfg).cuda().eval()
    if args.weights:
        net.load_weights(torch.load(args.weights, map_location='cpu'))
    else:
        print('No model weights loaded. Are you sure about this?')
    r = process_video(net, cfg, args.video, args.mask_dir, args.output_dir, num_objects=args.num_objects,
                      mem_cleanup_ratio=args.mem_cleanup_ratio, ingest=args.ingest, egress=args.egress, gt_dir=args.gt, gt_decode=args.gt_decode,
                      vis_modes=args.vis, soft_masks=args.soft_masks, alpha_matte=args.alpha, target_objects=args.target_objects, layer=args.layer,
                      decode_batch=args.decode_batch, tracks=args.tracks, min_region=args.min_region, fill_holes=args.fill_holes,
                      region_connectivity=args.region_connectivity, trimap=args.trimap, trimap_objects=args.trimap_objects, dilate_mask=args.dilate_mask,
                      polygons=args.polygons, cutout=args.cutout, png_codes=args.png_codes, matte_refine=matte_refine, redact=redact)
    if args.gt is not None and r['scores'] is not None:
        from .inference.utils.davis_metrics import global_line, summarize
        print('J&F: ' + global_line(summarize({path.basename(path.normpath(args.video)): r['scores']})[0]))
    if r.get('regions') is not None:
        from .eval_vos import region_line
        print(region_line([r['regions']]))
    print(f'Total processing time: {r["seconds"]}\nTotal processed frames: {r["frames"]}\n'
          f'FPS: {r["frames"] / max(r["seconds"], 1e-9)}\nMax allocated memory (MB): {torch.cuda.max_memory_allocated() / 2 ** 20}')


if __name__ == '__main__':
    main()
