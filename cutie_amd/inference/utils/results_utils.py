"""``ResultSaver``: probabilities -> object-id masks -> palette PNGs on a writer thread; same surface as the reference
cutie/inference/utils/results_utils.py:30-256 (``process`` / ``end`` / ``make_zip``).

MI355X-side difference: argmax + tmp-id -> object-id remap run as ONE kernel (PROB_TO_ID) that writes uint8 (int32 for
long ids), so the device-to-host copy is H*W bytes instead of the (K+1)*H*W*4 bytes of probabilities, and the host thread
only encodes the PNG.  ``save_scores`` (multi-scale testing, :94,195-209): probabilities are quantised to uint8 (x255,
truncation) ON THE DEVICE, so the copy is 4x smaller too; the reference stores them with hickle (HDF5, lzf), which is not in
this image, so the container here is ``<frame>.npz`` (key ``prob``) and ``backward.npz`` (keys ``obj_ids`` / ``tmp_ids``) --
``cutie_amd.merge_multi_scale`` reads these (and ``.hkl`` when hickle is importable).
BURST (a dataset name containing 'burst', :67-74,153-171): ``init_json`` is the sequence's json; on its annotated frames every object
with a non-empty mask is recorded as ``{'rle': <COCO compressed RLE>}`` in ``segmentations`` / ``video_json`` (collected by
utils/burst_utils.py BURSTResultHandler).  The strings come from utils/coco_rle.py, not pycocotools -- the same bytes.
Long ids (RGB masks): as in the reference (:171-178) every object gets a random colour (utils/pano_utils.ID2RGBConverter), NOT the
inverse of VideoReader's R + 256 G + 65536 B decoding.  Behaviour recorded from the executed reference: tests/golden/io/.

``egress='device'`` (not in the reference): the mask leaves the GPU as a finished zlib stream instead of an id
plane.  One op list per frame on the caller's stream -- argmax + remap (fused with the bilinear resampling when the frame was resized on
the way in, so the full-size probabilities never exist) and the PNG filter + DEFLATE + Adler-32 stage (csrc/png.hip) -- then ONE
non-blocking copy of the status block and the first slab of the stream into pinned memory with an event behind it.  ``process`` does
not wait; the writer thread waits on the event, checks the error word, wraps the bytes (utils/png.py) and writes the file.  The files
hold the same mode, palette and pixels as the host path's; their bytes differ (other filter and Huffman codes, always 8 bits).
With BURST the same op list carries the RLE stage (csrc/rle.hip) over the id plane on annotated frames: the objects' strings, their
table and a status block ride a second pinned copy in front of the same event, and the writer thread slices the strings out; if the
strings did not fit the device stream the writer encodes that frame on the host from a copy of the id plane.

``overlay='device'`` (not in the reference): the ``visualize`` JPEGs leave the GPU as finished entropy-coded
segments.  While the id plane is still on the device -- behind the id stage of either egress mode -- one more op (PROB_TO_ID flags == 128,
csrc/jpeg_enc.hip) blends the object colours over the uint8 frame and encodes the result exactly as libjpeg-turbo would; status and
stream ride a pinned copy in front of the frame's event, and the writer thread wraps them (utils/jpeg_writer.py) into ``<frame>.jpg``:
the bytes of the host overlay's file.  The frame comes as ``image_u8`` (device ingest keeps it: device_ingest.to_device(keep_u8=True));
without it the saver decodes ``path_to_image`` with PIL and uploads it -- the slow pairing: the decode and a synchronous copy per frame on
the stepping thread.  A frame whose stream does not fit the capacity is encoded by the host code, with one warning per saver.

``vis_modes`` / ``soft_masks`` / ``alpha_matte`` (the outputs of the reference's interactive tool, gui/interactive_utils.py:79-229 and
gui/resource_manager.py:154-173): behind the id stage one launch per mode (PROB_TO_ID flags == 256, csrc/matte.hip)
composes the frame from the probability planes, the uint8 frame and the id plane -- the reference's float arithmetic, its bytes -- and
the JPEG stage above encodes the composed frame (no id plane); the soft masks (flags == 512) and the alpha matte are uint8 planes that
go through the PNG stage and leave as greyscale PNGs.  Files: ``<output_root>/<video>/visualization/<mode>/<frame>.jpg``,
``.../soft_masks/<object id>/<frame>.png``, ``.../alpha/<frame>.png``.  Status blocks and stream heads ride pinned copies in front of
one event per frame; the writer thread wraps and writes.  The full-size float planes never leave the device.

``tracks`` (not in the reference; DESIGN.md section 19, utils/track_report.py): one row per object and frame -- area, box, centroid,
confidence.  Behind the id stage of every path -- with egress='host' before the plane's ``.cpu()`` -- one op (PROB_TO_ID flags == 1024,
csrc/tracks.hip) reads the uint8 id plane the PNG is written from and, where the frame has them, the probabilities ``step`` returned (at
the model's resolution, in place); the table of 48 bytes per object rides a pinned copy with an event behind it, and the writer thread
hands it to the ``TrackReport``.  ``end`` writes ``tracks.json`` and ``tracks_mot.txt`` into ``<tracks_output_root>/<video>/``.
``process_merged`` has S probability sources and no single model resolution: it passes none, and the confidence is null there.

``min_region`` / ``fill_holes`` (not in the reference): the region filter (PROB_TO_ID flags == 2048, csrc/regions.hip)
rewrites the uint8 id plane on the device as soon as it exists and before anything reads it: object components below ``min_region`` pixels
become background, then enclosed background components below ``fill_holes`` pixels get the id left of their first pixel.  With
egress='host' it runs on the mask right behind the argmax; with egress='device' the id stage, the filter, the PNG stage and the RLE stage
are one op list (the PNG stage then runs on its own on the filtered plane instead of fused with the argmax); ``process_merged`` does the
same in both branches.  The PNG, the BURST RLE strings of either codec, the overlays, the id input of the vis modes, the track report and
the scorer therefore all see the plane of the file that is written.  What comes from the probabilities does NOT change: the soft masks, the
alpha matte, the soft vis modes and ``save_scores`` -- and the model never sees the filtered plane: the probabilities ``step`` returns, the
memory bank and ``last_mask`` are untouched.  The four counts of a frame ride a 16-byte pinned copy with an event behind it; the writer
thread sums them, and ``end`` leaves the video's totals in ``self.regions``.  With both thresholds below 2 nothing is launched and no
byte changes.

``trimap`` / ``trimap_objects`` / ``dilate_mask`` (not in the reference): what matting and inpainting models take
next to the frame.  Behind the id plane -- and behind the region filter, so on the plane of the file that is written -- one op list of
its own (PROB_TO_ID flags == 4096, csrc/edt.hip: the exact squared Euclidean distance of every pixel to the edge of a set of ids, and
the band byte that is a compare of it) writes one uint8 plane per output: the trimap of the union of the target objects (0 sure
background | 128 within r_out outside or r_in inside the edge | 255 sure foreground), with ``trimap_objects`` one trimap per object of
the frame, and the union dilated by the disk of radius ``dilate_mask`` (0 | 255).  Nothing exists outside the frame: an object cut by
the frame's border is not eroded from there.  The planes go through the PNG stage and leave as 8-bit grey PNGs, like the soft masks:
``<output_root>/<video>/trimap/<frame>.png``, ``.../trimap_objects/<object id>/<frame>.png``, ``.../dilated/<frame>.png``.  The stage
reads nothing but the plane, so it runs under both egress modes and in ``process_merged``.  Off: no launch, no file.

``redact`` (not in the reference): the footage itself, edited with what the tracker knows -- the target objects
blurred, pixelated or painted over in every frame, or with ``background`` everything but them.  Behind the id plane and the mattes one op
list of its own: the weight plane (``edge='mask'``: the union of the targets on the plane of the file that is written, grown by the disk
of ``grow`` pixels -- the ``dilate_mask`` call of the distance stage; ``edge='matte'``: the matte of the targets, the refined one under
``matte_refine``), the effect and the blend (PROB_TO_ID flags == 65536, csrc/redact.hip: integers only, the bytes of tests/redact_ref.py)
into an RGB buffer, and the JPEG stage of the vis modes on it.  ``<output_root>/<video>/redacted/<frame>.jpg``.  Off: no launch, no
buffer, no file."""
import logging
import os
import shutil
from dataclasses import dataclass
from os import path
from queue import Queue
from threading import Thread
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from ...utils.pano_utils import ID2RGBConverter
from . import coco_rle
from . import jpeg_writer
from . import png as png_container
from .polygons import trace_rings
from .saver_buffers import POLY_TABLE, RLE_TABLE, BandBuffers, EgressBuffers, KeyedCache, MatteBuffers, PolygonBuffers, Pool, RedactBuffers, RegionBuffers, Slab, TrackBuffers, WriterCopies

log = logging.getLogger()


def voc_palette(n: int = 256) -> np.ndarray:
    """The PASCAL-VOC / DAVIS colour map [n,3] (bit-interleaving construction)."""
    pal = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[i] = (r, g, b)
    return pal


davis_palette_np = voc_palette()
davis_palette = davis_palette_np.tobytes()


EGRESS_MODES = ('host', 'device')
REDACT_MODES = ('blur', 'pixelate', 'fill')
REDACT_EDGES = ('mask', 'matte')
REDACT_KEYS = ('mode', 'strength', 'color', 'grow', 'edge', 'background', 'targets')
REDACT_DEFAULT_STRENGTH = {'blur': 12, 'pixelate': 16, 'fill': 0}     # a radius, a cell size, unused


def redact_config(redact) -> dict:
    """ResultSaver's ``redact`` with every key present and every value judged: ValueError names what is wrong."""
    from ... import ops as O
    if not isinstance(redact, dict):
        raise ValueError(f'redact is None or a dict with the keys {REDACT_KEYS}, not {redact!r}')
    unknown = sorted(set(redact) - set(REDACT_KEYS))
    if unknown:
        raise ValueError(f'redact: unknown keys {unknown}; the keys are {REDACT_KEYS}')
    mode = redact.get('mode')
    if mode not in REDACT_MODES:
        raise ValueError(f'redact: mode is one of {REDACT_MODES}, not {mode!r}')
    strength = redact.get('strength')
    strength = REDACT_DEFAULT_STRENGTH[mode] if strength is None else strength
    if isinstance(strength, bool) or not isinstance(strength, (int, np.integer)):
        raise ValueError(f'redact: strength is an integer, not {strength!r}')
    strength = int(strength)
    if mode == 'blur' and not 1 <= strength <= O.OpList.REDACT_MAX_RADIUS:
        raise ValueError(f'redact: blur radius {strength}, 1 .. {O.OpList.REDACT_MAX_RADIUS}')
    if mode == 'pixelate' and not 2 <= strength <= O.OpList.REDACT_MAX_CELL:
        raise ValueError(f'redact: pixelate cell {strength}, 2 .. {O.OpList.REDACT_MAX_CELL}')
    color = redact.get('color', (0, 0, 0))
    try:
        rgb = tuple(int(v) for v in color)
        ok = len(rgb) == 3 and all(0 <= v <= 255 for v in rgb) and all(int(v) == v for v in color)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'redact: color is three bytes (R, G, B), not {color!r}')
    try:
        grow = float(redact.get('grow', 0.0))
    except (TypeError, ValueError):
        grow = float('nan')
    if not 0.0 <= grow <= 255.0:                                # (also refuses nan)
        raise ValueError(f"redact: grow of {redact.get('grow')!r} pixels, 0 .. 255")
    edge = redact.get('edge', 'mask')
    if edge not in REDACT_EDGES:
        raise ValueError(f'redact: edge is one of {REDACT_EDGES}, not {edge!r}')
    if edge == 'matte' and grow != 0.0:
        raise ValueError('redact: grow dilates the id mask; with edge=\'matte\' it must be 0')
    targets = redact.get('targets')
    if targets is not None:
        try:
            targets = [int(v) for v in targets]
        except (TypeError, ValueError):
            raise ValueError(f'redact: targets is None (all objects) or a list of object ids, not {targets!r}')
    return dict(mode=mode, strength=strength, color=rgb, grow=grow, edge=edge, background=bool(redact.get('background', False)), targets=targets)
PNG_CODES = ('fixed', 'dynamic')   # the encoder of the soft masks and the alpha matte: the id planes' (csrc/png.hip) | filters + dynamic Huffman (csrc/png_photo.hip)
EGRESS_SLAB = 64 * 1024     # bytes of the first device-to-host copy of a frame: the status block + the head of the stream (a 480p mask is 5.5-7.9 KB)
OVERLAY_MODES = ('host', 'device')
JPEG_SLAB = 256 * 1024      # overlay='device': bytes of the first device-to-host copy of a frame's JPEG: status + the head of the stream (a 480p overlay is 30-120 KB)
RLE_SLAB = 256 * 1024       # BURST: bytes of the whole device-to-host copy: status, table (RLE_TABLE) and the strings (a frame that needs more is encoded on the host)
# polygons: the stage's edge capacity and the bytes of its stream.  The worst case of a plane is 32 bytes per lattice vertex (13 MB at 480p)
# per buffer in flight; outlines of video objects are far from it: a boundary edge costs at most one vertex of 4 bytes and a ring of 16 bytes
# has at least 4 edges, so 4 bytes per edge hold every frame whose edges fit (a staircase: every edge a corner) unless it also has many
# rings.  65536 edges are 16 times the 4096 of the stage's one-workgroup path; the bike example's frames (speckled masks of random weights) have 300 .. 3450 edges and
# streams of 0.9 .. 8.5 KB, 5 % and 3 % of the bounds.  A frame beyond either bound is traced on the host (warned once).  POLY_HEAD: the pinned head
# copied every frame -- status, table and the first 12 KB of the stream; the writer thread fetches the rest of a longer one.
POLY_EDGES = 65536
POLY_STREAM = 4 * POLY_EDGES
POLY_HEAD = 16 + POLY_TABLE + 12 * 1024
VIS_MODES = ('davis', 'light', 'fade', 'popup', 'layer')     # gui/interactive_utils.py get_visualization_torch ('mask', 'image': trivial; 'rgba': alpha_matte)


@dataclass
class _Job:
    """One frame for the writer thread.  The buffer sets come from pools and go back to them (``held``); the tensors are kept alive until
    the writer is done with the frame, so that what a launch reads outlives the launch on the stream that owns it, whoever made it."""
    saver: 'ResultSaver'
    mask: Optional[torch.Tensor]  # CPU uint8 / int32 [H,W], object ids (None with egress='device': the mask arrives in `egress`)
    frame_name: str
    path_to_image: Optional[str]
    all_obj_ids: list
    prob: Optional[torch.Tensor] = None      # CPU uint8 [K+1,H,W] (save_scores)
    last_frame: bool = False
    tmp_to_obj: Optional[dict] = None        # {tmp_id: object id} at the time of the frame
    egress: Optional[EgressBuffers] = None   # egress='device': the mask's zlib stream arrives in these
    rle: bool = False                        # egress='device', BURST: the objects' RLE strings arrive in them as well
    overlay: Optional[EgressBuffers] = None  # overlay='device': the JPEG's entropy-coded segment arrives in these (the same set as `egress` when both are on)
    frame: Optional[torch.Tensor] = None     # overlay='device': the uint8 frame the stage read
    ids: Optional[torch.Tensor] = None       # overlay='device': the id plane on the device (a frame whose stream overflowed is blended on the host)
    matte: Optional[MatteBuffers] = None     # vis_modes / soft_masks / alpha_matte: the frame's composed outputs arrive in these
    matte_objects: Tuple = ()                # ... the object id of every soft-mask plane, in plane order
    matte_keep: Tuple = ()                   # ... what the launches read (planes, frame, tables)
    tracks: Optional[TrackBuffers] = None    # tracks: the frame's table arrives in these (None with track_meta: a frame without objects)
    track_meta: Optional[Tuple] = None       # ... (frame index, object ids of the rows, H, W): the frame is reported
    regions: Optional[RegionBuffers] = None  # min_region / fill_holes: the frame's four counts arrive in these
    polygons: Optional[PolygonBuffers] = None  # polygons: the frame's table, rings and vertices arrive in these (None with poly_meta: a frame without objects)
    poly_meta: Optional[Tuple] = None        # ... (frame index, object ids of the table's rows, H, W): the frame is reported
    bands: Optional[BandBuffers] = None      # trimap / trimap_objects / dilate_mask: the frame's band planes arrive in these
    redact: Optional[RedactBuffers] = None   # redact: the JPEG segment of the redacted frame arrives in these
    redact_keep: Tuple = ()                  # ... what the launches read (planes, frame, tables)
    band_planes: Tuple = ()                  # ... (folder, object id or None) of every plane, in plane order

    def held(self) -> list:
        """the pooled buffer sets of the frame, each once"""
        sets = []
        for b in (self.egress, self.overlay, self.matte, self.tracks, self.regions, self.bands, self.polygons, self.redact):
            if b is not None and not any(b is s for s in sets):
                sets.append(b)
        return sets


class ResultSaver:
    def __init__(self, output_root, video_name, *, dataset, object_manager, use_long_id, palette=None, save_mask=True,
                 save_scores=False, score_output_root=None, visualize_output_root=None, visualize=False, init_json=None,
                 processor=None, egress='host', scorer=None, overlay='host', vis_modes=(), soft_masks=False, alpha_matte=False,
                 target_objects=None, layer=None, tracks=None, tracks_output_root=None, min_region=0, fill_holes=0, region_connectivity=8,
                 trimap=None, trimap_objects=False, dilate_mask=0.0, polygons=None, polygons_output_root=None, cutout=False, png_codes='fixed',
                 matte_refine=None, redact=None):
        """``processor`` (optional, not in the reference): the InferenceCore whose fused PROB_TO_ID kernel does argmax+remap;
        without it a plain torch argmax + lookup is used (e.g. for probabilities that did not come from an InferenceCore).
        ``egress``: 'host' (default: the id plane is copied to the host and PIL encodes it) | 'device' (the GPU writes the PNG's zlib
        stream, see the module docstring; needs ``processor``).  A saver falls back to the host path -- ``self.egress`` says which one
        runs -- with ``use_long_id`` (RGB masks), with ``visualize`` (the host overlay needs the ids on the host; not with
        ``overlay='device'``) and without ``save_mask``;
        ``save_scores`` keeps its own copy of the probabilities next to the device-encoded mask: with it -- multi-scale runs -- ``process``
        still builds the full-size fp32 probabilities when the frame was resized and blocks on their copy, so 'device' saves only the
        PNG encode there, not the stall.
        ``scorer`` (not in the reference; utils/davis_metrics.py SequenceScorer): every frame's uint8 id plane is
        handed to ``scorer.add`` while it is still on the device -- before the copy of the host path, behind the id stage of the device
        path and of ``process_merged`` -- and ``end`` leaves ``scorer.finish()`` in ``self.scores``.  Long ids cannot be scored.
        ``overlay``: 'host' (default: the writer thread re-decodes the frame, blends in float and PIL encodes the JPEG) | 'device' (the
        GPU blends and writes the JPEG's entropy-coded segment, see the module docstring; needs ``processor``; the files are the same
        bytes).  It only matters with ``visualize``; ``use_long_id`` savers keep the host overlay -- ``self.overlay`` says which one runs.
        ``vis_modes`` (a subset of VIS_MODES), ``soft_masks``, ``alpha_matte`` (not in the reference's batch tools; its interactive
        tool writes them, see the module docstring): composed on the GPU per frame; they need ``processor`` and, for the modes, the
        frame (``image_u8`` or ``path_to_image`` of ``process``); a ``use_long_id`` saver refuses them.  ``target_objects``: the object
        ids that 'popup', 'layer' and the matte keep (default: all objects of the frame; ids that are not -- yet, or any more -- objects
        are left out).  ``layer``: the RGBA image of mode 'layer' (a PIL image, a uint8 [h, w, 4] array or a file name), resized once
        to the output size with PIL and uploaded once.
        ``tracks`` (not in the reference; a utils/track_report.py TrackReport, see the module docstring): every frame's area, box,
        coordinate sums and confidence per object are counted on the device and reported to it; ``end`` writes its two files into
        ``tracks_output_root``/<video>/ (default: <output_root>/tracks).  Needs ``processor``; long ids (RGB masks) have no uint8 plane.
        ``min_region``, ``fill_holes``, ``region_connectivity`` (not in the reference; see the module docstring): object components of
        fewer than ``min_region`` pixels are dropped from the id plane and enclosed background components of fewer than ``fill_holes``
        pixels are filled, on the device, before anything reads the plane; components are connected under ``region_connectivity`` (4 |
        8).  A threshold below 2 switches its stage off; with both off nothing changes anywhere.  ``end`` leaves the video's totals in
        ``self.regions`` (None when off).  Needs ``processor``; long ids (RGB masks) have no uint8 plane.
        ``trimap`` = (r_in, r_out), ``trimap_objects``, ``dilate_mask`` = r (not in the reference; see the module docstring): radii in
        pixels, floats, 0 <= r <= 255; (0, 0), None and 0.0 mean off.  The union outputs take the ids of ``target_objects`` (default:
        all objects of the frame; ids that are not objects of the frame are left out, and a frame without any gets all-zero files);
        ``trimap_objects`` adds one trimap per object of the frame and needs ``trimap``.  Exact Euclidean distances: a pixel is in the
        band iff dx^2 + dy^2 <= r^2 to the nearest pixel across the edge.  Needs ``processor``; long ids have no uint8 plane.
        ``polygons`` (not in the reference; a utils/polygons.py PolygonReport): every object's outline on every frame
        is traced on the device into exact rings of lattice corners (PROB_TO_ID flags == 8192), on the plane the PNG is written from --
        behind the region filter, connected under ``region_connectivity`` -- and reported to it; ``end`` writes
        ``polygons_output_root``/<video>/polygons.json (default root: <output_root>/polygons).  A frame beyond the stage's bounded
        capacities is traced on the host (one warning).  Needs ``processor``; long ids have no uint8 plane.
        ``cutout`` (the 'rgba' output of the reference's interactive tool, gui/interactive_utils.py:218-229): per
        saved frame <output_root>/<video>/cutout/<frame>.png, an RGBA PNG whose RGB is the frame (``image_u8`` or ``path_to_image`` of
        ``process``) and whose A is the alpha matte of ``target_objects`` -- the plane ``alpha_matte`` writes --, filtered and
        entropy-coded on the device (PROB_TO_ID flags == 16384).  A frame too wide for the stage's row limit is written through PIL
        (one warning).  Needs ``processor``; a ``use_long_id`` saver and ``process_merged`` refuse it.
        ``png_codes``: 'fixed' (default: the soft masks and the alpha matte go through the id planes' encoder, as before) | 'dynamic'
        (they are encoded by the filtered, dynamic-Huffman stage with one byte per pixel: the same pixels in fewer bytes).  The id
        masks, trimaps and dilated masks never change encoder.
        ``matte_refine``: None (default: no launch, the same bytes) | (r, eps) -- the matte plane (``alpha_matte``, the A channel of
        ``cutout``) and, with ``soft_masks``, the K object planes go through the colour guided filter (PROB_TO_ID flags == 32768; DESIGN.md
        section 25) with the uint8 frame as the guide before the PNG stages read them: radius r (1 .. 64 pixels of the output frame), eps
        (1e-6 .. 1) in units of the frame scaled to [0, 1].  The planes of a frame share one launch, up to 16 of them.  The 'popup' and
        'layer' JPEGs keep their bytes: they are composed from the float planes inside their own launch.  The id masks, trimaps and
        dilated masks are untouched.  Needs one of ``alpha_matte`` / ``cutout`` / ``soft_masks`` and the ``processor``; a ``use_long_id``
        saver and ``process_merged`` refuse it.
        ``redact``: None (default: no launch, no buffer, no file) | dict(mode='blur' | 'pixelate' | 'fill', strength=the blur radius 1 ..
        64 (default 12) or the pixelate cell 2 .. 256 (default 16), color=(R, G, B) of 'fill', grow=pixels 0 .. 255 the targets' mask is
        dilated by, edge='mask' (default: the id plane of the mask file, 0 | 255) | 'matte' (the soft matte of the targets, the refined
        one under ``matte_refine``; grow must be 0), background=False | True (everything BUT the targets takes the effect: background
        blur), targets=None (all objects) | object ids) -- per frame ``<video>/redacted/<frame>.jpg``, the frame with the effect
        blended over it under that weight plane (PROB_TO_ID flags == 65536), through the JPEG stage and tables of
        the vis modes.  Works under both egress modes; needs the ``processor`` and the frame (``image_u8`` or ``path_to_image``); a
        ``use_long_id`` saver refuses it, and ``process_merged`` refuses edge='matte' (it has no probability planes of its own)."""
        if redact is not None:
            redact = redact_config(redact)
            if use_long_id:
                raise ValueError('redact: the weight plane is made from uint8 id planes; a use_long_id saver (RGB masks) cannot write redacted frames')
            if processor is None:
                raise ValueError('redact needs the processor (its device)')
        self.redact = redact
        self._redact_mask = redact is not None and redact['edge'] == 'mask'
        if matte_refine is not None:
            from ... import ops as O
            try:
                r, eps = matte_refine
                ok = int(r) == r and not isinstance(r, bool)
                r, eps = int(r), float(eps)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f'matte_refine is None or (radius, eps), an int and a float, not {matte_refine!r}')
            if not 1 <= r <= O.OpList.GUIDED_MAX_RADIUS:
                raise ValueError(f'matte_refine: radius {r}, 1 .. {O.OpList.GUIDED_MAX_RADIUS}')
            if not O.OpList.GUIDED_EPS_MIN <= eps <= O.OpList.GUIDED_EPS_MAX:
                raise ValueError(f'matte_refine: eps {eps}, {O.OpList.GUIDED_EPS_MIN} .. {O.OpList.GUIDED_EPS_MAX}')
            if not (alpha_matte or cutout or soft_masks):
                raise ValueError('matte_refine refines the planes of alpha_matte, cutout and soft_masks: none of them is set')
            if use_long_id:
                raise ValueError('matte_refine: the matte outputs are composed from uint8 id planes; a use_long_id saver (RGB masks) cannot write them')
            if processor is None:
                raise ValueError('matte_refine needs the processor (its device)')
            matte_refine = (r, eps)
        self.matte_refine = matte_refine
        if png_codes not in PNG_CODES:
            raise ValueError(f'png_codes must be one of {PNG_CODES}, not {png_codes!r}')
        self.cutout, self.png_codes = bool(cutout), png_codes
        if polygons is not None and use_long_id:
            raise ValueError('polygons: outlines are traced on uint8 id planes; a use_long_id saver (RGB masks) cannot report them')
        if polygons is not None and processor is None:
            raise ValueError('polygons needs the processor (its device)')
        if polygons is not None and int(region_connectivity) not in (4, 8):
            raise ValueError(f'region_connectivity is 4 or 8, not {region_connectivity}')
        self.polygons = polygons
        self.polygons_output_root = polygons_output_root if polygons_output_root is not None else path.join(output_root, 'polygons')
        self._polygon_count = 0
        if polygons is not None:
            polygons.connectivity = int(region_connectivity)
            if not polygons.video:
                polygons.video = video_name
        def radius(name, r):
            r = float(r)
            if not 0.0 <= r <= 255.0:                          # (also refuses nan)
                raise ValueError(f'{name}: a radius of {r} pixels, 0 .. 255')
            return r
        if trimap is not None:
            if len(tuple(trimap)) != 2:
                raise ValueError(f'trimap is (r_in, r_out), not {trimap!r}')
            trimap = tuple(radius('trimap', r) for r in trimap)
            trimap = trimap if max(trimap) > 0.0 else None
        dilate_mask = radius('dilate_mask', dilate_mask)
        if trimap_objects and trimap is None:
            raise ValueError('trimap_objects: one trimap per object needs trimap=(r_in, r_out)')
        self.trimap, self.trimap_objects, self.dilate_mask = trimap, bool(trimap_objects), dilate_mask
        self._bands_on = trimap is not None or dilate_mask > 0.0
        if self._bands_on and use_long_id:
            raise ValueError('trimap / dilate_mask: distances are measured on uint8 id planes; a use_long_id saver (RGB masks) cannot write them')
        if self._bands_on and processor is None:
            raise ValueError('trimap / dilate_mask need the processor (its device)')
        self.min_region, self.fill_holes, self.region_connectivity = int(min_region), int(fill_holes), int(region_connectivity)
        if self.min_region < 0 or self.fill_holes < 0:
            raise ValueError(f'min_region and fill_holes are not negative ({min_region}, {fill_holes})')
        self._regions_on = self.min_region >= 2 or self.fill_holes >= 2
        if self._regions_on and self.region_connectivity not in (4, 8):
            raise ValueError(f'region_connectivity is 4 or 8, not {region_connectivity}')
        if self._regions_on and use_long_id:
            raise ValueError('min_region / fill_holes: components are labelled on uint8 id planes; a use_long_id saver (RGB masks) cannot filter them')
        if self._regions_on and processor is None:
            raise ValueError('min_region / fill_holes need the processor (its device)')
        self.regions = None
        self._region_totals, self._region_frames = np.zeros(4, dtype=np.int64), 0
        if tracks is not None and use_long_id:
            raise ValueError('tracks: the statistics are counted on uint8 id planes; a use_long_id saver (RGB masks) cannot report them')
        if tracks is not None and processor is None:
            raise ValueError('tracks needs the processor (its device and object table)')
        self.tracks = tracks
        self.tracks_output_root = tracks_output_root if tracks_output_root is not None else path.join(output_root, 'tracks')
        self._track_count = 0
        if tracks is not None and not tracks.video_name:
            tracks.video_name = video_name
        vis_modes = tuple(vis_modes)
        unknown = [m for m in vis_modes if m not in VIS_MODES]
        if unknown or len(set(vis_modes)) != len(vis_modes):
            raise ValueError(f'vis_modes is a subset of {VIS_MODES}, not {vis_modes}')
        self.vis_modes, self.soft_masks, self.alpha_matte = vis_modes, bool(soft_masks), bool(alpha_matte)
        self._matte_on = bool(vis_modes or soft_masks or alpha_matte or self.cutout)
        if self._matte_on and use_long_id:
            raise ValueError('vis_modes / soft_masks / alpha_matte / cutout are composed from uint8 id planes and object planes on the device: '
                             'a use_long_id saver (RGB masks) cannot write them')
        if self._matte_on and processor is None:
            raise ValueError('vis_modes / soft_masks / alpha_matte / cutout need the processor (its device)')
        if 'layer' in vis_modes and layer is None:
            raise ValueError("vis mode 'layer' needs layer (an RGBA image)")
        self.target_objects = None if target_objects is None else [int(v) for v in target_objects]
        self._layer_src = layer
        if scorer is not None and use_long_id:
            raise ValueError('scorer: J&F is counted on uint8 id planes; long ids (RGB masks) cannot be scored')
        self.scorer, self.scores = scorer, None
        if egress not in EGRESS_MODES:
            raise ValueError(f'egress must be one of {EGRESS_MODES}, not {egress!r}')
        if egress == 'device' and processor is None:
            raise ValueError("egress='device' needs the processor (its device and object table)")
        if overlay not in OVERLAY_MODES:
            raise ValueError(f'overlay must be one of {OVERLAY_MODES}, not {overlay!r}')
        if overlay == 'device' and processor is None:
            raise ValueError("overlay='device' needs the processor (its device)")
        if save_scores and score_output_root is None:
            raise ValueError('save_scores needs score_output_root')
        self.save_scores, self.score_output_root = save_scores, score_output_root
        if 'burst' in dataset.lower() and init_json is None:
            raise NotImplementedError('a BURST dataset needs init_json (the json of the sequence): the predictions are written into it')
        self.output_root, self.video_name, self.dataset = output_root, video_name, dataset.lower()
        self.json_style = None
        if 'burst' in self.dataset:              # results_utils.py:67-74
            self.input_segmentations = init_json['segmentations']
            self.segmentations = [{} for _ in init_json['segmentations']]
            self.annotated_frames = init_json['annotated_image_paths']
            self.video_json = {k: v for k, v in init_json.items() if k != 'segmentations'}
            self.video_json['segmentations'] = self.segmentations
            self.json_style = 'burst'
        self._rle_warned = self._jpeg_warned = self._polygons_warned = self._cutout_warned = False
        self.use_long_id, self.palette, self.object_manager = use_long_id, palette, object_manager
        self.save_mask, self.visualize, self.visualize_output_root = save_mask, visualize, visualize_output_root
        self.processor = processor
        self.overlay = 'device' if (overlay == 'device' and visualize and not use_long_id) else 'host'
        self.egress = 'device' if (egress == 'device' and not use_long_id and (not visualize or self.overlay == 'device') and save_mask) else 'host'
        self._jpeg_tables = None                 # (quantisation tables on the host, on the device)
        self._copies = WriterCopies()
        self._scratch = KeyedCache(latest=True)  # per stage the scratch tensor of the current geometry
        self._tables = KeyedCache(latest=False)  # per stage the small device tables of an object set (they change when objects come or go, not per frame)
        if self.visualize:
            self.colors = np.array(self.palette, dtype=np.uint8).reshape(-1, 3) if self.palette is not None else davis_palette_np
        self.need_remapping = True
        self.id2rgb_converter = ID2RGBConverter()
        self.queue: Queue = Queue(maxsize=10)
        # buffer sets in flight: what the queue can hold + the one in the writer's hands + the one being filled
        limit, dev = self.queue.maxsize + 2, lambda: self.processor.network.device
        self._pools = dict(
            egress=Pool(limit, lambda H, W, png: EgressBuffers(H, W, dev(), self._slab, rle=self.json_style == 'burst' and png, png=png,
                                                               jpeg=self.overlay == 'device')),
            matte=Pool(limit, lambda H, W, K: MatteBuffers(H, W, K, self.vis_modes, self.alpha_matte, dev(), self._slab, **self._matte_forms(W))),
            tracks=Pool(limit, lambda: TrackBuffers(dev())),
            regions=Pool(limit, lambda: RegionBuffers(dev())),
            polygons=Pool(limit, lambda H, W: PolygonBuffers(H, W, dev(), self._slab)),
            bands=Pool(limit, lambda H, W, S: BandBuffers(H, W, S, dev(), self._slab)),
            redact=Pool(limit, lambda H, W: RedactBuffers(H, W, dev(), self._slab, refine=self.matte_refine is not None)))
        self.thread = Thread(target=_writer, args=(self.queue,), daemon=True)
        self.thread.start()

    def _slab(self, kind, H, W) -> Slab:
        """A [status | stream] slab of this saver for a plane of H x W: 'png' (an error word raises in the writer thread), 'jpeg' and
        'rle' (a frame that did not fit its stream is warned about once per saver, and the writer thread takes its other route)."""
        from ... import ops as O
        dev = self.processor.network.device
        if kind == 'png':
            return Slab(O.OpList.png_capacity(H, W), EGRESS_SLAB, dev, self._copies)
        if kind == 'png dynamic':                # a grey plane through the filtered, dynamic-Huffman stage
            return Slab(O.OpList.png_photo_capacity(H, W, 1), EGRESS_SLAB, dev, self._copies)
        if kind == 'cutout':                     # RGBA; the pinned head holds half the raw size, a photograph takes about a third
            return Slab(O.OpList.png_photo_capacity(H, W, 4), 16 + 2 * H * W, dev, self._copies, what='cut-out PNG')
        if kind == 'polygons':
            def beyond(length, capacity):
                if not self._polygons_warned:
                    self._polygons_warned = True
                    log.warning(f'polygon trace: a frame of {self.video_name} is beyond the stage\'s capacities ({POLY_EDGES} boundary edges, a stream '
                                f'of {capacity} bytes; it needs {length} bytes); such frames are traced on the host')
            return Slab(min(POLY_STREAM, O.OpList.polygon_capacity(H, W)[0]), POLY_HEAD, dev, self._copies, what='polygon', error_word=1,
                        fixed=POLY_TABLE, overflow=beyond)
        flag = f'_{kind}_warned'

        def overflow(length, capacity):
            if not getattr(self, flag):
                setattr(self, flag, True)
                log.warning(f'device {kind.upper()} encoder: a frame of {self.video_name} needs {length} bytes, the stream holds {capacity}; '
                            f'such frames are encoded on the host')
        if kind == 'jpeg':
            return Slab(O.OpList.jpeg_enc_capacity(H, W), JPEG_SLAB, dev, self._copies, what='JPEG', overflow=overflow)
        return Slab(RLE_SLAB - RLE_TABLE, RLE_SLAB, dev, self._copies, what='RLE', error_word=1, fixed=RLE_TABLE - 16, overflow=overflow)

    # ---- the three id sources ---------------------------------------------------------------------------------------------------
    def process(self, prob: torch.Tensor, frame_name: str, resize_needed: bool = False, shape: Optional[Tuple[int, int]] = None,
                last_frame: bool = False, path_to_image: str = None, image_u8: Optional[torch.Tensor] = None, *, frame_index: Optional[int] = None):
        """``image_u8`` (overlay='device'): the frame as uint8 [H, W, 3] at the output size, on the device or on the host; without it
        ``path_to_image`` is decoded with PIL and uploaded (slow: see the module docstring).
        ``frame_index`` (tracks): the frame's 1-based position in the video; without it the running count of reported frames."""
        rest = dict(last_frame=last_frame, path_to_image=path_to_image, image_u8=image_u8, frame_index=frame_index)
        if self.egress == 'device':              # one probability tensor, resampled inside the id stage: the full-size planes never exist
            dev = self.processor.network.device
            P, h, w = prob.shape
            out_hw = (int(shape[0]), int(shape[1])) if resize_needed else (h, w)
            lut_dev = self._lut_device(P, dev, uint8=True)
            prob = self._planes_f32(prob, dev)

            def id_stage(ol, ids, png):
                ol.prob_to_id(prob, lut_dev, ids, P=P, H=h, W=w, plane=prob.stride(0), ldrow=prob.stride(1),
                              out_hw=out_hw if resize_needed else None, png=png)

            def full_size():                     # (save_scores, as the host path: the scores of the output size)
                return F.interpolate(prob.unsqueeze(1), shape, mode='bilinear', align_corners=False)[:, 0] if resize_needed else prob
            return self._frame(frame_name, out_hw, id_stage, planes=prob, confidence=prob, scores=full_size, **rest)
        model_prob = prob                        # (tracks: the confidence is taken at the model's resolution)
        if resize_needed:
            prob = F.interpolate(prob.unsqueeze(1), shape, mode='bilinear', align_corners=False)[:, 0]
        out_dtype = torch.int32 if self.use_long_id else torch.uint8
        if self.processor is not None:
            mask = self.processor.output_prob_to_mask(prob, dtype=out_dtype)          # argmax + remap, one kernel
        else:
            idx = torch.argmax(prob, dim=0)
            lut = torch.zeros(prob.shape[0], dtype=torch.long, device=idx.device)
            for tmp_id, obj in self.object_manager.tmp_id_to_obj.items():
                if tmp_id < lut.shape[0]:
                    lut[tmp_id] = obj.id
            mask = lut[idx].to(out_dtype)
        return self._frame(frame_name, tuple(prob.shape[1:]), None, mask=mask, planes=prob, confidence=model_prob, scores=lambda: prob, **rest)

    # ---- multi-scale merge on the device -------------------------------------------------------------------------------------------
    def process_merged(self, probs, frame_name: str, shape: Tuple[int, int], last_frame: bool = False, path_to_image: str = None, *,
                       id_maps=None, image_u8: Optional[torch.Tensor] = None, frame_index: Optional[int] = None):
        """One frame of a multi-scale run (not in the reference, whose protocol is one run per size with ``save_scores`` and
        scripts/merge_multi_scale.py afterwards): ``probs`` = the members' [K+1, h_s, w_s] probabilities of the frame,
        every one resampled to ``shape``, quantised to uint8 and summed as the file route does, argmax + remap -- ONE kernel (PROB_TO_ID
        flags&16) that reads the members' views in place; no full-size plane and no score file exists.  egress='host': the id plane
        (uint8, int32 with long ids) is copied to the host and the writer thread does the rest (visualize, long ids); egress='device':
        the same op carries the PNG stage, as in ``process``.  ``id_maps``: the members' {tmp id: object id} tables -- they must be
        equal (the members see the same first masks in the same order); this saver's object manager is the first member's.
        ``tracks``: area, box and centroid of the merged plane are reported; the merge has S probability sources and no single model
        resolution, so no probabilities are passed and the confidence is null.  ``frame_index``: as in ``process``."""
        from ... import ops as O
        if self.json_style == 'burst':
            raise ValueError('process_merged: BURST has no multi-scale protocol (no json is written from merged scales)')
        if self.save_scores:
            raise ValueError('process_merged writes no scores: save_scores and the merge exclude each other')
        if self._matte_on:
            raise ValueError('process_merged has no probability planes of its own: vis_modes / soft_masks / alpha_matte / cutout need process')
        if self.redact is not None and self.redact['edge'] == 'matte':
            raise ValueError("process_merged has no probability planes of its own: redact with edge='matte' needs process")
        if self.processor is None:
            raise ValueError('process_merged needs the processor (its device; the merge has no host implementation)')
        own = {int(t): int(o.id) for t, o in self.object_manager.tmp_id_to_obj.items()}
        for m in (id_maps or ()):
            if {int(t): int(o) for t, o in m.items()} != own:
                raise ValueError(f'process_merged: the members disagree on tmp id -> object id ({m} against {own})')
        probs = list(probs)
        if not 1 <= len(probs) <= O.OpList.MERGE_MAX_SOURCES:
            raise ValueError(f'process_merged: {len(probs)} members, 1 .. {O.OpList.MERGE_MAX_SOURCES}')
        dev = self.processor.network.device
        P = int(probs[0].shape[0])
        if any(int(p.shape[0]) != P for p in probs):
            raise ValueError('process_merged: the members disagree on the number of planes')
        out_hw = (int(shape[0]), int(shape[1]))
        lut_dev = self._lut_device(P, dev, uint8=self.egress == 'device' or not self.use_long_id)
        probs = [self._planes_f32(p, dev) for p in probs]

        def id_stage(ol, ids, png):              # S merged sources
            ol.prob_to_id_merged(probs, lut_dev, ids, out_hw=out_hw, png=png)
        return self._frame(frame_name, out_hw, id_stage, last_frame=last_frame, path_to_image=path_to_image, image_u8=image_u8, frame_index=frame_index)

    # ---- the frame path -----------------------------------------------------------------------------------------------------------
    def _frame(self, frame_name, out_hw, id_stage, *, mask=None, planes=None, confidence=None, scores=None, last_frame=False,
               path_to_image=None, image_u8=None, frame_index=None):
        """One frame, whatever its id source.  ``id_stage(ol, ids, png)`` appends the stage that writes the id plane ``ids`` to the op
        list -- fused with the PNG stage when ``png`` = (stream, status, scratch) is given --; None: ``mask`` is the finished plane (the
        host path's torch argmax / ``output_prob_to_mask``) and nothing is appended.  ``planes``: the probabilities the vis modes and
        soft masks sample at ``out_hw``; ``confidence``: those the track report reads, at the model's resolution (None: a merge);
        ``scores()``: those ``save_scores`` keeps, at the output size.  Nothing waits here but the host path's copy of the plane (and
        of the scores).
        1. ONE op list: the id stage, the region filter -- before anything reads the plane --, with egress='device' the PNG stage
           (fused with the id stage when no filter stands between them) and, on an annotated BURST frame, the RLE stage;
        2. the scorer sees the plane on the device (a pooled plane is not handed out again before the writer is done with the frame);
        3. the overlay, the copy of the filter's counts, the vis modes / soft masks / matte, the track report and the trimaps /
           dilated mask, each an op list of
           its own behind the plane, each followed by its pinned copies;
        4. the frame's own pinned copies with the event behind every copy, and the job -- which keeps alive what the launches read
           until the writer has released the frame."""
        from ... import ops as O
        H, W = out_hw
        on_device = self.egress == 'device'
        all_ids = [o.id for o in self.object_manager.obj_to_tmp_id]
        ol, b, png = O.OpList(), None, None
        if on_device:
            dev = self.processor.network.device
            b = self._pools['egress'].take(H, W, True)
            ids = b.ids
            png = (b.png.stream, b.png.status,
                   self._scratch.get('png', (H, W), lambda: torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device=dev)))
        elif id_stage is not None:
            ids = torch.empty((H, W), dtype=torch.int32 if self.use_long_id else torch.uint8, device=self.processor.network.device)
        else:
            ids = mask.contiguous() if self._regions_on or self._bands_on or self.polygons is not None or self._redact_mask else mask
        fused = None if self._regions_on else png
        if id_stage is not None:
            id_stage(ol, ids, fused)
        rb = self._add_regions(ol, ids) if self._regions_on else None
        if png is not None and fused is None:    # the PNG stage on its own, on the filtered plane
            ol.png_deflate(ids, *png, H=H, W=W)
        rle = on_device and self.json_style == 'burst' and frame_name in self.annotated_frames
        if rle:                                  # the objects' RLE strings of the finished plane, in the order of all_ids
            n = len(all_ids)
            objs = self._tables.get('rle', tuple(all_ids), lambda: torch.tensor(all_ids or [0], dtype=torch.int32).to(dev))
            scratch = self._scratch.get('rle', (H, W, n), lambda: torch.empty(O.OpList.rle_scratch_words(H, W, n), dtype=torch.int32, device=dev))
            ol.rle_encode(ids, objs, b.rle.stream, b.rle_table, b.rle.status, scratch, H=H, W=W, n_objects=n)
        if len(ol):
            ol.run()
        if self.scorer is not None:
            self.scorer.add(frame_name, ids)
        fields = self._queue_overlay(b, ids, all_ids, path_to_image, image_u8) if self.overlay == 'device' else {}
        job_image = path_to_image if (fields or not on_device) else None    # (the writer reads the file again only for a host overlay)
        if rb is not None:                      # the pinned copy of the frame's counts (16 bytes) and the event behind it
            rb.host.copy_(rb.dev, non_blocking=True)
            rb.event.record()
            fields['regions'] = rb
        if self._matte_on:
            fields.update(self._queue_matte(planes, out_hw, ids, all_ids, path_to_image, image_u8))
        if self.tracks is not None:
            fields.update(self._queue_tracks(ids, all_ids, confidence, None, frame_index))
        if self._bands_on:
            fields.update(self._queue_bands(ids, all_ids))
        if self.polygons is not None:
            fields.update(self._queue_polygons(ids, all_ids, frame_index))
        if self.redact is not None:              # (behind the mattes: edge='matte' reads the plane they wrote)
            fields.update(self._queue_redact(planes, out_hw, ids, all_ids, path_to_image, image_u8, fields.get('matte')))
        if on_device:
            b.png.copy()
            if rle:
                b.rle.copy()
            b.event.record()
        q = (scores() * 255).to(torch.uint8).cpu() if self.save_scores else None   # == numpy astype(uint8) of prob*255
        self.queue.put(_Job(self, None if on_device else ids.cpu(), frame_name, job_image, all_ids, prob=q, last_frame=last_frame,
                            tmp_to_obj={t: o.id for t, o in self.object_manager.tmp_id_to_obj.items()} if last_frame else None,
                            egress=b, rle=rle, **fields))

    def _lut_device(self, P, dev, uint8=False):
        """plane -> object id as int32 [P] on the device (PROB_TO_ID's lut).  ``uint8``: the ids go into a uint8 plane."""
        lut = [0] * P
        for tmp_id, obj in self.object_manager.tmp_id_to_obj.items():
            if tmp_id < P:
                lut[tmp_id] = int(obj.id)
        if uint8 and max(lut) > 255:
            raise ValueError('object ids above 255 need use_long_id')
        return self._tables.get('lut', tuple(lut), lambda: torch.tensor(lut, dtype=torch.int32).to(dev))

    @staticmethod
    def _planes_f32(prob, dev):
        """probabilities as the launches read them: f32, on the device, last dimension contiguous (the view ``step`` returns is)"""
        if prob.dtype != torch.float32 or prob.device != dev or prob.stride(2) != 1:
            prob = prob.to(device=dev, dtype=torch.float32).contiguous()
        return prob

    # ---- min_region / fill_holes -------------------------------------------------------------------------------------------------
    def _add_regions(self, ol, ids) -> RegionBuffers:
        """Append the region filter of ``ids`` (uint8 [H, W] on the device, contiguous; rewritten in place) to the op list ``ol``.
        -> the frame's count buffers, copied once the list has been run."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(ids.shape[0]), int(ids.shape[1])
        scratch = self._scratch.get('regions', (H, W), lambda: torch.empty(O.OpList.region_scratch_words(H, W), dtype=torch.int32, device=dev))
        b = self._pools['regions'].take()
        ol.region_filter(ids, scratch, b.dev, min_region=self.min_region, fill_holes=self.fill_holes, connectivity=self.region_connectivity)
        return b

    # ---- trimap / trimap_objects / dilate_mask ------------------------------------------------------------------------------------
    def _queue_bands(self, ids, all_ids) -> dict:
        """Queue the distance stage of one frame on the current stream, behind the stage that wrote ``ids`` (uint8 [H, W] on the device)
        and behind the region filter: one op per threshold pair (the trimaps: the union first, then one set per object, split over ops
        of at most EDT_MAX_SETS sets; the dilated union), the PNG stage per plane, the pinned copies and one event.  -> the _Job fields.
        Nothing waits here."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(ids.shape[0]), int(ids.shape[1])
        union = tuple(all_ids) if self.target_objects is None else tuple(o for o in self.target_objects if o in all_ids)
        groups, planes = [], []                  # the trimaps' sets of ids; (folder, object id) of every plane
        if self.trimap is not None:
            objects = list(all_ids) if self.trimap_objects else []
            groups = [union] + [(o,) for o in objects]
            planes = [('trimap', None)] + [('trimap_objects', o) for o in objects]
        n = len(groups)
        if self.dilate_mask > 0.0:
            planes.append(('dilated', None))

        def table():
            t = np.zeros((max(n, 1), 256), dtype=np.uint8)
            for s, group in enumerate(groups or [union]):
                t[s, list(group)] = 1
            return torch.from_numpy(t).to(dev)
        sets = self._tables.get('bands', (union, tuple(all_ids) if n > 1 else None), table)
        b = self._pools['bands'].take(H, W, len(planes))
        most = min(max(n, 1), O.OpList.EDT_MAX_SETS)
        scratch = self._scratch.get('bands', (H, W, most), lambda: torch.empty(O.OpList.edt_scratch_words(most, H, W), dtype=torch.int32, device=dev))
        ol = O.OpList()
        if n:
            inner, outer = (int(r * r) for r in self.trimap)   # floor(r^2): dx^2 + dy^2 is an integer
            for a in range(0, n, most):
                ol.edt_band(ids, sets[a:a + most], scratch, band=b.band[a:min(a + most, n)], inner=inner, outer=outer, mid=128)
        if self.dilate_mask > 0.0:
            ol.edt_band(ids, sets[:1], scratch, band=b.band[n:n + 1], inner=0, outer=int(self.dilate_mask * self.dilate_mask), mid=255)
        png_scratch = self._scratch.get('bands png', (H, W), lambda: torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device=dev))
        for k, slab in enumerate(b.png):
            ol.png_deflate(b.band[k], slab.stream, slab.status, png_scratch, H=H, W=W)
        ol.run()
        for slab in b.png:
            slab.copy()
        b.event.record()
        return dict(bands=b, band_planes=tuple(planes))

    # ---- tracks -----------------------------------------------------------------------------------------------------------------
    def _queue_tracks(self, ids, all_ids, prob, lut_dev, frame_index) -> dict:
        """Queue the track statistics of one frame on the current stream, behind the stage that wrote ``ids`` (uint8 [H, W] on the
        device), the pinned copy of the table (48 bytes per object) and an event.  ``prob``: f32 [P, h, w] as ``step`` returned it, or
        None (no confidence); ``lut_dev``: its lut on the device, or None: ``_lut_device``'s.  -> the _Job fields.  Nothing waits here."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(ids.shape[0]), int(ids.shape[1])
        self._track_count += 1
        meta = (self._track_count if frame_index is None else int(frame_index), list(all_ids), H, W)
        n = len(all_ids)
        if n == 0:                               # a frame without objects is reported with no rows: nothing to launch
            return dict(track_meta=meta)
        if n > O.OpList.TRACK_MAX_OBJECTS:
            raise ValueError(f'tracks: {n} objects, at most {O.OpList.TRACK_MAX_OBJECTS} per frame')
        objs = self._tables.get('tracks', tuple(all_ids), lambda: torch.tensor(list(all_ids), dtype=torch.int32).to(dev))
        if prob is not None:
            prob = self._planes_f32(prob, dev)
            lut_dev = lut_dev if lut_dev is not None else self._lut_device(int(prob.shape[0]), dev)
        b = self._pools['tracks'].take()
        words = n * O.OpList.TRACK_WORDS
        ol = O.OpList()
        ol.track_stats(ids, objs, b.dev[:words], prob=prob, lut=lut_dev if prob is not None else None)
        ol.run()
        b.host[:words].copy_(b.dev[:words], non_blocking=True)
        b.event.record()
        return dict(tracks=b, track_meta=meta)

    # ---- polygons ---------------------------------------------------------------------------------------------------------------
    def _queue_polygons(self, ids, all_ids, frame_index) -> dict:
        """Queue the polygon trace of one frame on the current stream, behind the stage that wrote ``ids`` (uint8 [H, W] on the device)
        and behind the region filter, the pinned copy of the slab's head and an event.  -> the _Job fields.  Nothing waits here."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(ids.shape[0]), int(ids.shape[1])
        self._polygon_count += 1
        meta = (self._polygon_count if frame_index is None else int(frame_index), list(all_ids), H, W)
        n = len(all_ids)
        if n == 0:                               # a frame without objects is reported with no entries: nothing to launch
            return dict(poly_meta=meta)
        if n > O.OpList.POLY_MAX_OBJECTS:
            raise ValueError(f'polygons: {n} objects, at most {O.OpList.POLY_MAX_OBJECTS} per frame')
        objs = self._tables.get('polygons', tuple(all_ids), lambda: torch.tensor(list(all_ids), dtype=torch.int32).to(dev))
        edges = min(POLY_EDGES, O.OpList.polygon_capacity(H, W)[1])
        scratch = self._scratch.get('polygons', (H, W), lambda: torch.empty(O.OpList.polygon_scratch_words(H, W, n, edges), dtype=torch.int32, device=dev))
        b = self._pools['polygons'].take(H, W)
        ol = O.OpList()
        ol.polygon_trace(ids, objs, b.slab.stream, b.table[:4 * n], b.slab.status, scratch, connectivity=self.region_connectivity, edge_capacity=edges)
        ol.run()
        b.slab.copy()
        b.event.record()
        return dict(polygons=b, poly_meta=meta)

    # ---- overlay='device' -------------------------------------------------------------------------------------------------------
    def _queue_overlay(self, b, ids, all_ids, path_to_image, image_u8) -> dict:
        """Queue the blend + JPEG stage of one frame on the current stream, behind the stage that wrote ``ids`` (uint8 [H, W] on the
        device), and the pinned copy of its status and stream head.  ``b``: the frame's buffers (egress='device'; its event is recorded
        by the caller behind everything) or None: a set of its own is taken and its event recorded here.  -> the _Job fields.
        The frame tensor: the op list holds it while the stage is being queued, and the job holds it (and the id plane) until the
        writer thread is done with the frame -- so it outlives the launch that reads it on the stream that owns it, whoever made it."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(ids.shape[0]), int(ids.shape[1])
        image_u8 = self._frame_u8(H, W, dev, path_to_image, image_u8)
        qtables, scratch = self._jpeg_setup(H, W, dev)
        colors = self._tables.get('overlay colors', tuple(all_ids), lambda: torch.from_numpy(jpeg_writer.color_table(self.colors, all_ids)).to(dev))
        own = b is None
        if own:
            b = self._pools['egress'].take(H, W, False)
        ol = O.OpList()
        ol.jpeg_encode(image_u8, ids, colors, qtables, b.jpeg.stream, b.jpeg.status, scratch, H=H, W=W)
        ol.run()
        b.jpeg.copy()
        if own:
            b.event.record()
        return dict(overlay=b, frame=image_u8, ids=ids)

    # ---- vis_modes / soft_masks / alpha_matte -------------------------------------------------------------------------------------
    def _frame_u8(self, H, W, dev, path_to_image, image_u8):
        """The frame as packed uint8 [H, W, 3] on the device (overlay='device' and the vis modes read it)."""
        if image_u8 is None:
            if path_to_image is None:
                raise ValueError('Cannot visualize without path_to_image or image_u8')
            image_u8 = torch.from_numpy(np.array(Image.open(path_to_image).convert('RGB')))
        if image_u8.dtype != torch.uint8 or tuple(image_u8.shape) != (H, W, 3):
            raise ValueError(f'image_u8 is uint8 [{H}, {W}, 3] (the output size), not {image_u8.dtype} {tuple(image_u8.shape)}')
        if image_u8.device != dev or image_u8.stride(2) != 1 or image_u8.stride(1) != 3:
            image_u8 = image_u8.to(dev).contiguous()
        return image_u8

    def _jpeg_setup(self, H, W, dev):
        """-> the quantisation tables on the device (made once) and the JPEG stage's scratch for this geometry"""
        from ... import ops as O
        if self._jpeg_tables is None:
            qt = jpeg_writer.quant_tables(jpeg_writer.QUALITY)
            self._jpeg_tables = (qt, torch.from_numpy(qt.view(np.int16)).to(dev))
        return self._jpeg_tables[1], self._scratch.get('jpeg', (H, W), lambda: torch.empty(O.OpList.jpeg_enc_scratch_words(H, W), dtype=torch.int32, device=dev))

    def _layer(self, H, W, dev):
        """The RGBA layer at the output size on the device: resized with PIL and uploaded once per geometry."""
        def make():
            src = self._layer_src
            if isinstance(src, (str, os.PathLike)):
                src = Image.open(src)
            if not isinstance(src, Image.Image):
                src = Image.fromarray(np.asarray(src, dtype=np.uint8))
            return torch.from_numpy(np.ascontiguousarray(np.array(src.convert('RGBA').resize((W, H))))).to(dev)
        return self._scratch.get('layer', (H, W), make)

    def _matte_colors(self, all_ids, dev):
        """the reference's colour map of the hard vis modes: the palette scaled by 1.5 (gui/interactive_utils.py:42-44)"""
        def make():
            pal = np.array(self.palette, dtype=np.uint8).reshape(-1, 3) if self.palette is not None else davis_palette_np
            pal = (pal.astype(np.float32) * 1.5).clip(0, 255).astype(np.uint8)
            return torch.from_numpy(jpeg_writer.color_table(pal, all_ids)).to(dev)
        return self._tables.get('matte colors', tuple(all_ids), make)

    def _matte_forms(self, W) -> dict:
        """Which encoders a matte buffer set of width W is made for: ``cutout`` None | 'device' | 'host' (a row beyond the stage's
        limit: PIL, one warning), ``dynamic``: the grey planes through the filtered stage."""
        from ... import ops as O
        cutout = None
        if self.cutout:
            cutout = 'device' if O.OpList.png_photo_fits(W, 4) else 'host'
            if cutout == 'host' and not self._cutout_warned:
                self._cutout_warned = True
                log.warning(f'cut-outs: a row of {W} RGBA pixels is beyond the device PNG stage\'s limit of {O.OpList.PNG_PHOTO_ROW_LIMIT} bytes; '
                            f'the cut-outs of {self.video_name} are written through PIL')
        forms = dict(cutout=cutout, dynamic=self.png_codes == 'dynamic' and O.OpList.png_photo_fits(W, 1))
        if self.matte_refine is not None:            # (a saver without it builds its buffers with the arguments it always did)
            forms['refine'] = True
        return forms

    def _queue_matte(self, prob, out_hw, ids, all_ids, path_to_image, image_u8) -> dict:
        """Queue the composite launches of one frame on the current stream, behind the stage that wrote ``ids`` (uint8 [H, W] on the
        device), each followed by the JPEG stage on the composed frame, the soft-mask launch and the PNG stage per plane, the pinned
        copies of every status block and stream head, and one event.  ``prob``: f32 [P, h, w] as ``step`` returned it, sampled at
        ``out_hw`` inside the launches.  -> the _Job fields.  Nothing waits here."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(out_hw[0]), int(out_hw[1])
        P = int(prob.shape[0])
        prob = self._planes_f32(prob, dev)
        tmp_to_obj = {int(t): int(o.id) for t, o in self.object_manager.tmp_id_to_obj.items() if int(t) < P}
        K = P - 1 if self.soft_masks else 0
        b = self._pools['matte'].take(H, W, K)
        wanted = all_ids if self.target_objects is None else self.target_objects
        obj_to_tmp = {o: t for t, o in tmp_to_obj.items()}
        targets = [obj_to_tmp[o] for o in wanted if o in obj_to_tmp]
        ol = O.OpList()
        need_matte = self.alpha_matte or self.cutout                 # the cut-out's fourth channel is the plane alpha_matte writes
        frame = self._frame_u8(H, W, dev, path_to_image, image_u8) if (self.vis_modes or self.cutout or self.matte_refine is not None) else None
        if self.vis_modes:
            qtables, scratch = self._jpeg_setup(H, W, dev)
            colors = self._matte_colors(all_ids, dev) if any(m in ('davis', 'light', 'fade') for m in self.vis_modes) else None
            for k, mode in enumerate(self.vis_modes):
                soft = mode in ('popup', 'layer')
                with_matte = need_matte and soft and not any(m in ('popup', 'layer') for m in self.vis_modes[:k])
                ol.matte_composite(mode, b.frames[k], out_hw=(H, W), frame=frame, planes=prob if soft else None, targets=targets,
                                   ids=None if soft else ids, colors=None if soft else colors,
                                   layer=self._layer(H, W, dev) if mode == 'layer' else None, matte=b.matte if with_matte else None)
                ol.jpeg_encode(b.frames[k], None, None, qtables, b.jpeg[k].stream, b.jpeg[k].status, scratch, H=H, W=W)
        if need_matte and not any(m in ('popup', 'layer') for m in self.vis_modes):
            ol.matte_composite('alpha', None, out_hw=(H, W), planes=prob, targets=targets, matte=b.matte)
        if K > 0:
            ol.matte_soft(prob, b.planes[:K], out_hw=(H, W))
        if b.refined is not None:                # the guided filter under the frame: K planes and the matte in one launch, 16 at a time
            r, eps = self.matte_refine
            n, cap = int(b.refined.shape[0]), O.OpList.GUIDED_MAX_PLANES
            scratch = self._scratch.get('matte refine', (H, W, min(n, cap)),
                                        lambda: torch.empty(O.OpList.guided_scratch_words(min(n, cap), H, W), dtype=torch.int32, device=dev))
            for s0 in range(0, n, cap):
                s1 = min(s0 + cap, n)
                k1 = min(s1, K)
                ol.guided_filter(frame, b.planes[s0:k1] if k1 > s0 else None, b.refined[s0:s1], scratch, radius=r, eps=eps,
                                 last=b.matte if s1 > K else None)
        if b.dynamic:
            scratch = self._scratch.get('matte png dynamic', (H, W), lambda: torch.empty(O.OpList.png_photo_scratch_words(H, W, 1), dtype=torch.int32, device=dev))
            for k, slab in enumerate(b.png):
                ol.png_photo(b.final_plane(k), slab.stream, slab.status, scratch)
        else:
            scratch = self._scratch.get('matte png', (H, W), lambda: torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device=dev))
            for k, slab in enumerate(b.png):
                ol.png_deflate(b.final_plane(k), slab.stream, slab.status, scratch, H=H, W=W)
        if b.cutout is not None:                 # frame + matte -> RGBA, interleaved inside the stage: no RGBA buffer exists
            scratch = self._scratch.get('cutout', (H, W), lambda: torch.empty(O.OpList.png_photo_scratch_words(H, W, 4), dtype=torch.int32, device=dev))
            ol.png_photo(frame, b.cutout.stream, b.cutout.status, scratch, last=b.final_plane(K))
        ol.run()
        for slab in b.jpeg + b.png + ([b.cutout] if b.cutout is not None else []):
            slab.copy()
        b.event.record()
        return dict(matte=b, matte_objects=tuple(tmp_to_obj.get(q) for q in range(1, K + 1)), matte_keep=(prob, ol.keep, frame))

    # ---- redact ---------------------------------------------------------------------------------------------------------------------
    def _queue_redact(self, prob, out_hw, ids, all_ids, path_to_image, image_u8, matte) -> dict:
        """Queue the redacted frame of one frame on the current stream, behind the stage that wrote ``ids`` (uint8 [H, W] on the device),
        behind the region filter and behind the mattes (``matte``: the frame's MatteBuffers or None): the weight plane, the effect and
        the blend, the JPEG stage, the pinned copy of its status and stream head, and one event.  -> the _Job fields.  Nothing waits."""
        from ... import ops as O
        dev = self.processor.network.device
        H, W = int(out_hw[0]), int(out_hw[1])
        rc = self.redact
        frame = self._frame_u8(H, W, dev, path_to_image, image_u8)
        b = self._pools['redact'].take(H, W)
        ol = O.OpList()
        if rc['edge'] == 'mask':                 # the dilate_mask call: the union of the targets, grown by the disk of `grow` pixels, 0 | 255
            union = tuple(all_ids) if rc['targets'] is None else tuple(o for o in rc['targets'] if o in all_ids)

            def table():
                t = np.zeros((1, 256), dtype=np.uint8)
                t[0, list(union)] = 1
                return torch.from_numpy(t).to(dev)
            sets = self._tables.get('redact', union, table)
            scratch = self._scratch.get('redact band', (H, W), lambda: torch.empty(O.OpList.edt_scratch_words(1, H, W), dtype=torch.int32, device=dev))
            ol.edt_band(ids, sets, scratch, band=b.weight, inner=0, outer=int(rc['grow'] * rc['grow']), mid=255)
            weight = b.weight[0]
        elif matte is not None and matte.matte is not None and rc['targets'] == self.target_objects:
            weight = matte.final_plane(matte.K)  # the plane alpha_matte / cutout write, made by the launches queued before this list
        else:                                    # no output of the frame holds the targets' matte: it is composed (and refined) here
            if prob is None:
                raise ValueError("redact with edge='matte' needs the probability planes")
            prob = self._planes_f32(prob, dev)
            obj_to_tmp = {int(o.id): int(t) for t, o in self.object_manager.tmp_id_to_obj.items() if int(t) < int(prob.shape[0])}
            wanted = all_ids if rc['targets'] is None else rc['targets']
            ol.matte_composite('alpha', None, out_hw=(H, W), planes=prob, targets=[obj_to_tmp[o] for o in wanted if o in obj_to_tmp], matte=b.weight[0])
            weight = b.weight[0]
            if b.refined is not None:
                r, eps = self.matte_refine
                scratch = self._scratch.get('redact refine', (H, W), lambda: torch.empty(O.OpList.guided_scratch_words(1, H, W), dtype=torch.int32, device=dev))
                ol.guided_filter(frame, None, b.refined, scratch, radius=r, eps=eps, last=weight)
                weight = b.refined[0]
        key = (H, W, rc['mode'], rc['strength'])
        scratch = self._scratch.get('redact', key, lambda: torch.empty(O.OpList.redact_scratch_words(rc['mode'], H, W, rc['strength']), dtype=torch.int32, device=dev))
        ol.redact(frame, weight, b.out, scratch, mode=rc['mode'], strength=rc['strength'], color=rc['color'], invert=rc['background'])
        qtables, scratch = self._jpeg_setup(H, W, dev)
        ol.jpeg_encode(b.out, None, None, qtables, b.jpeg.stream, b.jpeg.status, scratch, H=H, W=W)
        ol.run()
        b.jpeg.copy()
        b.event.record()
        return dict(redact=b, redact_keep=(prob, ol.keep, frame, ids))

    def end(self):
        self.queue.put(None)
        self.queue.join()
        self.thread.join()
        for pool in self._pools.values():
            pool.reset()
        self._scratch.clear()
        if self._regions_on:
            t = [int(v) for v in self._region_totals]
            self.regions = dict(min_region=self.min_region, fill_holes=self.fill_holes, connectivity=self.region_connectivity,
                                frames=self._region_frames, islands_removed=t[0], pixels_cleared=t[1], holes_filled=t[2], pixels_filled=t[3])
        if self.scorer is not None:
            self.scores = self.scorer.finish()
        if self.tracks is not None:
            self.tracks.write(path.join(self.tracks_output_root, self.video_name))
        if self.polygons is not None:
            self.polygons.write(path.join(self.polygons_output_root, self.video_name))

    # ---- the writer thread: one function per output family, called by _writer in this order ---------------------------------------
    def _put(self, root, folder, name, data: bytes):
        os.makedirs(path.join(root, self.video_name, folder), exist_ok=True)
        with open(path.join(root, self.video_name, folder, name), 'wb') as f:
            f.write(data)

    def _mask_stream(self, b: EgressBuffers) -> bytes:
        """egress='device': the frame's zlib stream, once its copy has landed.  Raises when the device set the error word."""
        return b.png.fetch(b.event)

    def _write_mask(self, job):
        """``<frame>.png``: the device's stream wrapped (egress='device'; no PIL), or the id plane through PIL.
        -> the RGB mask of a long-id frame (the host overlay blends it)"""
        stem, rgb_mask = job.frame_name[:-4], None
        if job.egress is not None:
            b = job.egress
            self._put(self.output_root, '', stem + '.png', png_container.assemble(self._mask_stream(b), b.H, b.W, self.palette))
        elif self.save_mask:
            out_mask = job.mask.numpy()
            if self.use_long_id:
                m = out_mask.astype(np.uint32)
                rgb_mask = np.zeros((*m.shape[-2:], 3), dtype=np.uint8)
                for oid in job.all_obj_ids:
                    rgb_mask[m == oid] = self.id2rgb_converter.convert(oid)[1]
                out_img = Image.fromarray(rgb_mask)
            else:
                out_img = Image.fromarray(out_mask.astype(np.uint8))
                if self.palette is not None:
                    out_img.putpalette(self.palette)
            out_dir = path.join(self.output_root, self.video_name)
            os.makedirs(out_dir, exist_ok=True)
            out_img.save(path.join(out_dir, stem + '.png'))
        return rgb_mask

    def _device_rle(self, b: EgressBuffers, all_obj_ids) -> dict:
        """BURST, egress='device': {object id: RLE string} of the frame's non-empty objects from the device encoder.  If the strings
        did not fit the device stream, the frame is encoded here from a copy of the id plane (logged once)."""
        raw = b.rle.fetch(b.event)
        if raw is None:
            return _host_rle(self._copies.to_host(b.ids), all_obj_ids)
        table = np.frombuffer(raw, dtype=np.int32, count=4 * len(all_obj_ids)).reshape(-1, 4)
        raw = raw[RLE_TABLE - 16:]
        return {oid: raw[off:off + ln].decode('ascii') for oid, (off, ln, _, area) in zip(all_obj_ids, table.tolist()) if area > 0}

    def _write_burst(self, job):
        """BURST, an annotated frame: the objects' segmentations into ``self.segmentations`` (results_utils.py:153-171)"""
        if self.json_style != 'burst' or job.frame_name not in self.annotated_frames:
            return
        index = self.annotated_frames.index(job.frame_name)
        input_segments, frame_segments = self.input_segmentations[index], self.segmentations[index]
        if job.rle:
            strings = self._device_rle(job.egress, job.all_obj_ids)
        else:
            strings = _host_rle(job.mask.numpy(), [i for i in job.all_obj_ids if i not in input_segments])
        for oid in job.all_obj_ids:
            # (as executed: the object ids are ints, the keys of a json that was loaded from a file are strings, so the copy
            # only happens for an init_json whose keys are ints; everything else is encoded.  Keys turn into strings at json.dump)
            if oid in input_segments:
                frame_segments[oid] = input_segments[oid]
            elif oid in strings:
                frame_segments[oid] = {'rle': strings[oid]}

    def _write_scores(self, job):
        if not self.save_scores:
            return
        sc_dir = path.join(self.score_output_root, self.video_name)
        os.makedirs(sc_dir, exist_ok=True)
        if job.last_frame:                                     # the reference's backward.hkl: {object id: tmp id}
            ids = sorted(job.tmp_to_obj.items())
            np.savez(path.join(sc_dir, 'backward.npz'), obj_ids=np.array([o for _, o in ids], dtype=np.int64),
                     tmp_ids=np.array([t for t, _ in ids], dtype=np.int64))
        np.savez_compressed(path.join(sc_dir, job.frame_name[:-4] + '.npz'), prob=job.prob.numpy())

    def _write_matte(self, job):
        """The files of one frame's vis modes, soft masks and matte."""
        b, stem = job.matte, job.frame_name[:-4]
        if b is None:
            return
        for k, mode in enumerate(b.modes):
            segment = b.jpeg[k].fetch(b.event)
            if segment is not None:
                self._put(self.output_root, path.join('visualization', mode), stem + '.jpg', jpeg_writer.wrap(segment, b.H, b.W, self._jpeg_tables[0]))
            else:                                    # the segment did not fit the device stream: the composed frame through PIL
                folder = path.join(self.output_root, self.video_name, 'visualization', mode)
                os.makedirs(folder, exist_ok=True)
                Image.fromarray(self._copies.to_host(b.frames[k])).save(path.join(folder, stem + '.jpg'))
        for k, slab in enumerate(b.png):
            data = png_container.assemble(slab.fetch(b.event), b.H, b.W, None)
            if k >= b.K:
                self._put(self.output_root, 'alpha', stem + '.png', data)
            elif job.matte_objects[k] is not None:
                self._put(self.output_root, path.join('soft_masks', str(job.matte_objects[k])), stem + '.png', data)
        if b.cutout is not None:
            self._put(self.output_root, 'cutout', stem + '.png', png_container.assemble_image(b.cutout.fetch(b.event), b.H, b.W, 4))
        elif b.cutout_mode == 'host':                # a row beyond the device stage's limit: frame and matte through PIL
            b.event.synchronize()
            rgba = np.dstack([self._copies.to_host(job.matte_keep[2]), self._copies.to_host(b.final_plane(b.K))])     # (the refined plane under matte_refine)
            folder = path.join(self.output_root, self.video_name, 'cutout')
            os.makedirs(folder, exist_ok=True)
            Image.fromarray(rgba, 'RGBA').save(path.join(folder, stem + '.png'), compress_level=1)

    def _write_tracks(self, job):
        """The frame's rows to the track report: its table has landed behind its event (no table: a frame without objects)."""
        if job.track_meta is None:
            return
        index, objs, H, W = job.track_meta
        if job.tracks is not None:
            job.tracks.event.synchronize()
            table = job.tracks.host[:len(objs) * 12].numpy().reshape(-1, 12).copy()
        else:
            table = np.zeros((0, 12), dtype=np.int32)
        self.tracks.add(job.frame_name, index, table, objs, H, W)

    def _write_polygons(self, job):
        """The frame's rings to the polygon report: its slab has landed behind its event (no slab: a frame without objects).  A frame that
        did not fit the stage's capacities is traced here from the id plane (the host's copy, or a copy of the device's)."""
        if job.poly_meta is None:
            return
        index, objs, H, W = job.poly_meta
        n, b = len(objs), job.polygons
        raw = b.slab.fetch(b.event) if b is not None else b''
        if raw is None:
            plane = job.mask.numpy() if job.mask is not None else self._copies.to_host(job.egress.ids)
            rings, verts, table = trace_rings(np.ascontiguousarray(plane, dtype=np.uint8), objs, self.region_connectivity)
        else:
            R = int(b.slab.host[:16].view(torch.int32)[2]) if b is not None else 0
            table = np.frombuffer(raw, dtype=np.int32, count=4 * n).reshape(-1, 4).copy()
            rings = np.frombuffer(raw, dtype=np.int32, count=4 * R, offset=POLY_TABLE if R else 0).reshape(-1, 4).copy()
            verts = np.frombuffer(raw, dtype=np.uint32, offset=POLY_TABLE + 16 * R).copy() if b is not None else np.zeros(0, dtype=np.uint32)
        self.polygons.add(job.frame_name[:-4], index, rings, verts, table, objs, H, W)

    def _write_regions(self, job):
        """min_region / fill_holes: the frame's counts, landed behind their event, to the video's totals"""
        if job.regions is not None:
            job.regions.event.synchronize()
            self._region_totals += job.regions.host.numpy()
            self._region_frames += 1

    def _write_bands(self, job):
        """trimap / trimap_objects / dilate_mask: the frame's planes as 8-bit grey PNGs"""
        b = job.bands
        if b is None:
            return
        for (folder, oid), slab in zip(job.band_planes, b.png):
            data = png_container.assemble(slab.fetch(b.event), b.H, b.W, None)
            self._put(self.output_root, folder if oid is None else path.join(folder, str(oid)), job.frame_name[:-4] + '.png', data)

    def _write_redact(self, job):
        """``redacted/<frame>.jpg``: the device's segment wrapped; a segment that did not fit the device stream: the buffer through PIL"""
        b = job.redact
        if b is None:
            return
        stem = job.frame_name[:-4]
        segment = b.jpeg.fetch(b.event)
        if segment is not None:
            self._put(self.output_root, 'redacted', stem + '.jpg', jpeg_writer.wrap(segment, b.H, b.W, self._jpeg_tables[0]))
        else:
            folder = path.join(self.output_root, self.video_name, 'redacted')
            os.makedirs(folder, exist_ok=True)
            Image.fromarray(self._copies.to_host(b.out)).save(path.join(folder, stem + '.jpg'))

    def _write_overlay(self, job, rgb_mask):
        """``<frame>.jpg`` of ``visualize``: the device's segment wrapped (overlay='device'; no PIL), else the host's blend through PIL
        -- also for a frame whose segment did not fit the device stream."""
        stem = job.frame_name[:-4]
        segment = job.overlay.jpeg.fetch(job.overlay.event) if job.overlay is not None else None
        if segment is not None:
            self._put(self.visualize_output_root, '', stem + '.jpg', jpeg_writer.wrap(segment, job.overlay.H, job.overlay.W, self._jpeg_tables[0]))
        elif self.visualize:
            out_mask = job.mask.numpy() if job.mask is not None else None
            if job.overlay is not None:                        # the segment did not fit the device stream: this frame on the host
                if out_mask is None:
                    out_mask = job.ids.cpu().numpy()
                image_np = np.array(Image.open(job.path_to_image).convert('RGB')) if job.path_to_image is not None else job.frame.cpu().numpy()
            elif job.path_to_image is None:
                raise ValueError('Cannot visualize without path_to_image')
            else:
                image_np = np.array(Image.open(job.path_to_image).convert('RGB'))
            if rgb_mask is None:
                rgb_mask = np.zeros((*out_mask.shape, 3), dtype=np.uint8)
                for oid in job.all_obj_ids:
                    rgb_mask[out_mask == oid] = self.colors[oid % len(self.colors)]
            alpha = ((out_mask == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
            blend = (image_np * alpha + rgb_mask * (1 - alpha)).astype(np.uint8)
            vis_dir = path.join(self.visualize_output_root, self.video_name)
            os.makedirs(vis_dir, exist_ok=True)
            Image.fromarray(blend).save(path.join(vis_dir, stem + '.jpg'))


def _host_rle(ids: np.ndarray, all_obj_ids) -> dict:
    """{object id: RLE string} of the objects with a non-empty mask (results_utils.py:166-171)."""
    out = {}
    for oid in all_obj_ids:
        seg = ids == oid
        if seg.sum() > 0:
            out[oid] = coco_rle.encode(seg)
    return out


def _writer(queue: Queue):
    while True:
        job = queue.get()
        if job is None:
            queue.task_done()
            break
        try:
            s = job.saver
            rgb_mask = s._write_mask(job)
            s._write_burst(job)
            s._write_scores(job)
            s._write_matte(job)
            s._write_tracks(job)
            s._write_polygons(job)
            s._write_regions(job)
            s._write_bands(job)
            s._write_redact(job)
            s._write_overlay(job, rgb_mask)
        except Exception as e:                                 # keep the queue draining; surface the problem
            log.error(f'result writer failed on {job.frame_name}: {e}')
        finally:
            for b in job.held():                               # the frame's buffers go back to their pools
                b.pool.put(b)
        queue.task_done()


def make_zip(dataset, run_dir, exp_id, mask_output_root):
    """results_utils.py:233-256: the archive layouts the benchmark servers expect."""
    if dataset.startswith('y') or dataset == 'lvos-test':
        log.info(f'Making zip for {dataset}...')
        shutil.make_archive(path.join(run_dir, f'{exp_id}_{dataset}'), 'zip', run_dir, 'Annotations')
    elif dataset in ('d17-test-dev', 'mose-val'):
        log.info(f'Making zip for {dataset}...')
        shutil.make_archive(path.join(run_dir, f'{exp_id}_{dataset}'), 'zip', mask_output_root)
    else:
        log.info(f'Not making zip for {dataset}.')
