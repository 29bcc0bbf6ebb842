"""Frame-by-frame reader of one BURST sequence; same surface and semantics as the reference
cutie/inference/data/burst_video_reader.py:14-102: the frame list is the json's ``all_image_paths`` (with ``skip_frames`` > 0 every
skip_frames-th frame united with the annotated ones, sorted), ``info['save']`` only on annotated frames, the masks of an annotated frame
composed from its COCO RLE strings in dict order (a later object overwrites an earlier one; ids <= 255), ``size`` >= 0 resizes EVERY
frame (shorter side; bilinear + antialias for frames, nearest for masks), ``use_long_id = False`` and the DAVIS palette.

pycocotools is not required: the strings are decoded by inference/utils/coco_rle.py.  The image side is ``VideoReader``'s
(``_image``), so ``get(idx, ingest=...)`` serves the three ingest modes."""
import threading
from collections import Counter
from os import path
from typing import Dict, Optional

import numpy as np
import torch
from PIL import Image

from ..utils import coco_rle
from ..utils.results_utils import davis_palette
from .video_reader import INGEST_MODES, VideoReader, _nearest, _stem


class BURSTVideoReader(VideoReader):
    def __init__(self, image_root: str, sequence_json: Dict, *, size: int = -1, skip_frames: int = -1, ingest: str = 'host'):
        if ingest not in INGEST_MODES:
            raise ValueError(f'ingest must be one of {INGEST_MODES}, not {ingest!r}')
        self.ingest = ingest
        self.decode_fallbacks = Counter()
        self._fallback_lock = threading.Lock()
        self.sequence_json = sequence_json
        self.vid_name = sequence_json['seq_name']
        annotated = sequence_json['annotated_image_paths']
        self.annotated_frames = [_stem(f) for f in annotated]
        self.image_dir = self.size_dir = path.join(image_root, sequence_json['dataset'], self.vid_name)
        self.frames = sequence_json['all_image_paths']
        if skip_frames > 0:
            self.frames = sorted(set(self.frames[::skip_frames]).union(annotated))
        self.size, self.skip_frames = size, skip_frames
        self.use_long_id = False
        self.use_all_mask = True                              # every annotated frame brings its masks (eval_vos.lockstep_key)
        self.palette = davis_palette

    def get(self, idx, ingest: Optional[str] = None):
        ingest = self.ingest if ingest is None else ingest
        if ingest not in INGEST_MODES:
            raise ValueError(f'ingest must be one of {INGEST_MODES}, not {ingest!r}')
        frame = self.frames[idx]
        im_path = path.join(self.image_dir, frame)
        img, shape, resized, rgb_hw = self._image(frame, im_path, ingest, always=True)
        annotated = _stem(frame) in self.annotated_frames
        data = {}
        if annotated:
            segmentations = self.sequence_json['segmentations'][self.annotated_frames.index(_stem(frame))]
            if len(segmentations) > 0:
                mask = np.zeros(shape, dtype=np.uint8)
                for oid, segment in segmentations.items():
                    assert int(oid) <= 255, 'Too many objects in the frame -- long id needed'
                    mask[coco_rle.decode(segment['rle'], *shape) == 1] = int(oid)
                pil = Image.fromarray(mask)
                if resized:
                    pil = _nearest(pil, self.size)
                data['mask'] = torch.from_numpy(np.array(pil)).long()
                data['valid_labels'] = np.array([int(k) for k in segmentations.keys()])
        data.update(img)
        data['info'] = {'frame': frame, 'save': annotated, 'shape': shape, 'resize_needed': resized,
                        'time_index': self.frames.index(frame), 'path_to_image': im_path}
        if ingest != 'host':
            data['info']['rgb_shape'] = tuple(rgb_hw)
        return data

    def get_palette(self):
        return davis_palette
