"""``TrackReport``: one row per object and frame -- is it there, where is it, how large is it, how sure was the model -- for consumers
that use the engine as a tracker or a labelling back end (not in the reference).

The integers come from the device (PROB_TO_ID flags == 1024, csrc/tracks.hip; include/cutie_hip.h): per listed object a row of 12 int32
words -- 0 area | 1 xmin 2 ymin 3 xmax 4 ymax | 5,6 sum of x | 7,8 sum of y | 9 confidence samples | 10,11 confidence sum, the pairs 64-bit
values, low word first.  x is the column and y the row of the id plane the PNG is written from, 0-based.  Here they become, in float64:

  bbox       = [xmin, ymin, xmax - xmin + 1, ymax - ymin + 1]                 (COCO order: x, y, width, height)
  centroid   = [sum of x / area, sum of y / area]
  confidence = confidence sum / (65535 * confidence samples), or null when the object won no sample -- or no probabilities were given
               (``ResultSaver.process_merged``: the merge has S probability sources and no single model resolution).  The samples are
               those of the MODEL's resolution whose largest plane is the object's; the value is the mean of that largest probability,
               quantised to 16 bits per sample.

Files, one pair per video (``write``):

  tracks.json      {"video": name, "height": H, "width": W, "objects": [ids ...],
                    "frames": [{"frame": "00000", "index": 1,
                                "objects": {"1": {"area": 1234, "bbox": [x, y, w, h], "centroid": [cx, cy], "confidence": 0.97}, ...}}, ...]}
                   keys in this order, frames in the order reported; "objects" at the top: every id any frame listed, in order of first
                   appearance; an object without a pixel keeps its entry with "area": 0 and null for the rest, so the schema does not
                   depend on the content.  Floats are written with ``repr`` (json's own float format).
  tracks_mot.txt   MOT-challenge style rows ``index,id,x,y,w,h,confidence,-1,-1,-1`` for every object with area > 0, sorted by index, then
                   id.  NOTE: x, y are the json's 0-BASED xmin, ymin (the MOT benchmark's own files count from 1); the confidence has six
                   decimals, or -1 when it is null.  ``index`` is the frame's 1-based position in the video as the reader orders it."""
import json
import os
from typing import Dict, List, Optional

import numpy as np

WORDS = 12                       # int32 words of a table row (csrc/tracks.hip TRK_WORDS)


def _u64(lo: int, hi: int) -> int:
    return (int(lo) & 0xffffffff) | ((int(hi) & 0xffffffff) << 32)


def row_to_entry(row) -> Dict:
    """One table row -> the json entry of the object (Python ints and float64)."""
    area = int(row[0])
    if area <= 0:
        return {'area': 0, 'bbox': None, 'centroid': None, 'confidence': None}
    xmin, ymin, xmax, ymax = (int(v) for v in row[1:5])
    count, total = int(row[9]), _u64(row[10], row[11])
    return {'area': area, 'bbox': [xmin, ymin, xmax - xmin + 1, ymax - ymin + 1],
            'centroid': [_u64(row[5], row[6]) / area, _u64(row[7], row[8]) / area],
            'confidence': (total / (65535 * count)) if count > 0 else None}


class TrackReport:
    def __init__(self, video_name: str = ''):
        self.video_name = video_name
        self.height: Optional[int] = None
        self.width: Optional[int] = None
        self.objects: List[int] = []          # every id any frame listed, in order of first appearance
        self.frames: List[Dict] = []          # in the order reported

    def add(self, frame_name, frame_index, table_row_block, obj_ids, H, W):
        """One frame: ``table_row_block`` = int32 [n, 12] (anything numpy reads: the host copy of the device table), ``obj_ids`` the n
        object ids of its rows; ``frame_name`` with or without an extension; ``frame_index``: the frame's 1-based position in the video."""
        obj_ids = [int(v) for v in obj_ids]
        table = np.asarray(table_row_block).reshape(-1, WORDS)[:len(obj_ids)]
        if table.shape[0] != len(obj_ids):
            raise ValueError(f'TrackReport.add: {len(obj_ids)} objects, a table of {table.shape[0]} rows')
        H, W = int(H), int(W)
        if self.height is None:
            self.height, self.width = H, W
        elif (self.height, self.width) != (H, W):
            raise ValueError(f'TrackReport.add: a frame of {H} x {W} in a video of {self.height} x {self.width}')
        objects = {}
        for oid, row in zip(obj_ids, table.tolist()):
            if oid not in self.objects:
                self.objects.append(oid)
            objects[str(oid)] = row_to_entry(row)
        self.frames.append({'frame': os.path.splitext(str(frame_name))[0], 'index': int(frame_index), 'objects': objects})

    def as_dict(self) -> Dict:
        return {'video': self.video_name, 'height': self.height, 'width': self.width, 'objects': list(self.objects), 'frames': list(self.frames)}

    def json_text(self) -> str:
        return json.dumps(self.as_dict()) + '\n'

    def mot_text(self) -> str:
        rows = []
        for fr in self.frames:
            for key, e in fr['objects'].items():
                if e['area'] > 0:
                    rows.append((fr['index'], int(key), e))
        rows.sort(key=lambda r: (r[0], r[1]))
        return ''.join('%d,%d,%d,%d,%d,%d,%s,-1,-1,-1\n' % (index, oid, *e['bbox'], '-1' if e['confidence'] is None else '%.6f' % e['confidence'])
                       for index, oid, e in rows)

    def write(self, dir):
        """``dir``/tracks.json and ``dir``/tracks_mot.txt (the module docstring)."""
        os.makedirs(dir, exist_ok=True)
        with open(os.path.join(dir, 'tracks.json'), 'w') as f:
            f.write(self.json_text())
        with open(os.path.join(dir, 'tracks_mot.txt'), 'w') as f:
            f.write(self.mot_text())
