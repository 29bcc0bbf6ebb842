"""A BURST-style dataset in a temporary folder, for tests/test_burst_cpu.py and tests/test_gpu_burst.py: one or more copies of the four
tests/golden/bike frames as sequences, annotated on frames 0 and 2; object 1 comes with the first annotated frame, object 2 with the
second one; their masks are those of bike/00000.png, encoded with the codec under test's numpy side (coco_rle)."""
import json
import os
import shutil

import numpy as np
from PIL import Image

from cutie_amd.inference.utils import coco_rle

HERE = os.path.dirname(os.path.abspath(__file__))
BIKE = os.path.join(HERE, 'golden', 'bike')
FRAMES = ['00000.jpg', '00001.jpg', '00002.jpg', '00003.jpg']
ANNOTATED = ['00000.jpg', '00002.jpg']
DATASET = 'bikeset'


def first_mask() -> np.ndarray:
    return np.array(Image.open(os.path.join(BIKE, '00000.png')))


def sequence(name: str) -> dict:
    m = first_mask()
    return {'id': 1, 'dataset': DATASET, 'seq_name': name, 'width': int(m.shape[1]), 'height': int(m.shape[0]), 'fps': 30,
            'all_image_paths': list(FRAMES), 'annotated_image_paths': list(ANNOTATED), 'track_category_ids': {'1': 3, '2': 7},
            'segmentations': [{'1': {'rle': coco_rle.encode(m == 1)}}, {'2': {'rle': coco_rle.encode(m == 2)}}]}


def make(root, names=('bike',)):
    """-> (image root, path of the dataset json, the dataset json as written)"""
    images = os.path.join(str(root), 'frames')
    for name in names:
        d = os.path.join(images, DATASET, name)
        os.makedirs(d)
        for f in FRAMES:
            shutil.copy(os.path.join(BIKE, f), d)
    meta = {'split': 'val', 'category_names': {'3': 'person', '7': 'bicycle'}, 'sequences': [sequence(n) for n in names]}
    json_path = os.path.join(str(root), 'first_frame_annotations.json')
    with open(json_path, 'w') as f:
        json.dump(meta, f)
    return images, json_path, meta
