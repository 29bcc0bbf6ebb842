"""The BURST test set = one json of sequences over a folder of frames; same surface as the reference
cutie/inference/data/burst_test_dataset.py:6-26."""
import json

from .burst_video_reader import BURSTVideoReader
from .video_reader import INGEST_MODES


class BURSTTestDataset:
    def __init__(self, image_dir: str, json_dir: str, *, size: int = -1, skip_frames: int = -1, ingest: str = 'host'):
        if ingest not in INGEST_MODES:
            raise ValueError(f'ingest must be one of {INGEST_MODES}, not {ingest!r}')
        self.image_dir, self.json_dir, self.size, self.skip_frames, self.ingest = image_dir, json_dir, size, skip_frames, ingest
        with open(json_dir) as f:
            self.json = json.load(f)
        self.sequences = self.json['sequences']

    def get_datasets(self):
        for sequence in self.sequences:
            yield BURSTVideoReader(self.image_dir, sequence, size=self.size, skip_frames=self.skip_frames, ingest=self.ingest)

    def __len__(self):
        return len(self.sequences)
