"""``BURSTResultHandler``: collects the per-sequence json of every ``ResultSaver`` and writes ``predictions.json``; same surface as the
reference cutie/inference/utils/burst_utils.py:6-19 (the dataset json without its sequences, then the predicted ones appended)."""
import copy
import json
from os import path


class BURSTResultHandler:
    def __init__(self, dataset_json):
        self.dataset_json = copy.deepcopy(dataset_json)
        self.dataset_json['sequences'] = []          # the metadata stays, the input segmentations go

    def add_sequence(self, sequence_json):
        self.dataset_json['sequences'].append(sequence_json)

    def dump(self, root):
        with open(path.join(root, 'predictions.json'), 'w') as f:
            json.dump(self.dataset_json, f)
