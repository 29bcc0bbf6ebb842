"""The launch sequence of a ResultSaver, pinned: per frame the op lists it runs -- (kind, flags, ints, floats) of every descriptor, in order
and cut into the same lists -- and which stage reads what another wrote (every pointer slot as the ordinal of the address's first appearance
within the frame; a null pointer is 0).  tests/golden/saver_launches.json is what the tree before the saver's frame paths were made one
recorded; every later tree must reproduce it exactly.  The recorder is the interpreter of tests/mock_exec_regions.py; the three PROB_TO_ID
stages without a CPU interpreter are stubbed (flags == 128 leaves "0 bytes, no error" in its status block, flags == 256 and 512 do nothing):
what these leave in the files is not looked at.

``python tests/test_saver_launches_cpu.py`` rewrites the golden file from the tree it runs in."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(HERE))

from cutie_amd import _lib

from mock_exec import I32, view
from mock_exec_regions import RegionsMockExecutor

GOLDEN = os.path.join(HERE, 'golden', 'saver_launches.json')
OUT_HW = (37, 61)
THR = dict(min_region=4, fill_holes=4)


class Recorder(RegionsMockExecutor):
    def __init__(self):
        super().__init__()
        self.lists = []                      # per run(): [(kind, flags, ints, floats, pointers)]

    def run(self, arr):
        self.lists.append([(int(r['kind']), int(r['flags']), [int(v) for v in r['i']], [float(v) for v in r['f']], [int(v) for v in r['p']])
                           for r in arr])
        super().run(arr)

    def _op_36(self, flags, i, f, p):
        if flags == 128:                     # the JPEG stage: an empty segment, no error
            view(p[4], I32, (4,)).zero_()
        elif flags not in (256, 512):        # (the composites and the soft masks: nothing)
            super()._op_36(flags, i, f, p)

    def take_frame(self):
        """The lists run since the last call, pointers as ordinals of their first appearance (0 = null), trailing zeros trimmed."""
        seen, out = {}, []

        def trim(v):
            v = list(v)
            while v and v[-1] == 0:
                v.pop()
            return v
        for ops in self.lists:
            out.append([[kind, flags, trim(ints), trim(floats), trim(seen.setdefault(a, len(seen) + 1) if a else 0 for a in ptrs)]
                        for kind, flags, ints, floats, ptrs in ops])
        self.lists = []
        return out


class _Scorer:
    def add(self, frame_name, mask):
        assert mask.dtype == torch.uint8

    def finish(self):
        return 'done'


def _saver(out, om, **kw):
    from cutie_amd.inference.utils.results_utils import ResultSaver

    def to_mask(prob, dtype=torch.int64):
        lut = torch.zeros(prob.shape[0], dtype=torch.long)
        for t, o in om.tmp_id_to_obj.items():
            lut[t] = o.id
        return lut[prob.argmax(0)].to(dtype)
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om, output_prob_to_mask=to_mask)
    kw.setdefault('dataset', 'generic')
    return ResultSaver(os.path.join(out, 'masks'), 'vid', object_manager=om, use_long_id=False, processor=proc, **kw)


def _prob(rng, P, h=24, w=40):
    """[P, h, w] probabilities as the un-padded view of a padded buffer"""
    from test_track_report_cpu import softmax_planes
    buf = torch.full((P, h + 3, w + 8), 7.0)
    buf[:, 1:1 + h, 2:2 + w] = torch.from_numpy(softmax_planes(rng, P, h // 4, w // 4).repeat(4, 1).repeat(4, 2))
    return buf[:, 1:1 + h, 2:2 + w]


NAMES = ['00000.jpg', '00001.jpg', '00002.jpg']


def _burst():
    return dict(dataset='burst-val', init_json={'segmentations': [{}], 'annotated_image_paths': [NAMES[0]], 'seq_name': 'vid'})


def _tracks():
    from cutie_amd.inference.utils.track_report import TrackReport
    return TrackReport()


def _overlay(out):
    return dict(visualize=True, overlay='device', visualize_output_root=os.path.join(out, 'vis'))


MATTE = dict(vis_modes=('davis', 'popup'), soft_masks=True, alpha_matte=True)


def _all_on(out):
    return dict(egress='device', **_overlay(out), **MATTE, **THR, tracks=_tracks(), scorer=_Scorer(), **_burst())


# name -> (saver options given the output folder, frames, merged, object added before the last frame)
CASES = {}
for _egress in ('host', 'device'):
    _e = dict(egress=_egress)
    CASES[f'{_egress}-plain'] = (lambda out, e=_e: dict(e), 2, False, False)
    CASES[f'{_egress}-regions'] = (lambda out, e=_e: dict(e, **THR), 2, False, False)
    CASES[f'{_egress}-tracks'] = (lambda out, e=_e: dict(e, tracks=_tracks()), 2, False, False)
    CASES[f'{_egress}-scorer'] = (lambda out, e=_e: dict(e, scorer=_Scorer()), 2, False, False)
    CASES[f'{_egress}-burst'] = (lambda out, e=_e: dict(e, **_burst()), 2, False, False)
    CASES[f'{_egress}-overlay'] = (lambda out, e=_e: dict(e, **_overlay(out)), 2, False, False)
    CASES[f'{_egress}-merged'] = (lambda out, e=_e: dict(e), 2, True, False)
    CASES[f'{_egress}-merged-regions-tracks'] = (lambda out, e=_e: dict(e, **THR, tracks=_tracks()), 2, True, False)
CASES['matte'] = (lambda out: dict(MATTE), 2, False, False)
CASES['all-on'] = (_all_on, 2, False, False)
CASES['all-on-object-added'] = (_all_on, 3, False, True)


def record(name, resize, out):
    """The frames of one case: [[op list, ...], ...]"""
    from cutie_amd.inference.object_manager import ObjectManager
    options, T, merged, added = CASES[name]
    rng = np.random.default_rng(7)
    ex = Recorder()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    try:
        om = ObjectManager()
        om.add_new_objects([5, 3])
        saver = _saver(out, om, **options(out))
        H, W = OUT_HW if (resize or merged) else (24, 40)
        frames = []
        for t in range(T):
            if added and t == T - 1:
                om.add_new_objects([7])
            P = len(om.tmp_id_to_obj) + 1
            image = torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
            if merged:
                members = [_prob(rng, P, 24, 40), _prob(rng, P, 16, 28)]
                saver.process_merged(members, NAMES[t], (H, W), last_frame=t == T - 1, image_u8=image)
            else:
                saver.process(_prob(rng, P), NAMES[t], resize_needed=resize, shape=OUT_HW if resize else None, last_frame=t == T - 1,
                              image_u8=image)
            frames.append(ex.take_frame())
        saver.end()
        return frames
    finally:
        _lib.set_executor_for_testing(None)


def _key(name, resize):
    return f"{name}/{'resized' if resize else 'native'}"


def _variants():
    """(case, resize): a merge always resamples its members, so it has one variant"""
    return [(n, r) for n in CASES for r in ((False, True) if not CASES[n][2] else (True,))]


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('name,resize', _variants())
def test_the_launch_sequence_is_the_recorded_one(tmp_path, golden, name, resize):
    got = record(name, resize, str(tmp_path))
    want = golden[_key(name, resize)]
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert [len(ops) for ops in g] == [len(ops) for ops in w], f'frame {t}: the op lists are cut differently'
        assert g == w, f'frame {t}'


def test_the_record_covers_the_matrix(golden):
    assert sorted(golden) == sorted(_key(n, r) for n, r in _variants())
    flags = lambda frame: [[op[1] for op in ops] for ops in frame]
    # an all-on frame: [ids, filter, png, rle] [overlay] [composites + their JPEG stages, alpha in the popup, soft, png x 3] [tracks]
    assert flags(golden['all-on/resized'][0]) == [[4, 2048, 8, 32], [128], [256, 128, 256, 128, 512, 8, 8, 8], [1024]]
    assert flags(golden['all-on/resized'][1]) == [[4, 2048, 8], [128], [256, 128, 256, 128, 512, 8, 8, 8], [1024]]      # not annotated: no strings
    assert flags(golden['all-on-object-added/native'][2]) == [[0, 2048, 8], [128], [256, 128, 256, 128, 512, 8, 8, 8, 8], [1024]]
    assert flags(golden['device-plain/native'][0]) == [[8]] and flags(golden['device-plain/resized'][0]) == [[12]]       # fused: the filter is off
    assert flags(golden['host-plain/native'][0]) == [] and flags(golden['host-regions/native'][0]) == [[2048]]
    assert flags(golden['device-merged/resized'][0]) == [[28]] and flags(golden['host-merged-regions-tracks/resized'][0]) == [[20, 2048], [1024]]


if __name__ == '__main__':
    import tempfile
    rec = {}
    for n, r in _variants():
        with tempfile.TemporaryDirectory() as d:
            rec[_key(n, r)] = record(n, r, d)
    with open(GOLDEN, 'w') as f:
        json.dump(rec, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print(GOLDEN, os.path.getsize(GOLDEN), 'bytes')
