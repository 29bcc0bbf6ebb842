"""Everything on in one ResultSaver against each output family alone (the combinations the features' own tests check only pairwise): device
egress, the device overlay, two vis modes, the soft masks, the matte, the track report, a scorer and the region filter in saver A; savers
B .. E switch on one family each (B: device egress; C: host egress with the device overlay; D: the vis modes, soft masks and matte --
on device egress as in A, where the launches sample the model's planes in place: the host path resamples them with torch first, which is
other arithmetic --; E: the track report and the scorer).  Every file of A is the bytes of the same relative path of the saver that owns the family; tracks.json and
the region totals match; the planes the scorer saw are the pixels of the PNGs.  An object is added before the third frame, so the
object-keyed tables and the matte buffers' plane count change inside the video."""
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib

from test_track_report_cpu import softmax_planes

pytestmark = pytest.mark.gpu
NAMES = ['00000.jpg', '00001.jpg', '00002.jpg']
THR = dict(min_region=4, fill_holes=4)


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


class Scorer:
    def __init__(self):
        self.seen = []

    def add(self, frame_name, mask):
        assert mask.dtype == torch.uint8 and mask.device.type == 'cuda'
        self.seen.append((frame_name, mask.clone()))

    def finish(self):
        return [(n, m.cpu().numpy()) for n, m in self.seen]


@pytest.fixture(scope='module')
def inputs():
    """per frame the probabilities [P, 24, 40] on the device (blocky planes with single samples flipped: specks and holes for the filter;
    un-padded views of padded buffers) -- P = 3, 3, 4 -- and per output size the uint8 frames"""
    rng = np.random.default_rng(31)
    probs = []
    for P in (3, 3, 4):
        soft = softmax_planes(rng, P, 6, 10).repeat(4, 1).repeat(4, 2)
        flip = rng.random((24, 40)) < 0.06
        soft[:, flip] = np.roll(soft, 1, axis=0)[:, flip]
        buf = torch.full((P, 27, 48), 7.0, device='cuda')
        buf[:, 1:25, 2:42] = torch.from_numpy(soft).cuda()
        probs.append(buf[:, 1:25, 2:42])
    images = {hw: [torch.from_numpy(rng.integers(0, 256, size=(*hw, 3), dtype=np.uint8)).cuda() for _ in NAMES] for hw in ((24, 40), (37, 61))}
    return probs, images


def _run(root, probs, images, shape, **kw):
    """one saver over the three frames -> (saver, {relative path: bytes} of everything it wrote)"""
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver, davis_palette
    om = ObjectManager()
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cuda', torch.cuda.current_device())), object_manager=om)
    proc.output_prob_to_mask = lambda prob, dtype=torch.int64: InferenceCore.output_prob_to_mask(proc, prob, dtype=dtype)
    saver = ResultSaver(os.path.join(root, 'masks'), 'vid', dataset='generic', object_manager=om, use_long_id=False, palette=list(davis_palette),
                        processor=proc, visualize_output_root=os.path.join(root, 'vis'), tracks_output_root=os.path.join(root, 'tracks'), **THR, **kw)
    om.add_new_objects([5, 3])
    for t, name in enumerate(NAMES):
        if t == 2:
            om.add_new_objects([7])
        saver.process(probs[t], name, resize_needed=shape is not None, shape=shape, last_frame=t == 2, image_u8=images[t], frame_index=t + 1)
    saver.end()
    files = {}
    for folder, _, names in os.walk(root):
        for n in names:
            full = os.path.join(folder, n)
            with open(full, 'rb') as f:
                files[os.path.relpath(full, root)] = f.read()
    return saver, files


def _family(rel):
    parts = rel.split(os.sep)
    if parts[0] == 'vis':
        return 'overlay'
    if parts[0] == 'tracks':
        return 'tracks'
    return 'mask' if len(parts) == 3 else 'matte'        # masks/vid/<frame>.png | masks/vid/{visualization,soft_masks,alpha}/...


@pytest.mark.parametrize('shape', [(37, 61), None], ids=['resized', 'native'])
def test_everything_on_equals_each_family_alone(tmp_path, inputs, shape):
    from cutie_amd.inference.utils.track_report import TrackReport
    probs, images = inputs
    images = images[shape or (24, 40)]
    matte = dict(vis_modes=('davis', 'popup'), soft_masks=True, alpha_matte=True)
    overlay = dict(visualize=True, overlay='device')
    runs = {name: _run(str(tmp_path / name), probs, images, shape, **kw) for name, kw in (
        ('A', dict(egress='device', **overlay, **matte, tracks=TrackReport(), scorer=Scorer())),
        ('mask', dict(egress='device')),
        ('overlay', dict(egress='host', **overlay)),
        ('matte', dict(egress='device', **matte)),        # (as in A the launches sample the model's planes in place; egress='host' resamples them with torch first)
        ('tracks', dict(tracks=TrackReport(), scorer=Scorer())))}
    a, files = runs['A']
    assert a.egress == 'device' and a.overlay == 'device' and runs['mask'][0].egress == 'device'
    assert runs['overlay'][0].egress == 'host' and runs['overlay'][0].overlay == 'device'
    stems = [n[:-4] for n in NAMES]
    want = [os.path.join('masks', 'vid', s + '.png') for s in stems] + [os.path.join('vis', 'vid', s + '.jpg') for s in stems]
    want += [os.path.join('masks', 'vid', 'visualization', m, s + '.jpg') for m in matte['vis_modes'] for s in stems]
    want += [os.path.join('masks', 'vid', 'alpha', s + '.png') for s in stems]
    want += [os.path.join('masks', 'vid', 'soft_masks', str(o), s + '.png') for o, ss in ((5, stems), (3, stems), (7, stems[2:])) for s in ss]
    want += [os.path.join('tracks', 'vid', n) for n in ('tracks.json', 'tracks_mot.txt')]
    assert sorted(files) == sorted(want)
    for rel, data in files.items():
        owner = runs[_family(rel)][1]
        assert rel in owner and data == owner[rel], rel
    assert a.tracks.json_text() == runs['tracks'][0].tracks.json_text() and len(a.tracks.frames) == 3
    assert a.regions['frames'] == 3 and a.regions['islands_removed'] > 0
    for name, (saver, _) in runs.items():
        assert saver.regions == a.regions, name
    # the scorer saw the plane of the file
    for saver in (a, runs['tracks'][0]):
        assert [n for n, _ in saver.scores] == NAMES
        for n, plane in saver.scores:
            assert np.array_equal(plane, np.array(Image.open(tmp_path / 'A' / 'masks' / 'vid' / (n[:-4] + '.png')))), n
