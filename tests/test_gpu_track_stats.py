"""The track statistics on the MI355X (PROB_TO_ID flags == 1024, csrc/tracks.hip) against the numpy model (tests/track_ref.py): the table
word for word -- over the shapes at which the kernels take another path (degenerate rows and columns, the tails of a wave, of a 16-byte load
and of a block, a plane that does not start on a 16-byte boundary, every LDS row in use, sums beyond 2^32), with the table pre-filled with
garbage between guard rows and the planes checked to be untouched; every refusal of the launcher; and end to end: eval_vos --tracks with
host egress, device egress, in lock step and multi-scale, against the PNGs those runs wrote and the probabilities `step` returned."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config

import track_ref as R
from test_track_report_cpu import blobs, check_report_against_files, softmax_planes, u64

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 1024
FILL = 0x7f7f7f7f


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device_table(ids, objects, prob=None, lut=None, offset=0):
    """the stage on one plane -> int32 [n, 12]; the table is pre-filled with 0x7f bytes and sits between guards; ``prob``: a tensor on the
    device (any view); ``offset``: bytes between a 16-byte boundary and the plane's first pixel"""
    H, W = ids.shape
    n = len(objects)
    buf = torch.full((GUARD + n * 12 + GUARD,), FILL, dtype=torch.int32, device='cuda')
    table = buf[GUARD:GUARD + n * 12].view(n, 12)
    room = torch.zeros(16 + H * W, dtype=torch.uint8, device='cuda')
    plane = room[offset:offset + H * W].view(H, W)
    plane.copy_(torch.from_numpy(np.ascontiguousarray(ids)))
    assert plane.data_ptr() % 16 == offset
    before = prob.clone() if prob is not None else None
    lut_dev = torch.tensor(lut, dtype=torch.int32).cuda() if lut is not None else None
    ol = O.OpList()
    ol.track_stats(plane, objects, table, prob=prob, lut=lut_dev)
    ol.run()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + n * 12:] == FILL).all())
    assert np.array_equal(plane.cpu().numpy(), ids)
    if prob is not None:
        assert torch.equal(prob.view(torch.int32), before.view(torch.int32))
    return table.cpu().numpy()


def _check(ids, objects, prob=None, lut=None, offset=0, what=''):
    got = _device_table(ids, objects, prob, lut, offset)
    want = R.table(ids, objects, prob.cpu().numpy() if prob is not None else None, lut)
    assert np.array_equal(got, want), (what, ids.shape, objects, got.tolist(), want.tolist())
    return want


LISTED = [3, 1, 2, 200, 255]


@pytest.mark.parametrize('H,W', [(1, 1), (1, 37), (37, 1), (7, 5), (64, 64), (65, 129)])
def test_kernel_equals_the_model(H, W):
    rng = np.random.default_rng(H * 131 + W)
    z = np.zeros((H, W), dtype=np.uint8)
    corners = z.copy()
    for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        corners[y, x] = LISTED[k]                                           # objects of one pixel, in each corner (one pixel: the last one wins)
    planes = [('blobs', blobs(rng, H, W, [0, 0, 1, 2, 3, 7, 200, 255])), ('noise', rng.choice([0, 1, 2, 3, 7, 200, 255], size=(H, W)).astype(np.uint8)),
              ('background', z), ('one object everywhere', z + 2), ('an unlisted object everywhere', z + 7), ('corners', corners),
              ('checkerboard', ((np.add.outer(np.arange(H), np.arange(W)) % 2) * 3).astype(np.uint8))]
    seen = 0
    for name, ids in planes:
        for offset in (0, 3):                                               # one 16-byte load per chunk | byte loads
            want = _check(ids, LISTED, offset=offset, what=name)
            seen += int(want[:, 0].sum())
        if name == 'one object everywhere':
            assert want[2].tolist()[:5] == [H * W, 0, 0, W - 1, H - 1]      # the box is the whole plane
    assert seen > 0


def test_every_lds_row_in_use():
    ids = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = _check(ids, list(range(1, 256)), what='ids 1 .. 255')
    assert want[:, 0].tolist() == [1] * 255
    _check(ids, list(range(255, 0, -1)), what='ids 255 .. 1')
    rng = np.random.default_rng(5)
    _check(rng.integers(0, 256, size=(65, 129)).astype(np.uint8), list(range(1, 256)), offset=5, what='noise of all ids')


def test_the_conventions_of_the_list():
    rng = np.random.default_rng(3)
    ids = blobs(rng, 33, 70, [0, 1, 2, 9, 200, 255])
    listed = [2, 0, 300, 9, 2, 77, 255, -4, 9]
    want = _check(ids, listed, what='listed, unlisted, duplicate, 0 and 300')
    assert want[4].tolist() == want[0].tolist() and want[8].tolist() == want[3].tolist() and want[1].tolist() == [0, 70, 33, -1, -1] + [0] * 7
    _check(ids, [9], what='one entry')
    _check(ids, [300], what='one absent entry')
    # n == 0: nothing is written, nothing is needed
    assert _device_table(ids, []).shape == (0, 12)
    ol = O.OpList()
    ol.add(O.PROB_TO_ID, 1024, [0, 33, 70, 0, 0, 0, 0, 0, 0, 0], [], [None, None, torch.from_numpy(ids).cuda(), None, None, None, None, None])
    ol.run()
    torch.cuda.synchronize()


def test_sums_beyond_32_bits():
    H, W = 513, 4096
    ids = np.ones((H, W), dtype=np.uint8)
    want = _check(ids, [1, 2], what='one object fills the plane')
    assert u64(want[0], 5) == H * W * (W - 1) // 2 > 1 << 32 and want[1].tolist()[:5] == [0, W, H, -1, -1]
    ids[:, W // 2:] = 2                                                     # the same plane split between two objects
    ids[200:300, 1000:3000] = 0
    want = _check(ids, [1, 2], what='split between two objects')
    hole = 100 * sum(range(1000, 3000))
    assert u64(want[0], 5) + u64(want[1], 5) + hole == H * W * (W - 1) // 2 and int(want[0, 0]) + int(want[1, 0]) == H * W - 100 * 2000


def test_a_480p_plane_with_three_blobs():
    H, W = 480, 854
    yy, xx = np.mgrid[:H, :W]
    ids = np.zeros((H, W), dtype=np.uint8)
    for oid, (cy, cx, ry, rx) in ((1, (120, 200, 80, 150)), (2, (300, 600, 150, 90)), (3, (400, 100, 60, 60))):
        ids[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = oid
    want = _check(ids, [1, 2, 3], what='three blobs')
    assert want[:, 0].min() > 1000
    a = _device_table(ids, [3, 2, 1])
    assert np.array_equal(a[::-1], want) and np.array_equal(_device_table(ids, [1, 2, 3]), want)      # the same launch again; another order


# ---- confidence -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [2, 4, 8])
def test_confidence_equals_the_model(P):
    h, w = 30, 54
    rng = np.random.default_rng(P)
    lut = [0] + [int(v) for v in rng.choice(np.arange(1, 256), size=P - 1, replace=False)]
    listed = lut[1:][::-1] + [lut[1], 0, 300]
    ids = blobs(rng, 37, 61, [0] + lut[1:])
    soft = softmax_planes(rng, P, h, w)
    cases = {'softmax': soft}
    tie = soft.copy()
    tie[1, :, ::3] = tie[0, :, ::3] = tie.max(0)[:, ::3]                    # planes 0 and 1 share the largest value: plane 0 wins
    if P > 2:
        tie[2, :, 1::3] = tie[1, :, 1::3] = tie.max(0)[:, 1::3] * np.float32(0.5) + np.float32(0.5)      # ... and two object planes: plane 1 wins
    cases['tie'] = tie
    odd = soft.copy()
    odd[P - 1, 3, 4] = np.nan
    odd[0, 5, 6] = np.nan
    odd[:, 7, 8] = -0.25
    odd[:, 9, 10] = np.linspace(-3, -1, P)
    odd[1, 11, 12] = 1.75
    odd[1, 13, :] = 1.0
    cases['nan, negative, above 1'] = odd
    back = np.zeros_like(soft)
    back[0] = 1.0
    cases['background only'] = back
    for name, prob in cases.items():
        want = _check(ids, listed, torch.from_numpy(prob).cuda(), lut, what=name)
        pad = torch.full((P, h + 3, w + 10), 9.0, device='cuda')
        pad[:, 2:2 + h, 7:7 + w] = torch.from_numpy(prob).cuda()
        view = pad[:, 2:2 + h, 7:7 + w]                                     # the strided view cut from a padded buffer
        assert not view.is_contiguous() and np.array_equal(_device_table(ids, listed, view, lut), want), name
        if name == 'background only':
            assert want[:, 9:].tolist() == [[0, 0, 0]] * len(listed)
        elif name == 'softmax':
            assert want[0, 9] > 0 and u64(want[0], 10) > 0
    none = _check(ids, listed, what='p0 == 0')
    assert none[:, 9:].tolist() == [[0, 0, 0]] * len(listed) and np.array_equal(none[:, :9], want[:, :9])
    # planes larger than one sweep of the grid, two planes of one object
    big = softmax_planes(rng, 3, 480, 854, sharp=1.0)
    _check(ids, [5, 6], torch.from_numpy(big).cuda(), [0, 5, 5], what='480 x 854, two planes of one object')


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_launcher():
    H, W, n = 37, 70, 3
    ids = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    objs = torch.arange(1, 257, dtype=torch.int32, device='cuda')
    table = torch.full((256, 12), -7, dtype=torch.int32, device='cuda')
    lut = torch.zeros(256, dtype=torch.int32, device='cuda')
    prob = torch.zeros((2, 30, 54), dtype=torch.float32, device='cuda')
    odd = torch.zeros(64, dtype=torch.int32, device='cuda')
    good = dict(flags=1024, P=2, H=H, W=W, plane=30 * 54, ldrow=54, h=30, w=54, n=n, p0=prob, p1=lut, ids=ids, objs=objs, table=table)
    cases = [(dict(flags=1024 | f), 'unknown flags') for f in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)]
    cases += [(dict(H=0), 'empty shape'), (dict(W=0), 'empty shape'), (dict(W=-3), 'empty shape'), (dict(H=1 << 16, W=1 << 15), 'exceeds 2^31 pixels'),
              (dict(n=-1), '-1 objects'), (dict(n=256), '256 objects'), (dict(P=0), '0 probability planes'), (dict(P=257), '257 probability planes'),
              (dict(h=0), 'empty probability planes'), (dict(h=1 << 16, w=1 << 15, ldrow=1 << 15), 'exceed 2^31 samples'), (dict(ldrow=53), 'row stride 53'),
              (dict(ids=None), 'the id plane (p2)'), (dict(p1=None), 'need the lut (p1)'), (dict(objs=None), 'the object ids (p6)'),
              (dict(table=None), 'the table (p7)'), (dict(table=odd[1:]), 'table 16-byte aligned'), (dict(objs=odd.view(torch.uint8)[1:]), 'object ids 4-byte aligned'),
              (dict(p0=odd.view(torch.uint8)[1:]), 'lut 4-byte aligned'), (dict(p1=odd.view(torch.uint8)[2:]), 'lut 4-byte aligned')]
    lib = _lib.load()
    assert _lib.has_track_stats() and lib.cutie_hip_abi_version() == 11
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [a['P'], a['H'], a['W'], a['plane'], a['ldrow'], a['h'], a['w'], 0, 0, a['n']], [],
               [a['p0'], a['p1'], a['ids'], None, None, None, a['objs'], a['table']])
        arr = ol.finalize()
        assert lib.cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in lib.cutie_hip_last_error().decode(), (change, lib.cutie_hip_last_error().decode())
    torch.cuda.synchronize()
    assert bool((table == -7).all())
    with pytest.raises(ValueError, match='256 objects'):
        O.OpList().track_stats(ids, list(range(256)), table)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    _lib.set_executor_for_testing(None)
    n = CUTIE(default_config()).cuda().eval()
    n.load_weights(S.decisive_state_dict())
    return n


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    """the tests/golden/bike frames as two videos of one dataset, and as a dataset of one video"""
    root = str(tmp_path_factory.mktemp('tracks'))
    src = os.path.join(HERE, 'golden', 'bike')
    for name in ('bikeA', 'bikeB'):
        img_dir, msk_dir = (os.path.join(root, d, name) for d in ('JPEGImages', 'Annotations'))
        os.makedirs(img_dir)
        os.makedirs(msk_dir)
        shutil.copy(os.path.join(src, '00000.png'), msk_dir)
        for t in range(4):
            shutil.copy(os.path.join(src, f'0000{t}.jpg'), img_dir)
    for d in ('JPEGImages', 'Annotations'):
        shutil.copytree(os.path.join(root, d, 'bikeA'), os.path.join(root, 'one', d, 'bikeA'))
    return root


def test_eval_vos_tracks_host_device_lockstep_multiscale(net, dataset, monkeypatch):
    from cutie_amd import eval_vos as E
    from cutie_amd.inference.utils.results_utils import ResultSaver
    seen = {}                                                               # (video, index) -> (prob as `step` returned it, lut) of the current run
    queue_tracks = ResultSaver._queue_tracks

    def recording(self, ids, all_ids, prob, lut_dev, frame_index):
        if prob is not None:
            lut = self._lut_device(int(prob.shape[0]), prob.device).cpu().tolist()
            seen[self.video_name, frame_index] = (prob.detach().float().cpu().numpy().copy(), lut)
        return queue_tracks(self, ids, all_ids, prob, lut_dev, frame_index)
    monkeypatch.setattr(ResultSaver, '_queue_tracks', recording)
    root, one = dataset, os.path.join(dataset, 'one')
    reports = {}
    for name, base, names, extra in (('host', one, ['bikeA'], []), ('device', one, ['bikeA'], ['--egress', 'device']),
                                     ('lockstep', root, ['bikeA', 'bikeB'], ['--egress', 'device', '--lockstep', '2']),
                                     ('sizes', one, ['bikeA'], ['--egress', 'device', '--sizes', '480', '600'])):
        seen.clear()
        out = os.path.join(root, 'out_' + name)
        ap = E.arg_parser()
        args = ap.parse_args(['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out,
                              '--dataset', 'd17-val', '--tracks'] + extra)
        E.check_args(ap, args)
        res = E.run_dataset(net, default_config(), args)
        assert sorted(r['tracks']['video'] for r in res.values()) == names
        for r in res.values():
            rep = r['tracks']
            video = rep['video']
            assert r['frames'] == 4 and rep == json.load(open(os.path.join(out, 'tracks', video, 'tracks.json')))
            assert (rep['height'], rep['width']) == (480, 854) and rep['objects'] == [1, 2]
            assert [(f['frame'], f['index']) for f in rep['frames']] == [(f'0000{t}', t + 1) for t in range(4)]
            check_report_against_files(rep, os.path.join(out, 'Annotations', video))       # geometry = numpy's reading of the written PNGs
            assert rep['frames'][0]['objects']['1']['area'] > 0
            for fr in rep['frames']:
                if name == 'sizes':                                         # S probability sources, no single model resolution
                    assert all(e['confidence'] is None for e in fr['objects'].values()) and not seen
                    continue
                prob, lut = seen[video, fr['index']]                         # confidence = the model on the probabilities `step` returned
                want = R.table(np.zeros((1, 1), dtype=np.uint8), rep['objects'], prob, lut)
                for k, oid in enumerate(rep['objects']):
                    e = fr['objects'][str(oid)]
                    conf = u64(want[k], 10) / (65535 * int(want[k, 9])) if int(want[k, 9]) else None
                    assert e['confidence'] == (conf if e['area'] > 0 else None), (name, video, fr['frame'], oid)
            mot = open(os.path.join(out, 'tracks', video, 'tracks_mot.txt')).read().splitlines()
            assert len(mot) == sum(e['area'] > 0 for f in rep['frames'] for e in f['objects'].values()) > 0
            reports[name, video] = dict(rep, video='')
    assert reports['device', 'bikeA'] == reports['lockstep', 'bikeA'] == reports['lockstep', 'bikeB']      # the clip alone and two copies side by side
    assert any(e['confidence'] is not None for f in reports['host', 'bikeA']['frames'] for e in f['objects'].values())
