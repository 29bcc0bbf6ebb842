"""The per-object track report on the CPU (PROB_TO_ID flags == 1024): the numpy model of the stage (tests/track_ref.py)
against independent arithmetic -- scipy.ndimage for area, box and centroid, a float64 restatement with np.argmax for the confidence --, its
conventions, the two writers (cutie_amd/inference/utils/track_report.py), OpList.track_stats, and the host wiring -- ResultSaver(tracks=...)
on every path and eval_vos --tracks -- through an executor that answers the stage with the model (tests/mock_exec_tracks.py).  Every report
is compared with what numpy reads from the PNG that was written for the frame: the report and the files cannot drift apart."""
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.utils.track_report import TrackReport, row_to_entry

import track_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def u64(row, w):
    return (int(row[w]) & 0xffffffff) | ((int(row[w + 1]) & 0xffffffff) << 32)


def blobs(rng, H, W, ids, cell=5):
    low = rng.choice(ids, size=(-(-H // cell), -(-W // cell)))
    return low.astype(np.uint8).repeat(cell, 0).repeat(cell, 1)[:H, :W]


def softmax_planes(rng, P, h, w, sharp=4.0):
    z = rng.standard_normal((P, h, w)).astype(np.float32) * np.float32(sharp)
    e = np.exp(z - z.max(0))
    return (e / e.sum(0)).astype(np.float32)


# ---- the model against independent arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,n', [(1, 1, 1), (7, 5, 2), (33, 70, 5), (64, 64, 9), (65, 129, 3), (120, 213, 40)])
def test_model_geometry_equals_scipy(H, W, n):
    rng = np.random.default_rng(H * 1000 + W)
    listed = [int(v) for v in rng.choice(np.arange(1, 256), size=n, replace=False)]
    for kind in ('blobs', 'noise'):
        pool = [0, 0] + listed + [7 if 7 not in listed else 8]
        ids = blobs(rng, H, W, pool) if kind == 'blobs' else rng.choice(pool, size=(H, W)).astype(np.uint8)
        t = R.table(ids, listed)
        assert t.dtype == np.int32 and t.shape == (n, 12)
        area = ndimage.sum(np.ones_like(ids, dtype=np.float64), ids, index=listed)
        boxes = ndimage.find_objects(ids.astype(np.int32), max_label=255)
        for k, oid in enumerate(listed):
            assert int(t[k, 0]) == int(area[k]), (kind, oid)
            e = row_to_entry(t[k])
            if int(area[k]) == 0:
                assert t[k].tolist() == [0, W, H, -1, -1] + [0] * 7 and e == {'area': 0, 'bbox': None, 'centroid': None, 'confidence': None}
                continue
            ys, xs = boxes[oid - 1]
            assert t[k, 1:5].tolist() == [xs.start, ys.start, xs.stop - 1, ys.stop - 1], (kind, oid)
            assert e['bbox'] == [xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start]
            cy, cx = ndimage.center_of_mass(np.ones_like(ids, dtype=np.float64), ids, oid)
            assert abs(e['centroid'][0] - cx) <= 1e-9 * max(1.0, cx) and abs(e['centroid'][1] - cy) <= 1e-9 * max(1.0, cy), (kind, oid)
            assert t[k, 9:].tolist() == [0, 0, 0] and e['confidence'] is None


@pytest.mark.parametrize('P,h,w', [(2, 30, 54), (4, 30, 54), (8, 17, 23), (3, 1, 1)])
def test_model_confidence_equals_a_float64_restatement(P, h, w):
    rng = np.random.default_rng(P * 100 + h)
    prob = softmax_planes(rng, P, h, w)
    lut = [0] + [int(v) for v in rng.choice(np.arange(1, 256), size=P - 1, replace=False)]
    listed = lut[1:][::-1]
    ids = np.zeros((4, 4), dtype=np.uint8)
    t = R.table(ids, listed, prob, lut)
    arg = np.argmax(prob, axis=0)                                            # the first maximum, like the stage (no NaN here)
    top = np.take_along_axis(prob, arg[None], 0)[0].astype(np.float64)
    for k, oid in enumerate(listed):
        won = arg == lut.index(oid)
        assert int(t[k, 9]) == int(won.sum())
        got = u64(t[k], 10)
        # q16 rounds v * 65535 to the nearest integer through two float32 roundings: within 0.5 + 2^-8 of the float64 product per sample
        assert abs(got - float((top[won] * 65535.0).sum())) <= (0.5 + 2.0 ** -8) * max(1, int(won.sum()))
        if won.any():
            assert abs(row_to_entry([1] + t[k, 1:].tolist())['confidence'] - top[won].mean()) <= 1e-5      # (an entry needs a pixel: area 1)
    assert all(int(t[k, 0]) == 0 for k in range(len(listed)))               # the id plane is background: the confidence does not need a pixel


def test_q16():
    v = np.array([np.nan, -1.0, -0.0, 0.0, 1e-9, 0.5 / 65535, 0.25, 0.5, 0.999999, 1.0, 1.5, np.inf, -np.inf], dtype=np.float32)
    want = [0, 0, 0, 0, 0, int(np.float32(np.float32(0.5 / 65535) * np.float32(65535)) + np.float32(0.5)), 16384, 32768, 65535, 65535, 65535, 65535, 0]
    assert R.q16(v).tolist() == want
    assert R.q16(np.float32(0.25)).tolist() == 16384


# ---- conventions -----------------------------------------------------------------------------------------------------------------------------
def test_conventions_of_the_object_list():
    rng = np.random.default_rng(3)
    ids = blobs(rng, 33, 70, [0, 1, 2, 9, 200, 255])
    listed = [2, 0, 300, 9, 2, 77, 255, -4, 9]                               # 1 and 200 are not listed; 77 has no pixel; 2 and 9 repeat
    t = R.table(ids, listed)
    empty = [0, 70, 33, -1, -1] + [0] * 7
    assert t[1].tolist() == t[2].tolist() == t[5].tolist() == t[7].tolist() == empty
    assert t[4].tolist() == t[0].tolist() and t[8].tolist() == t[3].tolist() and int(t[0, 0]) == int((ids == 2).sum()) > 0
    assert int(t[6, 0]) == int((ids == 255).sum()) > 0
    assert R.table(ids, []).shape == (0, 12)
    alone = R.table(ids, [9])                                                # a row does not depend on what else is listed
    assert alone[0].tolist() == t[3].tolist()


def test_conventions_of_the_confidence():
    h, w = 6, 9
    prob = np.full((3, h, w), 0.2, dtype=np.float32)
    prob[1, :, :4] = 0.7                                                     # plane 1 wins columns 0 .. 3
    prob[2, :, 4:] = 0.7                                                     # plane 2 wins the rest ...
    prob[1, 0, 8] = 0.7                                                      # ... but for an exact tie at (0, 8): the first plane wins
    prob[2, 1, 5] = np.nan                                                   # a NaN is never larger: plane 0 keeps (1, 5)
    prob[0, 2, 2] = np.nan                                                   # nothing is larger than a NaN in plane 0
    prob[1, 3, 0] = 1.5                                                      # above 1: counts 65535
    prob[:, 4, 4] = -0.5                                                     # all negative: plane 0 wins
    prob[:, 5, 8] = [-3.0, -2.0, -1.0]                                       # the largest is negative: plane 2 wins, q16 = 0
    lut = [0, 5, 3]
    ids = np.zeros((2, 2), dtype=np.uint8)
    t = R.table(ids, [3, 5, 0], prob, lut)
    q07 = int(R.q16(np.float32(0.7)))
    n5 = 4 * h - 1 + 1                                                       # columns 0 .. 3 without (2, 2), and the tie
    n3 = 5 * h - 1 - 1 - 1                                                   # columns 4 .. 8 without the tie, the NaN and (4, 4)
    assert t[1, 9] == n5 and u64(t[1], 10) == (n5 - 1) * q07 + 65535
    assert t[0, 9] == n3 and u64(t[0], 10) == (n3 - 1) * q07                 # (5, 8) counts as a sample and adds 0
    assert t[2].tolist() == [0, 2, 2, -1, -1] + [0] * 7                      # entry 0 is absent although plane 0 stands for id 0
    # the strided, un-padded view cut from a padded buffer: the same table
    pad = np.full((3, h + 5, w + 7), np.float32(9.0))
    pad[:, 2:2 + h, 3:3 + w] = prob
    view = pad[:, 2:2 + h, 3:3 + w]
    assert not view.flags['C_CONTIGUOUS'] and np.array_equal(R.table(ids, [3, 5, 0], view, lut), t, equal_nan=True)
    # no probabilities: words 9 .. 11 are 0
    assert R.table(ids, [3, 5, 0])[:, 9:].tolist() == [[0, 0, 0]] * 3
    # two planes of one object: both count for it
    both = R.table(ids, [5], prob, [0, 5, 5])
    assert both[0, 9] == n5 + n3 and u64(both[0], 10) == u64(t[0], 10) + u64(t[1], 10)


def test_the_sums_pass_32_bits():
    ids = np.ones((513, 4096), dtype=np.uint8)
    t = R.table(ids, [1])
    assert u64(t[0], 5) == 513 * 4096 * 4095 // 2 > 1 << 32 and u64(t[0], 7) == 4096 * 513 * 512 // 2
    assert t[0, :5].tolist() == [513 * 4096, 0, 0, 4095, 512]
    assert row_to_entry(t[0])['centroid'] == [2047.5, 256.0]


# ---- writers ---------------------------------------------------------------------------------------------------------------------------------
def _row(area, xmin, ymin, xmax, ymax, sx, sy, cnt=0, total=0):
    return [area, xmin, ymin, xmax, ymax, sx & 0xffffffff, sx >> 32, sy & 0xffffffff, sy >> 32, cnt, total & 0xffffffff, total >> 32]


EXPECTED_JSON = ('{"video": "clip", "height": 4, "width": 6, "objects": [2, 1], "frames": ['
                 '{"frame": "00003", "index": 4, "objects": {"2": {"area": 4, "bbox": [1, 0, 2, 2], "centroid": [1.5, 0.5], "confidence": 0.5}, '
                 '"1": {"area": 0, "bbox": null, "centroid": null, "confidence": null}}}, '
                 '{"frame": "00001", "index": 2, "objects": {"2": {"area": 3, "bbox": [0, 1, 2, 3], "centroid": [0.3333333333333333, 2.0], "confidence": null}, '
                 '"1": {"area": 1, "bbox": [5, 3, 1, 1], "centroid": [5.0, 3.0], "confidence": 1.0}}}, '
                 '{"frame": "00007", "index": 8, "objects": {}}]}\n')
EXPECTED_MOT = ('2,1,5,3,1,1,1.000000,-1,-1,-1\n'
                '2,2,0,1,2,3,-1,-1,-1,-1\n'
                '4,2,1,0,2,2,0.500000,-1,-1,-1\n')


def test_writers(tmp_path):
    rep = TrackReport('clip')
    rep.add('00003.jpg', 4, np.array([_row(4, 1, 0, 2, 1, 6, 2, 2, 65535), _row(0, 6, 4, -1, -1, 0, 0)], dtype=np.int64), [2, 1], 4, 6)
    rep.add('00001', 2, torch.tensor([_row(3, 0, 1, 1, 3, 1, 6), _row(1, 5, 3, 5, 3, 5, 3, 7, 7 * 65535)]), [2, 1], 4, 6)
    rep.add('00007.png', 8, np.zeros((0, 12), dtype=np.int32), [], 4, 6)
    rep.write(str(tmp_path / 'tracks' / 'clip'))
    assert open(tmp_path / 'tracks' / 'clip' / 'tracks.json').read() == EXPECTED_JSON
    assert open(tmp_path / 'tracks' / 'clip' / 'tracks_mot.txt').read() == EXPECTED_MOT
    back = json.loads(EXPECTED_JSON)
    assert list(back) == ['video', 'height', 'width', 'objects', 'frames'] and back == rep.as_dict()
    with pytest.raises(ValueError, match='4 x 7'):
        rep.add('00008', 9, np.zeros((0, 12)), [], 4, 7)
    with pytest.raises(ValueError, match='2 objects'):
        rep.add('00008', 9, np.zeros((1, 12)), [1, 2], 4, 6)
    big = row_to_entry(_row(513 * 4096, 0, 0, 4095, 512, 513 * 4096 * 4095 // 2, 4096 * 513 * 512 // 2, 3, 3 * 65535 - 1))
    assert big['centroid'] == [2047.5, 256.0] and big['confidence'] == (3 * 65535 - 1) / (65535 * 3)


# ---- the op --------------------------------------------------------------------------------------------------------------------------------
def test_track_stats_descriptor_and_argument_checks():
    from mock_exec_tracks import TracksMockExecutor
    _lib.set_executor_for_testing(TracksMockExecutor())
    try:
        assert O.OpList.TRACK_MAX_OBJECTS == 255
        ids = torch.zeros((5, 7), dtype=torch.uint8)
        table = torch.zeros((2, 12), dtype=torch.int32)
        buf = torch.zeros((3, 9, 16), dtype=torch.float32)
        prob = buf[:, 2:8, 3:12]
        lut = torch.tensor([0, 4, 6], dtype=torch.int32)
        ol = O.OpList()
        ol.track_stats(ids, [4, 6], table)
        ol.track_stats(ids, torch.tensor([4, 6], dtype=torch.int32), table, prob=prob, lut=lut)
        ol.track_stats(ids, [], torch.zeros((0, 12), dtype=torch.int32))
        arr = ol.finalize()
        assert arr['kind'].tolist() == [O.PROB_TO_ID] * 3 and arr['flags'].tolist() == [1024] * 3
        assert arr['i'][0, :10].tolist() == [0, 5, 7, 0, 0, 0, 0, 0, 0, 2] and arr['p'][0, 0] == 0 and arr['p'][0, 1] == 0
        assert arr['i'][1, :10].tolist() == [3, 5, 7, 144, 16, 6, 9, 0, 0, 2]
        assert arr['p'][1, 0] == prob.data_ptr() and arr['p'][1, 1] == lut.data_ptr() and arr['p'][1, 2] == ids.data_ptr() and arr['p'][1, 7] == table.data_ptr()
        assert arr['i'][2, 9] == 0 and arr['p'][2, 6] == 0 and arr['p'][2, 7] == 0
        for change, msg in ((dict(ids_plane=ids.int()), 'uint8'), (dict(ids_plane=torch.zeros((5, 8), dtype=torch.uint8)[:, :7]), 'contiguous'),
                            (dict(obj_ids=list(range(1, 257)), table=torch.zeros((256, 12), dtype=torch.int32)), '256 objects'),
                            (dict(table=torch.zeros((3, 12), dtype=torch.int32)), r'int32 \[2, 12\]'), (dict(table=table.long()), 'int32'),
                            (dict(prob=prob), 'come together'), (dict(lut=lut), 'come together'), (dict(prob=prob.double(), lut=lut), 'f32'),
                            (dict(prob=prob.permute(0, 2, 1), lut=lut), 'contiguous last'), (dict(prob=prob, lut=lut[:2]), r'int32 \[3\]'),
                            (dict(prob=torch.zeros((257, 2, 2)), lut=torch.zeros(257, dtype=torch.int32)), '257 probability planes'),
                            (dict(obj_ids=torch.tensor([4, 6])), 'int32')):
            with pytest.raises(ValueError, match=msg):
                O.OpList().track_stats(**dict(dict(ids_plane=ids, obj_ids=[4, 6], table=table), **change))
    finally:
        _lib.set_executor_for_testing(None)


# ---- host wiring -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tracks_executor():
    from mock_exec_tracks import TracksMockExecutor
    ex = TracksMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    yield ex
    _lib.set_executor_for_testing(None)


def geometry_of_png(png_path, obj_ids):
    """{str(id): (area, bbox, centroid)} of the file, by numpy alone"""
    ids = np.array(Image.open(png_path))
    out = {}
    for oid in obj_ids:
        ys, xs = np.nonzero(ids == oid)
        if len(xs) == 0:
            out[str(oid)] = (0, None, None)
        else:
            out[str(oid)] = (len(xs), [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)],
                             [float(xs.astype(np.float64).mean()), float(ys.astype(np.float64).mean())])
    return ids.shape, out


def check_report_against_files(report, mask_dir):
    """area, box and centroid of every reported frame = what numpy gets from the PNG that was written for it"""
    assert report['frames']
    for fr in report['frames']:
        shape, want = geometry_of_png(os.path.join(mask_dir, fr['frame'] + '.png'), [int(k) for k in fr['objects']])
        assert shape == (report['height'], report['width'])
        for key, e in fr['objects'].items():
            area, bbox, cen = want[key]
            assert (e['area'], e['bbox']) == (area, bbox), (fr['frame'], key)
            if area:
                assert abs(e['centroid'][0] - cen[0]) <= 1e-9 * max(1.0, cen[0]) and abs(e['centroid'][1] - cen[1]) <= 1e-9 * max(1.0, cen[1])
            else:
                assert e['centroid'] is None and e['confidence'] is None


def _saver(out, tracks, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    om.add_new_objects([5, 3])

    def to_mask(prob, dtype=torch.int64):
        return torch.tensor([0, 5, 3])[prob.argmax(0)].to(dtype)
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om, output_prob_to_mask=to_mask)
    return ResultSaver(out, 'vid', dataset='generic', object_manager=om, use_long_id=False, processor=proc, tracks=tracks, **kw)


def _frames(T=3, P=3, h=24, w=40):
    rng = np.random.default_rng(11)
    out = []
    for t in range(T):
        buf = torch.full((P, h + 3, w + 8), 7.0)
        buf[:, 1:1 + h, 2:2 + w] = torch.from_numpy(softmax_planes(rng, P, h // 4, w // 4).repeat(4, 1).repeat(4, 2))
        out.append(buf[:, 1:1 + h, 2:2 + w])                                 # the un-padded view of a padded buffer, as `step` returns it
    return out


@pytest.mark.parametrize('egress', ['host', 'device'])
@pytest.mark.parametrize('resize', [False, True])
def test_saver_reports_what_it_writes(tmp_path, tracks_executor, egress, resize):
    out = str(tmp_path / 'masks')
    rep = TrackReport()
    saver = _saver(out, rep, egress=egress, tracks_output_root=str(tmp_path / 'tracks'))
    assert saver.egress == egress
    probs = _frames()
    shape = (37, 61) if resize else None
    for t, p in enumerate(probs):
        saver.process(p, f'{t:05d}.jpg', resize_needed=resize, shape=shape, **({'frame_index': 10 * t + 1} if t else {}))
    saver.end()
    H, W = shape or (24, 40)
    assert tracks_executor.track_calls == [(H, W, 2, True)] * 3
    got = json.load(open(tmp_path / 'tracks' / 'vid' / 'tracks.json'))
    assert got == rep.as_dict() and got['video'] == 'vid' and (got['height'], got['width']) == (H, W) and got['objects'] == [5, 3]
    assert [(f['frame'], f['index']) for f in got['frames']] == [('00000', 1), ('00001', 11), ('00002', 21)]     # the running count, then what was passed
    check_report_against_files(got, os.path.join(out, 'vid'))
    for t, fr in enumerate(got['frames']):                                   # the confidence: the model on the probabilities at the MODEL's resolution
        want = R.table(np.zeros((1, 1), dtype=np.uint8), [5, 3], probs[t].numpy(), [0, 5, 3])
        for k, oid in enumerate((5, 3)):
            e = fr['objects'][str(oid)]
            conf = u64(want[k], 10) / (65535 * int(want[k, 9]))
            assert int(want[k, 9]) > 0 and e['area'] > 0 and e['confidence'] == conf
    assert sum(len(l.split(',')) == 10 for l in open(tmp_path / 'tracks' / 'vid' / 'tracks_mot.txt')) == sum(e['area'] > 0 for f in got['frames'] for e in f['objects'].values())


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_merged_reports_geometry_and_no_confidence(tmp_path, tracks_executor, egress):
    out = str(tmp_path / 'masks')
    rep = TrackReport()
    saver = _saver(out, rep, egress=egress)
    rng = np.random.default_rng(2)
    for t in range(2):
        members = [torch.from_numpy(softmax_planes(rng, 3, 6, 10).repeat(k, 1).repeat(k, 2)) for k in (3, 4)]
        saver.process_merged(members, f'{t:05d}.jpg', (31, 47))
    saver.end()
    assert tracks_executor.track_calls == [(31, 47, 2, False)] * 2
    got = json.load(open(os.path.join(out, 'tracks', 'vid', 'tracks.json')))           # the default root: <output_root>/tracks
    assert [f['index'] for f in got['frames']] == [1, 2]
    check_report_against_files(got, os.path.join(out, 'vid'))
    assert all(e['confidence'] is None for f in got['frames'] for e in f['objects'].values())
    assert any(e['area'] > 0 for f in got['frames'] for e in f['objects'].values())


def test_saver_refusals_and_defaults(tmp_path, tracks_executor):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    with pytest.raises(ValueError, match='use_long_id'):
        ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, processor=object(), tracks=TrackReport())
    with pytest.raises(ValueError, match='processor'):
        ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, tracks=TrackReport())
    saver = _saver(str(tmp_path / 'm'), None)                                # off by default: no launch, no folder
    saver.process(_frames(1)[0], '00000.jpg')
    saver.end()
    assert tracks_executor.track_calls == [] and not os.path.exists(tmp_path / 'm' / 'tracks')
    # a frame without objects is reported without rows and without a launch
    from cutie_amd.inference.utils.results_utils import ResultSaver as RS
    rep = TrackReport('e')
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om,
                                 output_prob_to_mask=lambda prob, dtype=torch.int64: torch.zeros(prob.shape[1:], dtype=dtype))
    s = RS(str(tmp_path / 'e'), 'e', dataset='generic', object_manager=om, use_long_id=False, processor=proc, tracks=rep)
    s.process(torch.ones((1, 4, 5)), '00000.jpg')
    s.end()
    assert tracks_executor.track_calls == [] and rep.as_dict()['frames'] == [{'frame': '00000', 'index': 1, 'objects': {}}]


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
def _args(argv):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(argv)
    E.check_args(ap, args)
    return args


def test_eval_vos_switch_and_its_rules(tmp_path, capsys):
    base = ['--images', 'a', '--masks', 'b', '--output', 'c']
    assert _args(base).tracks is False and _args(base + ['--tracks']).tracks is True
    rgb = tmp_path / 'long' / 'v'
    os.makedirs(rgb)
    Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(rgb / '00000.png')
    with pytest.raises(SystemExit) as e:
        _args(['--images', 'a', '--masks', str(tmp_path / 'long'), '--output', 'c', '--tracks'])
    assert e.value.code == 2 and 'long-id' in capsys.readouterr().err
    from cutie_amd import process_video as PV
    assert PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c', '--tracks']).tracks is True


@pytest.fixture(scope='module')
def bike_dataset(tmp_path_factory):
    """the tests/golden/bike frames as two videos of one dataset, and as a dataset of one video"""
    root = str(tmp_path_factory.mktemp('tracks'))
    src = os.path.join(HERE, 'golden', 'bike')
    for name in ('bikeA', 'bikeB'):
        img_dir, msk_dir = (os.path.join(root, d, name) for d in ('JPEGImages', 'Annotations'))
        os.makedirs(img_dir)
        os.makedirs(msk_dir)
        shutil.copy(os.path.join(src, '00000.png'), msk_dir)
        for t in range(3):
            shutil.copy(os.path.join(src, f'0000{t}.jpg'), img_dir)
    for d in ('JPEGImages', 'Annotations'):
        shutil.copytree(os.path.join(root, d, 'bikeA'), os.path.join(root, 'one', d, 'bikeA'))
    return root


def test_eval_vos_tracks_one_by_one_and_in_lock_step(bike_dataset):
    """eval_vos --tracks on the bike example (run at --size 48: the frames are resized on the way in, so the confidence is taken at the
    model's resolution and the geometry at the files'): the reports equal the files, and two copies of the clip in lock step report what
    the clip reports alone."""
    from mock_exec_tracks import TracksMockExecutor
    from cutie_amd import eval_vos as E
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    ex = TracksMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    try:
        net = CUTIE(default_config())
        net.load_weights(make_state_dict(seed=0))
        root, one = bike_dataset, os.path.join(bike_dataset, 'one')
        reports = {}
        for name, base, extra in (('alone', one, []), ('lockstep', root, ['--lockstep', '2'])):
            out = os.path.join(root, 'out_' + name)
            args = _args(['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out,
                          '--size', '48', '--tracks'] + extra)
            res = E.run_dataset(net, default_config(), args)
            for r in res.values():
                rep = r['tracks']
                assert r['frames'] == 3 and rep == json.load(open(os.path.join(out, 'tracks', rep['video'], 'tracks.json')))
                assert (rep['height'], rep['width']) == (480, 854) and rep['objects'] == [1, 2]
                assert [(f['frame'], f['index']) for f in rep['frames']] == [('00000', 1), ('00001', 2), ('00002', 3)]
                check_report_against_files(rep, os.path.join(out, 'Annotations', rep['video']))
                assert rep['frames'][0]['objects']['1']['area'] > 0 and rep['frames'][0]['objects']['1']['confidence'] is not None
                assert os.path.getsize(os.path.join(out, 'tracks', rep['video'], 'tracks_mot.txt')) > 0
                reports[name, rep['video']] = dict(rep, video='')
        assert all(with_prob and (H, W) == (480, 854) for H, W, n, with_prob in ex.track_calls) and len(ex.track_calls) == 9
        assert reports['alone', 'bikeA'] == reports['lockstep', 'bikeA'] == reports['lockstep', 'bikeB']
    finally:
        _lib.set_executor_for_testing(None)
