"""The polygon trace on the CPU: the model (tests/polygon_ref.py) against things it shares no code with -- the crack-parity fill, the
pixel count, scipy's component counts of the object and of its complement --, the product's host tracer and the list conventions against
the model, the writer of polygons.json against expected text, every ValueError of OpList.polygon_trace, and the wiring of ResultSaver,
eval_vos and process_video on every path through the descriptor interpreter (tests/mock_exec_polygons.py), every report checked against
the model's reading of the PNG that was written for the frame."""
import json
import logging
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.utils.polygons import PolygonReport, ring_area2, trace_rings

import polygon_ref as R
from test_edt_cpu import THR, _args, _frames, _pngs, _saver, _tree

HERE = os.path.dirname(os.path.abspath(__file__))
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
EIGHT = np.ones((3, 3), dtype=int)


def corpus():
    """random planes from 1 x 1 to 24 x 24 with 1 .. 4 ids at densities 0.2 / 0.5 / 0.8"""
    rng = np.random.default_rng(2024)
    for k in range(90):
        H, W = (int(v) for v in rng.integers(1, 25, 2)) if k >= 6 else ((1, 1), (1, 2), (2, 1), (2, 2), (1, 24), (24, 1))[k]
        ids = 1 + k % 4
        density = (0.2, 0.5, 0.8)[k % 3]
        yield (rng.integers(1, ids + 1, size=(H, W)) * (rng.random((H, W)) < density)).astype(np.uint8), list(range(1, ids + 1))


CORPUS = list(corpus())


def unpack(verts):
    return [(int(p) & 0xffff, int(p) >> 16) for p in verts]


@pytest.mark.parametrize('conn', [4, 8])
def test_the_model_against_what_it_shares_no_code_with(conn):
    for plane, objs in CORPUS:
        H, W = plane.shape
        rings, verts, table, E = R.trace(plane, objs, conn)
        filled = R.fill(rings, verts, H, W)
        assert E == int(rings[:, 3].sum()) and len(verts) == int(rings[:, 2].sum())
        for k, v in enumerate(objs):
            F = plane == v
            mine = rings[table[k, 0]:table[k, 0] + table[k, 1]]
            assert (mine[:, 0] == k).all() and table[k, 2] == (mine[0, 1] if len(mine) else table[k, 2])
            assert np.array_equal(filled.get(k, np.zeros((H, W), dtype=bool)), F)                    # the rings fill back to the object
            outer = holes = area2 = 0
            firsts = []
            for _, v0, nv, L in mine.tolist():
                pts = unpack(verts[v0:v0 + nv])
                a2 = R.shoelace2(pts)
                area2 += a2
                assert nv >= 4 and nv % 2 == 0 and pts[0] == min(pts, key=lambda p: (p[1], p[0]))     # the first vertex: the smallest (y, x)
                steps = [(pts[(q + 1) % nv][0] - x, pts[(q + 1) % nv][1] - y) for q, (x, y) in enumerate(pts)]
                assert all((dx == 0) != (dy == 0) for dx, dy in steps)                               # one coordinate changes
                assert all((steps[q][0] == 0) != (steps[q - 1][0] == 0) for q in range(nv))          # horizontal and vertical alternate: no collinear point
                assert L == sum(abs(dx) + abs(dy) for dx, dy in steps)                               # the Manhattan length
                vertical_first = steps[0][0] == 0
                assert vertical_first == (a2 < 0)                                                    # a hole iff its first edge is vertical
                holes += a2 < 0
                outer += a2 > 0
                firsts.append((pts[0][1], pts[0][0], 1 if vertical_first else 0))
            assert firsts == sorted(firsts)                                                          # rings in the order of their first edge
            assert area2 == 2 * int(F.sum())                                                         # signed areas add up to the pixel count
            assert outer == ndimage.label(F, structure=EIGHT if conn == 8 else FOUR)[1]
            dual = ndimage.label(np.pad(~F, 1, constant_values=True), structure=FOUR if conn == 8 else EIGHT)[1]
            assert holes == dual - 1


def test_saddles_and_bounds():
    for diag in ([[1, 0], [0, 1]], [[0, 1], [1, 0]]):
        plane = np.array(diag, dtype=np.uint8)
        assert R.trace(plane, [1], 8)[0][:, 2:].tolist() == [[8, 8]]
        assert R.trace(plane, [1], 4)[0][:, 2:].tolist() == [[4, 4], [4, 4]]
    board = ((np.add.outer(np.arange(8), np.arange(8)) % 2) + 1).astype(np.uint8)
    for conn in (4, 8):
        rings, verts, _, E = R.trace(board, [1, 2], conn)
        nbytes, edges = O.OpList.polygon_capacity(8, 8)
        assert len(verts) <= 4 * 81 and 4 * len(rings) <= len(verts) and 16 * len(rings) + 4 * len(verts) <= nbytes and E <= edges
        assert E == edges - 2 * (8 + 8)                                     # every inner crack in both directions, the frame's border in one


def test_the_host_tracer_equals_the_model():
    for plane, objs in CORPUS:
        for conn in (4, 8):
            want = R.trace(plane, objs, conn)
            got = trace_rings(plane, objs, conn)
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want[:3])), (plane.tolist(), conn)


def test_list_conventions():
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 7, size=(12, 17)).astype(np.uint8)
    objs = [2, 0, 300, 2, 9, -1, 5, 1]                                      # entries outside 1 .. 255, a repeat, an id without a pixel; 3, 4, 6 unlisted
    for conn in (4, 8):
        for trace in (lambda: R.trace(plane, objs, conn)[:3], lambda: trace_rings(plane, objs, conn)):
            rings, verts, table = trace()
            assert set(rings[:, 0].tolist()) == {0, 6, 7}
            assert table[:, 1].tolist()[1:6] == [0] * 5 and table[:, 3].tolist()[1:6] == [0] * 5
            assert (table[1:6, 0] == table[0, 1]).all() and (table[1:6, 2] == table[0, 3]).all()      # absent and empty rows: the running offsets
            assert np.array_equal(rings[:, 2:], np.concatenate([R.trace(plane, [v], conn)[0] for v in (2, 5, 1)])[:, 2:])      # each object alone
            filled = R.fill(rings, verts, *plane.shape)
            assert sorted(filled) == [0, 6, 7] and all(np.array_equal(filled[k], plane == v) for k, v in ((0, 2), (6, 5), (7, 1)))
        rings, verts, table = trace_rings(plane, [], conn)
        assert rings.shape == (0, 4) and verts.shape == (0,) and table.shape == (0, 4)
        words, table, status = R.stage(plane, [], conn, 1, 0)
        assert words is None and status.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        trace_rings(plane, [1], 6)
    with pytest.raises(ValueError):
        trace_rings(plane.astype(np.int32), [1], 8)


def test_the_writer(tmp_path):
    plane = np.array([[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 1, 2], [0, 0, 0, 0]], dtype=np.uint8)
    report = PolygonReport('clip', connectivity=8)
    report.add('00000', 1, *trace_rings(plane, [1, 2, 7], 8), [1, 2, 7], 4, 4)
    report.add('00001', 2, *trace_rings(np.zeros((4, 4), dtype=np.uint8), [1, 2], 8), [1, 2], 4, 4)
    report.add('00002', 3, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 4)), [], 4, 4)
    path = report.write(str(tmp_path / 'out' / 'clip'))
    assert path == str(tmp_path / 'out' / 'clip' / 'polygons.json')
    want = ('{"video": "clip", "height": 4, "width": 4, "connectivity": 8, "objects": [1, 2, 7], "frames": ['
            '{"frame": "00000", "index": 1, "objects": {'
            '"1": {"area": 8, "rings": [{"hole": false, "area": 9, "perimeter": 12, "points": [0, 0, 3, 0, 3, 3, 0, 3]}, '
            '{"hole": true, "area": 1, "perimeter": 4, "points": [1, 1, 1, 2, 2, 2, 2, 1]}]}, '
            '"2": {"area": 1, "rings": [{"hole": false, "area": 1, "perimeter": 4, "points": [3, 2, 4, 2, 4, 3, 3, 3]}]}, '
            '"7": {"area": 0, "rings": []}}}, '
            '{"frame": "00001", "index": 2, "objects": {"1": {"area": 0, "rings": []}, "2": {"area": 0, "rings": []}}}, '
            '{"frame": "00002", "index": 3, "objects": {}}]}')
    assert open(path).read() == want
    assert ring_area2([(0, 0), (3, 0), (3, 3), (0, 3)]) == 18
    with pytest.raises(ValueError):
        report.add('00003', 4, np.zeros((0, 4)), np.zeros(0), np.zeros((0, 4)), [], 5, 4)


def test_polygon_trace_descriptor_and_argument_checks():
    H, W, n, C = 9, 14, 3, 200
    need = O.OpList.polygon_scratch_words(H, W, n, C)
    assert need == 64 + 4 + 152 + 14 * 200 + 512 + 512 and O.OpList.polygon_capacity(H, W) == (32 * 150, 2 * (9 * 15 + 10 * 14))
    ids = torch.zeros((H, W), dtype=torch.uint8)
    good = dict(stream=torch.zeros(256, dtype=torch.int32), table=torch.zeros(n * 4, dtype=torch.int32), status=torch.zeros(4, dtype=torch.int32),
                scratch=torch.zeros(need, dtype=torch.int32))
    call = lambda ids=ids, objs=(1, 2, 3), edge_capacity=C, **kw: O.OpList().polygon_trace(
        ids, objs, *[kw.pop(k, good[k]) for k in ('stream', 'table', 'status', 'scratch')], edge_capacity=edge_capacity, **kw)
    ol = O.OpList()
    ol.polygon_trace(ids, [1, 2, 3], good['stream'], good['table'], good['status'], good['scratch'], connectivity=4, edge_capacity=C, path=1)
    kind, flags, ints, _, ptrs = ol.recs[0][:5]
    objs = [t for t in ol.keep if torch.is_tensor(t) and t.dtype == torch.int32 and t.tolist() == [1, 2, 3]][0]      # the list, uploaded and kept
    assert (kind, flags) == (O.PROB_TO_ID, 8192) and list(ints[:10]) == [0, H, W, C, 1024, 4, 1, 0, need, n]
    assert list(ptrs[:8]) == [0, 0, ids.data_ptr(), good['stream'].data_ptr(), good['status'].data_ptr(), good['scratch'].data_ptr(), objs.data_ptr(),
                              good['table'].data_ptr()]
    ol = O.OpList()
    ol.polygon_trace(ids, [], good['stream'].view(torch.uint8), torch.zeros(0, dtype=torch.int32), good['status'], good['scratch'], edge_capacity=C)
    assert ol.recs[0][4][6] == 0 and ol.recs[0][4][7] == 0 and ol.recs[0][2][5] == 8          # n == 0: no list, no table; 8 is the default
    odd = torch.zeros(need + 8, dtype=torch.int32)
    for change, msg in [(dict(ids=ids.to(torch.int32)), 'uint8'), (dict(ids=torch.zeros((H, W + 1), dtype=torch.uint8)[:, :W]), 'contiguous'),
                        (dict(ids=torch.zeros((0, 4), dtype=torch.uint8)), 'H, W >= 1'),
                        (dict(ids=torch.zeros((1, 65536), dtype=torch.uint8)), '65535'),
                        (dict(objs=list(range(256))), '256 objects'), (dict(objs=torch.zeros(3, dtype=torch.int64)), 'int32'),
                        (dict(connectivity=6), 'connectivity 6'), (dict(path=2), 'path 2'), (dict(edge_capacity=0), 'edge_capacity 0'),
                        (dict(stream=torch.zeros(16, dtype=torch.float32)), 'stream is'), (dict(stream=torch.zeros(18, dtype=torch.uint8)), '18 bytes'),
                        (dict(stream=good['stream'][1:]), 'stream is 16-byte aligned'),
                        (dict(table=torch.zeros(n * 4 + 4, dtype=torch.int32)), 'table is'), (dict(table=odd[1:1 + n * 4]), 'table is 16-byte aligned'),
                        (dict(status=torch.zeros(3, dtype=torch.int32)), 'status is'),
                        (dict(scratch=good['scratch'][:need - 1]), f'at least {need} words'), (dict(scratch=odd[1:1 + need]), 'scratch is 16-byte aligned'),
                        (dict(scratch=good['scratch'].to(torch.int64)), 'scratch is')]:
        with pytest.raises(ValueError, match=msg.replace('[', r'\[')):
            call(**change)
    with pytest.raises(ValueError, match='2\\^29'):
        O.OpList().polygon_trace(_Shaped(32768, 16384), [1], good['stream'], good['table'][:4], good['status'], good['scratch'], edge_capacity=C)


class _Shaped:
    """a stand-in for a uint8 plane too large to allocate: only what the checks in front of the buffers look at"""
    dtype = torch.uint8

    def __init__(self, H, W):
        self.shape = (H, W)

    def dim(self):
        return 2

    def is_contiguous(self):
        return True


def test_a_stale_library_is_named(monkeypatch):
    monkeypatch.setattr(_lib, '_executor', None)
    monkeypatch.setattr(_lib, 'has_polygons', lambda: False)
    with pytest.raises(_lib.HipLibraryError, match='8192'):
        O.OpList().polygon_trace(torch.zeros((2, 2), dtype=torch.uint8), [1], None, None, None, None, edge_capacity=4)


# ---- host wiring -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def executor():
    from mock_exec_polygons import PolygonMockExecutor
    ex = PolygonMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    yield ex
    _lib.set_executor_for_testing(None)


def check_report_against_masks(report, folder, conn, objects=None):
    """every frame of a report (a dict) against the model's reading of the PNG written for the frame -> the number of rings seen"""
    seen = 0
    assert list(report)[:6] == ['video', 'height', 'width', 'connectivity', 'objects', 'frames'] and report['connectivity'] == conn
    for frame in report['frames']:
        plane = np.array(Image.open(os.path.join(folder, frame['frame'] + '.png')))
        assert plane.shape == (report['height'], report['width'])
        objs = [int(k) for k in frame['objects']]
        if objects is not None:
            assert objs == objects
        rings, verts, table, _ = R.trace(plane, objs, conn)
        for k, oid in enumerate(objs):
            entry = frame['objects'][str(oid)]
            assert entry['area'] == int((plane == oid).sum())
            mine = rings[table[k, 0]:table[k, 0] + table[k, 1]]
            assert len(entry['rings']) == len(mine)
            for ring, (_, v0, nv, L) in zip(entry['rings'], mine.tolist()):
                pts = unpack(verts[v0:v0 + nv])
                assert ring['points'] == [c for p in pts for c in p] and ring['perimeter'] == L
                assert ring['area'] == abs(R.shoelace2(pts)) // 2 and ring['hole'] == (R.shoelace2(pts) < 0)
                seen += 1
    return seen


NAMES = [f'{t:05d}.png' for t in range(3)]


@pytest.mark.parametrize('egress', ['host', 'device'])
@pytest.mark.parametrize('resize', [False, True])
@pytest.mark.parametrize('filtered', [False, True])
def test_saver_reports_the_written_masks(tmp_path, executor, egress, resize, filtered):
    probs = _frames()
    shape = (37, 61) if resize else None
    extra = THR if filtered else {}
    runs = {}
    for name, kw in (('plain', {}), ('poly', dict(polygons=PolygonReport()))):
        saver = _saver(str(tmp_path / name), egress=egress, **extra, **kw)
        for t, p in enumerate(probs):
            saver.process(p, f'{t:05d}.jpg', resize_needed=resize, shape=shape)
        saver.end()
        runs[name] = _tree(str(tmp_path / name))
        if name == 'plain':
            assert executor.polygon_calls == [] and sorted(runs[name]) == ['vid/' + f for f in NAMES]   # off: no launch, no file
    assert {f: b for f, b in runs['poly'].items() if f != 'polygons/vid/polygons.json'} == runs['plain']   # the masks are the same bytes
    report = json.loads(runs['poly']['polygons/vid/polygons.json'])
    conn = 4 if filtered else 8
    assert report == saver.polygons.as_dict() and report['video'] == 'vid' and report['objects'] == [5, 3]
    assert [f['index'] for f in report['frames']] == [1, 2, 3] and [f['frame'] for f in report['frames']] == ['00000', '00001', '00002']
    assert check_report_against_masks(report, str(tmp_path / 'poly' / 'vid'), conn, objects=[5, 3]) > 6
    H, W = shape or (24, 40)
    assert [c[:5] for c in executor.polygon_calls] == [(H, W, 2, conn, 0)] * 3 and all(c[5][1] == 0 for c in executor.polygon_calls)
    if filtered:                                 # the filtered plane is traced: no outer ring below min_region pixels (4-connected)
        assert all(r['hole'] or r['area'] >= 4 for f in report['frames'] for o in f['objects'].values() for r in o['rings'])


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_merged_and_tracks_agree(tmp_path, executor, egress):
    from cutie_amd.inference.utils.track_report import TrackReport
    from test_track_report_cpu import softmax_planes
    rng = np.random.default_rng(2)
    frames = [[torch.from_numpy(softmax_planes(rng, 3, 6, 10).repeat(k, 1).repeat(k, 2)) for k in (3, 4)] for _ in range(2)]
    saver = _saver(str(tmp_path / 'm'), egress=egress, polygons=PolygonReport(), tracks=TrackReport('vid'), polygons_output_root=str(tmp_path / 'elsewhere'))
    for t, members in enumerate(frames):
        saver.process_merged(members, f'{t:05d}.jpg', (31, 47), frame_index=t + 5)
    saver.end()
    report = json.load(open(tmp_path / 'elsewhere' / 'vid' / 'polygons.json'))
    assert [f['index'] for f in report['frames']] == [5, 6]
    assert check_report_against_masks(report, str(tmp_path / 'm' / 'vid'), 8) >= 2
    tracks = saver.tracks.as_dict()
    assert [f['frame'] for f in tracks['frames']] == [f['frame'] for f in report['frames']]
    for ft, fp in zip(tracks['frames'], report['frames']):                  # both reports agree on every area
        assert {k: e['area'] for k, e in ft['objects'].items()} == {k: e['area'] for k, e in fp['objects'].items()}


def test_overflow_falls_back_to_the_host_tracer(tmp_path, executor, monkeypatch, caplog):
    from cutie_amd.inference.utils import results_utils as RU
    probs = _frames()
    want = _saver(str(tmp_path / 'want'), polygons=PolygonReport())
    for t, p in enumerate(probs):
        want.process(p, f'{t:05d}.jpg')
    want.end()
    for egress, name, value, bit in (('host', 'POLY_EDGES', 16, 2), ('device', 'POLY_STREAM', 64, 1), ('host', 'POLY_STREAM', 64, 1)):
        executor.polygon_calls.clear()
        monkeypatch.setattr(RU, name, value)
        out = str(tmp_path / f'{egress}_{name}')
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            saver = _saver(out, egress=egress, polygons=PolygonReport())
            for t, p in enumerate(probs):
                saver.process(p, f'{t:05d}.jpg')
            saver.end()
        assert [c[5][1] for c in executor.polygon_calls] == [bit] * 3           # every frame overflowed
        assert len([r for r in caplog.records if 'polygon trace' in r.getMessage()]) == 1     # one warning per saver
        assert saver.polygons.as_dict() == want.polygons.as_dict()
        monkeypatch.undo()


def test_a_long_stream_is_fetched_behind_the_head(tmp_path, executor, monkeypatch):
    from cutie_amd.inference.utils import results_utils as RU
    from cutie_amd.inference.utils.saver_buffers import POLY_TABLE
    probs = _frames()
    want = _saver(str(tmp_path / 'want'), polygons=PolygonReport())
    monkeypatch.setattr(RU, 'POLY_HEAD', 16 + POLY_TABLE + 32)                 # the pinned head ends inside the rings
    got = _saver(str(tmp_path / 'got'), polygons=PolygonReport())
    for t, p in enumerate(probs):
        want.process(p, f'{t:05d}.jpg')
        got.process(p, f'{t:05d}.jpg')
    want.end()
    got.end()
    assert got.polygons.as_dict() == want.polygons.as_dict() and all(c[5][0] > 32 for c in executor.polygon_calls)


def test_saver_refusals_and_a_frame_without_objects(tmp_path, executor):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    with pytest.raises(ValueError, match='use_long_id'):
        ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, processor=object(), polygons=PolygonReport())
    with pytest.raises(ValueError, match='processor'):
        ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, polygons=PolygonReport())
    with pytest.raises(ValueError, match='4 or 8'):
        _saver(str(tmp_path / 'c'), polygons=PolygonReport(), region_connectivity=6)
    saver = _saver(str(tmp_path / 'none'), objects=(), polygons=PolygonReport('named'))
    saver.process(torch.ones((1, 8, 9)), '00000.jpg')
    saver.end()
    assert executor.polygon_calls == []
    assert json.load(open(tmp_path / 'none' / 'polygons' / 'vid' / 'polygons.json')) == {
        'video': 'named', 'height': 8, 'width': 9, 'connectivity': 8, 'objects': [], 'frames': [{'frame': '00000', 'index': 1, 'objects': {}}]}


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
def test_the_switches_and_their_rules(tmp_path, capsys):
    base = ['--images', 'a', '--masks', 'b', '--output', 'c']
    assert _args(base).polygons is False and _args(base + ['--polygons']).polygons is True
    rgb = tmp_path / 'long' / 'v'
    os.makedirs(rgb)
    Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(rgb / '00000.png')
    with pytest.raises(SystemExit) as e:
        _args(['--images', 'a', '--masks', str(tmp_path / 'long'), '--output', 'c', '--polygons'])
    assert e.value.code == 2 and 'long-id' in capsys.readouterr().err
    from cutie_amd import process_video as PV
    assert PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c', '--polygons']).polygons is True
    assert PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c']).polygons is False


@pytest.fixture(scope='module')
def bike_dataset(tmp_path_factory):
    """the tests/golden/bike frames as two videos of one dataset, and as a dataset of one video"""
    root = str(tmp_path_factory.mktemp('polygons'))
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


def test_eval_vos_and_process_video_on_the_bike_example(bike_dataset):
    """eval_vos --polygons on the bike example (run at --size 48), alone and with --lockstep 2: the reports are the same, every frame is the
    model's reading of the PNG written for it, the PNGs are those of the run without the switch, which issues no launch; process_video too."""
    from mock_exec_polygons import PolygonMockExecutor
    from cutie_amd import eval_vos as E
    from cutie_amd import process_video as PV
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    ex = PolygonMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    try:
        net = CUTIE(default_config())
        net.load_weights(make_state_dict(seed=0))
        root, one = bike_dataset, os.path.join(bike_dataset, 'one')
        common = lambda base, out: ['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out, '--size', '48']
        plain_out = os.path.join(root, 'out_plain')
        E.run_dataset(net, default_config(), _args(common(one, plain_out)))
        assert ex.polygon_calls == [] and not os.path.exists(os.path.join(plain_out, 'polygons'))       # off: no launch, no file
        plain = _tree(os.path.join(plain_out, 'Annotations', 'bikeA'))
        reports = {}
        for name, base, extra in (('alone', one, []), ('lockstep', root, ['--lockstep', '2']), ('four', one, ['--region-connectivity', '4'])):
            out = os.path.join(root, 'out_' + name)
            res = E.run_dataset(net, default_config(), _args(common(base, out) + ['--polygons'] + extra))
            assert all(r['frames'] == 3 for r in res.values())
            for r in res.values():
                video = r['polygons']['video']
                on_disk = json.load(open(os.path.join(out, 'polygons', video, 'polygons.json')))
                assert on_disk == r['polygons'] and _tree(os.path.join(out, 'Annotations', video)) == plain
                assert check_report_against_masks(on_disk, os.path.join(out, 'Annotations', video), 4 if name == 'four' else 8) >= 3
                reports[name, video] = dict(on_disk, video=None)
        assert sorted(reports) == [('alone', 'bikeA'), ('four', 'bikeA'), ('lockstep', 'bikeA'), ('lockstep', 'bikeB')]
        assert reports['lockstep', 'bikeA'] == reports['alone', 'bikeA'] == reports['lockstep', 'bikeB']
        assert [f['index'] for f in reports['alone', 'bikeA']['frames']] == [1, 2, 3]
        assert all(c[:2] == (480, 854) and c[5][1] == 0 for c in ex.polygon_calls) and len(ex.polygon_calls) == 12
        frames, masks = os.path.join(one, 'JPEGImages', 'bikeA'), os.path.join(one, 'Annotations', 'bikeA')
        r = PV.process_video(net, PV.video_config(max_internal_size=48), frames, masks, os.path.join(root, 'pv'), polygons=True)
        on_disk = json.load(open(os.path.join(root, 'pv', 'polygons', 'polygons.json')))
        assert on_disk == r['polygons'] and [f['frame'] for f in on_disk['frames']] == [f'{t:07d}' for t in range(3)]
        assert check_report_against_masks(on_disk, os.path.join(root, 'pv'), 8) >= 3
    finally:
        _lib.set_executor_for_testing(None)
