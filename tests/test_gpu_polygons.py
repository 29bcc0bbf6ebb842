"""The polygon trace on the MI355X (PROB_TO_ID flags == 8192, csrc/polygons.hip) against the model (tests/polygon_ref.py): stream, object
table and status word for word, between guard words, the plane unchanged; every case with connectivity 4 and 8 and with i6 = 0 and 1, whose
outputs must be the same words -- over the smallest shapes and both saddles, holes and nesting, borders and the corner maximum, the list
conventions, planes at an aligned and a misaligned start, rings far longer than a workgroup, a frame-sized plane, both capacity errors,
every refusal of the launcher and the flag combinations; and end to end: eval_vos --polygons under host egress, device egress, lock step and
multi-scale, every frame's rings filled back to the PNG written next to them."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config

import polygon_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
FILL = 0x5a5a5a5a


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device(ids, obj_ids, conn, path, edge_capacity, stream_bytes, offset=0):
    """the stage on one plane -> (stream words uint32, table, status); every buffer sits between guards that must survive and the plane
    must come back unchanged; ``offset``: bytes between a 16-byte boundary and the plane's first pixel"""
    H, W = ids.shape
    n = len(obj_ids)
    room = torch.full((GUARD + 16 + H * W + GUARD,), 0xa5, dtype=torch.uint8, device='cuda')
    plane = room[GUARD + offset:GUARD + offset + H * W].view(H, W)
    plane.copy_(torch.from_numpy(np.ascontiguousarray(ids)))
    assert plane.data_ptr() % 16 == offset
    before = room.clone()
    words = O.OpList.polygon_scratch_words(H, W, n, edge_capacity)
    sw, tw = stream_bytes // 4, 4 * n
    sbuf = torch.full((GUARD + words + GUARD,), FILL, dtype=torch.int32, device='cuda')
    obuf = torch.full((GUARD + sw + GUARD,), FILL, dtype=torch.int32, device='cuda')
    tbuf = torch.full((GUARD + tw + GUARD,), FILL, dtype=torch.int32, device='cuda')
    ubuf = torch.full((GUARD + 4 + GUARD,), FILL, dtype=torch.int32, device='cuda')
    ol = O.OpList()
    ol.polygon_trace(plane, obj_ids, obuf[GUARD:GUARD + sw], tbuf[GUARD:GUARD + tw], ubuf[GUARD:GUARD + 4], sbuf[GUARD:GUARD + words],
                     connectivity=conn, edge_capacity=edge_capacity, path=path)
    ol.run()
    torch.cuda.synchronize()
    assert torch.equal(room, before)                                         # read only
    for buf, size in ((sbuf, words), (obuf, sw), (tbuf, tw), (ubuf, 4)):
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + size:] == FILL).all())
    return (obuf[GUARD:GUARD + sw].cpu().numpy().view(np.uint32), tbuf[GUARD:GUARD + tw].cpu().numpy().reshape(n, 4),
            ubuf[GUARD:GUARD + 4].cpu().numpy())


def _check(ids, obj_ids, what='', offsets=(0,), slack=3):
    """both connectivities, both paths, the capacities just large enough (the stream exactly) -> {conn: (rings, verts, table, E)}"""
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    out = {}
    for conn in (4, 8):
        rings, verts, table, E = R.trace(ids, obj_ids, conn)                 # once per case: every run below shares it
        nbytes = 16 * len(rings) + 4 * len(verts)
        want_s, want_t, want_u = R.stage(ids, obj_ids, conn, max(E, 1) + slack, nbytes)
        for offset in offsets:
            got = [_device(ids, obj_ids, conn, path, max(E, 1) + slack, nbytes, offset) for path in (0, 1)]
            for path, (s, t, u) in enumerate(got):
                tag = (what, ids.shape, conn, path, offset)
                assert u.tolist() == want_u.tolist(), (tag, u.tolist(), want_u.tolist())
                assert np.array_equal(t, want_t), (tag, t.tolist(), want_t.tolist())
                if want_s is not None:
                    assert np.array_equal(s, want_s), (tag, np.flatnonzero(s != want_s)[:8].tolist())
            for a, b in zip(got[0], got[1]):
                assert np.array_equal(a, b), (what, conn, offset, 'the two paths differ')
        out[conn] = (rings, verts, table, E)
    return out


def _plane(rows):
    return np.array(rows, dtype=np.uint8)


def noise(rng, H, W, density, ids=3):
    return (rng.integers(1, ids + 1, size=(H, W)) * (rng.random((H, W)) < density)).astype(np.uint8)


def spiral(H, W):
    """a one-pixel-wide spiral from the corner inwards, one pixel between its arms"""
    g = np.zeros((H, W), dtype=np.uint8)
    x = y = d = 0
    step = ((1, 0), (0, 1), (-1, 0), (0, -1))
    free = lambda x, y: 0 <= x < W and 0 <= y < H and not g[y, x]
    while True:
        g[y, x] = 1
        for turn in (0, 1):
            dx, dy = step[(d + turn) % 4]
            if free(x + dx, y + dy) and (not (0 <= x + 2 * dx < W and 0 <= y + 2 * dy < H) or not g[y + 2 * dy, x + 2 * dx]):
                d = (d + turn) % 4
                break
        else:
            return g
        x, y = x + dx, y + dy


def comb(H, W):
    g = np.zeros((H, W), dtype=np.uint8)
    g[:, ::2] = 1
    g[0, :] = 1
    return g


def test_smallest_shapes_and_saddles():
    _check(_plane([[1]]), [1], '1 x 1 filled')
    _check(_plane([[0]]), [1], '1 x 1 empty')
    run = (np.arange(37) % 5 < 3).astype(np.uint8) * 2
    _check(run[None, :], [2], '1 x 37')
    _check(run[:, None], [2], '37 x 1')
    for diag in ([[1, 0], [0, 1]], [[0, 1], [1, 0]]):
        got = _check(_plane(diag), [1], 'saddle')
        assert got[8][0][:, 2:].tolist() == [[8, 8]]                         # one ring that touches itself
        assert got[4][0][:, 2:].tolist() == [[4, 4], [4, 4]]                 # two squares


def test_holes_and_nesting():
    ring = np.ones((3, 3), dtype=np.uint8)
    ring[1, 1] = 0
    got = _check(ring, [1], 'hole')
    assert got[8][0][:, 2].tolist() == [4, 4]
    got = _check(_plane([[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]]), [1], 'hole at a saddle')          # (1, 1) and (2, 2) meet at a vertex
    assert got[8][0][:, 3].tolist() == [12, 4] and got[4][0][:, 3].tolist() == [16]      # 4: the "hole" is a bay of the outside
    nest = np.zeros((9, 11), dtype=np.uint8)
    nest[1:8, 1:10] = 1
    nest[2:7, 2:9] = 0
    nest[3:6, 3:8] = 1
    _check(nest, [1], 'nested, one id')
    nest[3:6, 3:8] = 2
    _check(nest, [1, 2], 'nested, two ids')
    _check(nest, [2, 1], 'nested, two ids, list reversed')


def test_borders_and_corner_density():
    got = _check(np.full((5, 9), 7, dtype=np.uint8), [7], 'full frame')
    assert got[8][1].tolist() == [0, 9, 9 | 5 << 16, 5 << 16]
    board = (np.add.outer(np.arange(8), np.arange(8)) % 2).astype(np.uint8)
    _check(board, [1], 'checkerboard')
    _check(board + 1, [1, 2], 'checkerboard of two ids')
    _check(_plane([[1, 2], [2, 1]]), [1, 2], 'two ids at a vertex')
    _check(_plane([[1, 2], [3, 4]]), [1, 2, 3, 4], 'four ids at a vertex')


def test_list_conventions():
    _check(np.arange(256, dtype=np.uint8).reshape(16, 16), list(range(1, 256)), 'ids 1 .. 255')
    rng = np.random.default_rng(5)
    ids = noise(rng, 33, 70, 0.5, ids=6)
    _check(ids, [2, 0, 300, 2, 9, -1, 5, 1], 'unlisted ids, entries outside 1 .. 255, a repeat, an object without a pixel')
    _check(ids, [], 'n == 0')
    _check(np.zeros((33, 70), dtype=np.uint8), [1, 2], 'nothing to trace')
    _check(ids, torch.tensor([3, 1], dtype=torch.int32, device='cuda'), 'ids on the device')


@pytest.mark.parametrize('H,W', [(7, 5), (64, 64), (65, 129)])
def test_random_planes(H, W):
    rng = np.random.default_rng(H * 131 + W)
    for density in (0.2, 0.5, 0.8):
        _check(noise(rng, H, W, density), [1, 2, 3], f'noise {density}', offsets=(0, 1))


def test_long_rings():
    got = _check(spiral(64, 64), [1], 'spiral')
    assert got[8][0].shape[0] == 1 and got[8][0][0, 3] > 4000                 # one ring far longer than a workgroup
    got = _check(comb(65, 129), [1], 'comb')
    assert got[8][0].shape[0] == 1 and got[8][0][0, 3] > 8000


def test_the_small_path_and_its_threshold():
    S = O.OpList.POLY_SMALL_EDGES
    got = _check(spiral(48, 48), [1], 'a long ring inside one workgroup')
    assert got[8][0].shape[0] == 1 and 2048 < got[8][0][0, 3] <= S
    dots = np.zeros((67, 67), dtype=np.uint8)
    dots[::2, ::2] = 1 + (np.arange(34 * 34).reshape(34, 34) % 3)            # isolated pixels: four edges each
    ys, xs = np.nonzero(dots)
    for pixels in (S // 4 - 1, S // 4, S // 4 + 1):                         # the last plane of the small path and the first beyond it
        ids = dots.copy()
        ids[ys[pixels:], xs[pixels:]] = 0
        got = _check(ids, [1, 2, 3], f'{pixels} isolated pixels')
        assert got[8][3] == 4 * pixels


def test_a_480p_plane():
    H, W = 480, 854
    yy, xx = np.mgrid[:H, :W]
    ids = np.zeros((H, W), dtype=np.uint8)
    ids[(yy - 200) ** 2 + (xx - 300) ** 2 < 150 ** 2] = 1
    ids[(yy - 210) ** 2 + (xx - 310) ** 2 < 40 ** 2] = 0                     # a hole
    ids[(yy - 100) ** 2 * 4 + (xx - 700) ** 2 < 120 ** 2] = 2
    ids[400:, 500:] = 3                                                      # cut by the border
    got = _check(ids, [1, 2, 3], '480p', offsets=(1,))
    assert got[8][2][:, 1].tolist() == [2, 1, 1]


def test_capacities():
    rng = np.random.default_rng(11)
    ids = noise(rng, 33, 70, 0.5)
    objs = [1, 2, 3]
    for conn in (4, 8):
        rings, verts, table, E = R.trace(ids, objs, conn)
        nbytes = 16 * len(rings) + 4 * len(verts)
        for path in (0, 1):
            s, t, u = _device(ids, objs, conn, path, E, nbytes - 4)          # one word short: bit 1, an untouched stream, valid totals
            _, want_t, want_u = R.stage(ids, objs, conn, E, nbytes - 4)
            assert u.tolist() == want_u.tolist() == [nbytes, 1, len(rings), E]
            assert np.array_equal(t, want_t) and bool((t[:, [0, 2]] == 0).all()) and np.array_equal(t[:, [1, 3]], table[:, [1, 3]])
            assert bool((s == FILL).all())
            s, t, u = _device(ids, objs, conn, path, E - 1, nbytes)          # bit 2: nothing is traced
            assert u.tolist() == [0, 2, 0, E] and bool((t == 0).all()) and bool((s == FILL).all())
            s, t, u = _device(ids, objs, conn, path, E, nbytes)              # both exactly enough
            assert u.tolist() == [nbytes, 0, len(rings), E]


def test_refusals_come_from_the_launcher():
    H, W, n, C = 37, 70, 3, 500
    need = O.OpList.polygon_scratch_words(H, W, n, C)
    ids = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    objs = torch.tensor([1, 2, 3], dtype=torch.int32, device='cuda')
    scratch = torch.full((need + 4,), -7, dtype=torch.int32, device='cuda')
    stream = torch.full((1024,), -7, dtype=torch.int32, device='cuda')
    table = torch.full((16,), -7, dtype=torch.int32, device='cuda')
    status = torch.full((4,), -7, dtype=torch.int32, device='cuda')
    good = dict(flags=8192, H=H, W=W, C=C, cap=4096, conn=8, path=0, hi=0, words=need, n=n, ids=ids, objs=objs, scratch=scratch, stream=stream,
                table=table, status=status)
    cases = [(dict(flags=8192 | f), 'unknown flags') for f in [1 << k for k in range(31) if k != 13]]
    cases += [(dict(H=0), 'empty shape'), (dict(W=0), 'empty shape'), (dict(W=-3), 'empty shape'),
              (dict(H=65536), '16 bits'), (dict(W=65536), '16 bits'), (dict(H=32768, W=16384), '2^29 lattice vertices'),
              (dict(n=-1), '-1 objects'), (dict(n=256), '256 objects'),
              (dict(conn=6), 'connectivity 6'), (dict(conn=0), 'connectivity 0'), (dict(path=2), 'path 2'), (dict(path=-1), 'path -1'),
              (dict(C=0), 'edge capacity 0'), (dict(C=-5), 'edge capacity -5'),
              (dict(cap=-4), 'stream capacity -4'), (dict(cap=4094), 'stream capacity 4094'),
              (dict(ids=None), 'the id plane (p2)'), (dict(status=None), 'the status (p4)'), (dict(stream=None), 'the stream (p3)'),
              (dict(scratch=None), 'the scratch (p5)'), (dict(objs=None), 'the object ids (p6)'), (dict(table=None), 'the object table (p7)'),
              (dict(stream=stream[1:]), 'stream 16-byte aligned'), (dict(scratch=scratch[1:]), 'scratch 16-byte aligned'),
              (dict(table=table[2:]), 'object table 16-byte aligned'),
              (dict(words=need - 1), f'scratch of {need - 1} words'), (dict(words=0), 'scratch of 0 words'), (dict(words=-1), 'scratch of -1 words')]
    lib = _lib.load()
    assert _lib.has_polygons() and lib.cutie_hip_build_flags() & 128 and lib.cutie_hip_abi_version() == 11
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [0, a['H'], a['W'], a['C'], a['cap'], a['conn'], a['path'], a['hi'], a['words'], a['n']], [],
               [None, None, a['ids'], a['stream'], a['status'], a['scratch'], a['objs'], a['table']])
        arr = ol.finalize()
        assert lib.cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in lib.cutie_hip_last_error().decode(), (change, lib.cutie_hip_last_error().decode())
    torch.cuda.synchronize()
    for t in (scratch, stream, table, status):
        assert bool((t == -7).all())
    assert bool((ids == 0).all())


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
    root = str(tmp_path_factory.mktemp('polygons'))
    src = os.path.join(HERE, 'golden', 'bike')
    for name in ('bikeA', 'bikeB'):
        img_dir, msk_dir = (os.path.join(root, d, name) for d in ('JPEGImages', 'Annotations'))
        for d in (img_dir, msk_dir):
            os.makedirs(d)
        shutil.copy(os.path.join(src, '00000.png'), msk_dir)
        for t in range(4):
            shutil.copy(os.path.join(src, f'0000{t}.jpg'), img_dir)
    for d in ('JPEGImages', 'Annotations'):
        shutil.copytree(os.path.join(root, d, 'bikeA'), os.path.join(root, 'one', d, 'bikeA'))
    return root


def _run(net, base, out, extra):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out,
                          '--dataset', 'd17-val'] + extra)
    E.check_args(ap, args)
    return E.run_dataset(net, default_config(), args)


REPORTS = {}


@pytest.mark.parametrize('name', ['host', 'device', 'lockstep', 'sizes'])
def test_eval_vos_polygons(net, dataset, name):
    from cutie_amd.inference.utils import results_utils as RU
    root, one = dataset, os.path.join(dataset, 'one')
    base, names, extra = {'host': (one, ['bikeA'], []), 'device': (one, ['bikeA'], ['--egress', 'device']),
                          'lockstep': (root, ['bikeA', 'bikeB'], ['--egress', 'device', '--lockstep', '2']),
                          'sizes': (one, ['bikeA'], ['--egress', 'device', '--sizes', '480', '600'])}[name]
    plain, out = os.path.join(root, 'plain_' + name), os.path.join(root, 'out_' + name)
    _run(net, base, plain, extra)
    _run(net, base, out, extra + ['--polygons'])
    assert not os.path.exists(os.path.join(plain, 'polygons'))
    for video in names:
        folder = os.path.join(out, 'Annotations', video)
        files = sorted(f for f in os.listdir(folder) if f.endswith('.png'))
        assert files == [f'0000{t}.png' for t in range(4)]
        for f in files:                          # the mask PNGs are those of the run without the switch
            assert open(os.path.join(folder, f), 'rb').read() == open(os.path.join(plain, 'Annotations', video, f), 'rb').read()
        report = json.load(open(os.path.join(out, 'polygons', video, 'polygons.json')))
        assert [f['frame'] for f in report['frames']] == [f[:-4] for f in files] and report['connectivity'] == 8
        rings = 0
        for frame in report['frames']:           # every frame's rings fill back to the PNG written for it
            plane = np.array(Image.open(os.path.join(folder, frame['frame'] + '.png')))
            H, W = plane.shape
            edges = nbytes = 0
            for oid, entry in frame['objects'].items():
                acc = np.zeros((H, W + 1), dtype=bool)
                for ring in entry['rings']:
                    pts = np.array(ring['points']).reshape(-1, 2)
                    for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, axis=0)):
                        if x0 == x1:
                            acc[min(y0, y1):max(y0, y1), x0] ^= True
                    edges += ring['perimeter']
                    nbytes += 16 + 4 * len(pts)
                    rings += 1
                assert np.array_equal(np.logical_xor.accumulate(acc, axis=1)[:, :W], plane == int(oid)) and entry['area'] == int((plane == int(oid)).sum())
            print(f'{name} {video} {frame["frame"]}: {edges} boundary edges, a stream of {nbytes} bytes')
            assert 0 < edges <= RU.POLY_EDGES // 8 and nbytes <= RU.POLY_STREAM // 8      # the bike example stays far below the saver's capacities
        assert rings >= 4                        # a no-op cannot pass
        REPORTS[name, video] = dict(report, video=None)
    if name == 'lockstep':                       # the clips in lock step and the clip alone report the same
        assert REPORTS['lockstep', 'bikeA'] == REPORTS['lockstep', 'bikeB']
        if ('device', 'bikeA') in REPORTS:
            assert REPORTS['lockstep', 'bikeA'] == REPORTS['device', 'bikeA']
