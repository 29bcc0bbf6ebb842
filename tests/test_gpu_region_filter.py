"""The region filter on the MI355X (PROB_TO_ID flags == 2048, csrc/regions.hip) against the numpy model (tests/region_ref.py): the plane byte
for byte and counts word for word, with guard bytes before and after the plane, the scratch and counts, under both connectivities and with
an aligned and a +1-byte plane start -- over the sizes at which the kernels take another path (degenerate rows and columns, one pixel less
than a tile, a tile, one more, two tiles and one, in each dimension), the contents that stress the merges (percolating noise, a checkerboard,
a serpentine through every tile, nested rings, holes whose fill pixel lies in the neighbour tile), areas exactly at the threshold within a
tile, across a seam and across a tile corner, the threshold extremes, order independence, every refusal of the launcher; and end to end:
eval_vos --min-region --fill-holes with host egress, device egress, in lock step and multi-scale, against the model applied to the PNGs of
the unfiltered run."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config

import region_ref as R
from test_region_filter_cpu import DENSITIES, noise, rings, serpentine, smallest_components
from test_track_report_cpu import check_report_against_files

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 256
FILL = 0x5a5a5a5a
TH, TW = O.OpList.REGION_TILE_H, O.OpList.REGION_TILE_W


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device(ids, min_region, fill_holes, connectivity, offset=0):
    """the stage on one plane -> (plane, counts); plane, scratch and counts sit between guards that must survive; counts is pre-filled with
    garbage; ``offset``: bytes between a 16-byte boundary and the plane's first pixel"""
    H, W = ids.shape
    room = torch.full((GUARD + 16 + H * W + GUARD,), 0xa5, dtype=torch.uint8, device='cuda')
    assert room.data_ptr() % 16 == 0
    lo = GUARD + offset
    plane = room[lo:lo + H * W].view(H, W)
    plane.copy_(torch.from_numpy(np.ascontiguousarray(ids)))
    assert plane.data_ptr() % 16 == offset
    words = O.OpList.region_scratch_words(H, W)
    sbuf = torch.full((GUARD + words + GUARD,), FILL, dtype=torch.int32, device='cuda')
    cbuf = torch.full((GUARD + 4 + GUARD,), FILL, dtype=torch.int32, device='cuda')
    ol = O.OpList()
    ol.region_filter(plane, sbuf[GUARD:GUARD + words], cbuf[GUARD:GUARD + 4], min_region=min_region, fill_holes=fill_holes, connectivity=connectivity)
    ol.run()
    torch.cuda.synchronize()
    assert bool((room[:lo] == 0xa5).all()) and bool((room[lo + H * W:] == 0xa5).all())
    assert bool((sbuf[:GUARD] == FILL).all()) and bool((sbuf[GUARD + words:] == FILL).all())
    assert bool((cbuf[:GUARD] == FILL).all()) and bool((cbuf[GUARD + 4:] == FILL).all())
    return plane.cpu().numpy(), cbuf[GUARD:GUARD + 4].cpu().numpy()


_wants = {}


def _want(ids, min_region, fill_holes, connectivity):
    """the model's answer, computed once per case (the aligned and the +1 run share it)"""
    key = (ids.shape, ids.tobytes(), min_region, fill_holes, connectivity)
    if key not in _wants:
        _wants.clear()
        _wants[key] = R.region_filter(ids, min_region, fill_holes, connectivity)
    return _wants[key]


def _check(ids, min_region, fill_holes, what='', connectivities=(4, 8), offsets=(0, 1)):
    total = np.zeros(4, dtype=np.int64)
    for conn in connectivities:
        for offset in offsets:
            want, counts = _want(ids, min_region, fill_holes, conn)
            got, got_counts = _device(ids, min_region, fill_holes, conn, offset)
            assert np.array_equal(got_counts, counts), (what, ids.shape, conn, offset, got_counts.tolist(), counts.tolist())
            assert np.array_equal(got, want), (what, ids.shape, conn, offset, np.argwhere(got != want)[:8].tolist())
            total += counts
    return total


SIZES = [(1, 1), (1, 37), (37, 1), (7, 5), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (TH - 1, 2 * TW + 1), (2 * TH + 1, TW)]


@pytest.mark.parametrize('H,W', SIZES)
def test_kernel_equals_the_model(H, W):
    rng = np.random.default_rng(H * 977 + W)
    z = np.zeros((H, W), dtype=np.uint8)
    board = ((np.add.outer(np.arange(H), np.arange(W)) % 2) + 1).astype(np.uint8)       # two ids: plane-spanning under 8, one pixel per component under 4
    planes = [('background', z), ('one object', z + 9), ('checkerboard', board), ('serpentine', serpentine(H, W)), ('rings', rings(H, W))]
    planes += [(f'noise {d}', noise(rng, H, W, d)) for d in DENSITIES]
    seen = np.zeros(4, dtype=np.int64)
    for name, ids in planes:
        for min_region, fill_holes in ((5, 5), (40, 0), (0, 40), (3, 200)):
            seen += _check(ids, min_region, fill_holes, what=name)
    if H * W > 64:
        assert (seen > 0).all(), seen.tolist()                               # (both stages did something somewhere)
    # thresholds 0 and 1 switch a stage off; counts are written all the same
    for thr in ((0, 0), (1, 1)):
        assert _check(planes[-3][1], *thr, what='off').tolist() == [0, 0, 0, 0]
    # the extremes: every object goes; every enclosed hole goes
    total = _check(planes[-3][1], H * W + 1, 0, what='clears every object')
    assert total[1] == 4 * int((planes[-3][1] != 0).sum())
    _check(planes[-3][1], 0, H * W, what='fills every hole')
    _check(rings(H, W), H * W + 1, H * W, what='both extremes')


def test_a_480p_plane():
    H, W = 480, 854
    rng = np.random.default_rng(7)
    ids = noise(rng, H, W, 0.5)
    want, counts = R.region_filter(ids, 30, 30, 8)
    a, ca = _device(ids, 30, 30, 8, offset=1)
    b, cb = _device(ids, 30, 30, 8, offset=1)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)                   # order independence: the same bytes twice
    assert np.array_equal(a, want) and np.array_equal(ca, counts) and (counts > 0).all()
    for d in (0.41, 0.59):                                                   # the two site-percolation thresholds: the most tortuous components
        _check(noise(rng, H, W, d), 2000, 2000, what=f'noise {d}', offsets=(0,))
    _check(serpentine(H, W), H * W // 4, 0, what='serpentine, kept', connectivities=(4,), offsets=(1,))
    _check(serpentine(H, W), H * W, 50, what='serpentine, dropped', connectivities=(8,), offsets=(0,))
    yy, xx = np.mgrid[:H, :W]
    blobs = np.zeros((H, W), dtype=np.uint8)
    for oid, (cy, cx, ry, rx) in ((1, (120, 200, 80, 150)), (2, (300, 600, 150, 90)), (3, (400, 100, 60, 60))):
        blobs[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = oid
    blobs[rng.random((H, W)) < 0.002] = 2                                    # specks of object 2 everywhere, pinholes in the blobs
    blobs[rng.random((H, W)) < 0.002] = 0
    total = _check(blobs, 20, 20, what='three blobs with specks and pinholes')
    assert (total > 0).all()


def test_every_id_is_an_object():
    ids = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16), 16, 0), 16, 1)        # ids 0 .. 255 as 16 x 16 blocks
    assert _check(ids, 256, 0, what='blocks of 256 pixels stay').tolist() == [0, 0, 0, 0]
    assert _check(ids, 257, 0, what='blocks of 256 pixels go')[:2].tolist() == [4 * 255, 4 * 255 * 256]
    ids[0:16, 0:16] = 1
    ids[4:8, 4:8] = 0
    assert _check(ids, 0, 17, what='a hole inside id 1')[2:].tolist() == [4, 64]


def _with_component(H, W, pixels, oid=3):
    ids = np.zeros((H, W), dtype=np.uint8)
    for y, x in pixels:
        ids[y, x] = oid
    return ids


def test_areas_at_the_threshold():
    H, W = 2 * TH + 3, 2 * TW + 5
    inside = [(3, 5), (3, 6), (3, 7), (4, 7), (5, 7), (5, 8)]
    across_row_seam = [(TH - 2, 9), (TH - 1, 9), (TH, 9), (TH + 1, 9), (TH + 1, 10), (TH + 2, 10)]
    across_column_seam = [(5, TW - 3), (5, TW - 2), (5, TW - 1), (5, TW), (5, TW + 1), (6, TW + 1)]
    around_corner = [(TH - 2, TW - 1), (TH - 1, TW - 1), (TH - 1, TW), (TH, TW), (TH, TW - 1), (TH + 1, TW - 1)]        # all four tiles
    for name, pixels in (('inside', inside), ('row seam', across_row_seam), ('column seam', across_column_seam), ('corner', around_corner)):
        n = len(pixels)
        ids = _with_component(H, W, pixels)
        assert _check(ids, n, 0, what=name + ': area N stays')[:2].tolist() == [0, 0]
        assert _check(ids, n + 1, 0, what=name + ': area N - 1 goes')[:2].tolist() == [4, 4 * n]
        hole = 7 - _with_component(H, W, pixels, 7)                          # the same shape as a hole in object 7
        assert _check(hole, 0, n, what=name + ': hole of N stays')[2:].tolist() == [0, 0]
        assert _check(hole, 0, n + 1, what=name + ': hole of N - 1 goes')[2:].tolist() == [4, 4 * n]
    # across the corner by the diagonal alone: one component under 8, two under 4
    for pixels in ([(TH - 1, TW - 1), (TH, TW)], [(TH - 1, TW), (TH, TW - 1)]):
        ids = _with_component(H, W, pixels)
        assert _check(ids, 2, 0, connectivities=(8,))[:2].tolist() == [0, 0] and _check(ids, 2, 0, connectivities=(4,))[:2].tolist() == [4, 4]
        hole = 7 - _with_component(H, W, pixels, 7)
        assert _check(hole, 0, 2, connectivities=(4,))[2:].tolist() == [4, 4] and _check(hole, 0, 3, connectivities=(8,))[2:].tolist() == [2, 4]


def test_holes_and_their_fill_pixel():
    H, W = 2 * TH + 3, 2 * TW + 5
    ids = np.full((H, W), 4, dtype=np.uint8)
    ids[:, :TW] = 6
    ids[5:8, TW:TW + 3] = 0                                                  # first pixel in column 0 of a tile: filled from the neighbour tile, with 6
    ids[TH:TH + 2, 10:12] = 0                                                # first pixel in row 0 of a tile
    total = _check(ids, 0, 10, what='fill pixel in the neighbour tile', connectivities=(8,), offsets=(0,))
    assert total[2:].tolist() == [2, 13]
    assert (R.region_filter(ids, 0, 10, 8)[0][5:8, TW:TW + 3] == 6).all()
    # a hole that touches the frame's border by one pixel is none: every border and every corner
    for y, x in ((0, 9), (H - 1, 9), (9, 0), (9, W - 1), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        yi, xi = min(max(y, 1), H - 2), min(max(x, 1), W - 2)                # the border pixel's neighbour inside (a corner's: the diagonal one)
        ids = np.full((H, W), 4, dtype=np.uint8)
        ids[yi, xi] = ids[y, x] = 0
        corner = yi != y and xi != x
        assert _check(ids, 0, 100, what=f'open at {(y, x)}', offsets=(0,), connectivities=(8,))[2:].tolist() == [0, 0]
        assert _check(ids, 0, 100, what=f'open at {(y, x)}', offsets=(0,), connectivities=(4,))[2:].tolist() == ([1, 1] if corner else [0, 0])
        ids[y, x] = 4                                                        # closed again
        assert _check(ids, 0, 100, what=f'closed at {(y, x)}', offsets=(0,))[2:].tolist() == [2, 2]
    # a speck of B inside A ends up as A: islands run before holes
    ids = np.full((H, W), 4, dtype=np.uint8)
    ids[TH - 1:TH + 1, TW - 1:TW + 1] = 9
    got, counts = _device(ids, 5, 5, 8)
    assert (got == 4).all() and counts.tolist() == [1, 4, 1, 4]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_launcher():
    H, W = 37, 70
    ids = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    scratch = torch.full((2 * H * W + 1,), -7, dtype=torch.int32, device='cuda')
    counts = torch.full((4,), -7, dtype=torch.int32, device='cuda')
    odd = torch.zeros(2 * H * W + 8, dtype=torch.int32, device='cuda').view(torch.uint8)
    good = dict(flags=2048, H=H, W=W, a=5, b=5, conn=8, words=2 * H * W, hi=0, ids=ids, scratch=scratch, counts=counts)
    cases = [(dict(flags=2048 | f), 'unknown flags') for f in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)]
    cases += [(dict(H=0), 'empty shape'), (dict(W=0), 'empty shape'), (dict(W=-3), 'empty shape'), (dict(H=1 << 16, W=1 << 15), 'exceeds 2^31 pixels'),
              (dict(a=-1), 'negative threshold'), (dict(b=-2), 'negative threshold'), (dict(conn=6), 'connectivity 6'), (dict(conn=0), 'connectivity 0'),
              (dict(ids=None), 'the id plane (p2)'), (dict(scratch=None), 'the scratch (p5)'), (dict(counts=None), 'counts (p7)'),
              (dict(scratch=odd[1:]), '4-byte aligned'), (dict(counts=odd[2:]), '4-byte aligned'),
              (dict(words=2 * H * W - 1), 'scratch of 5179 words'), (dict(words=0), 'scratch of 0 words'), (dict(words=-1), 'scratch of -1 words')]
    lib = _lib.load()
    assert _lib.has_region_filter() and lib.cutie_hip_build_flags() & 32 and lib.cutie_hip_abi_version() == 11
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [0, a['H'], a['W'], a['a'], a['b'], a['conn'], 0, 0, a['words'], a['hi']], [],
               [None, None, a['ids'], None, None, a['scratch'], None, a['counts']])
        arr = ol.finalize()
        assert lib.cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in lib.cutie_hip_last_error().decode(), (change, lib.cutie_hip_last_error().decode())
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((scratch == -7).all()) and bool((ids == 0).all())


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
    """the tests/golden/bike frames as two videos of one dataset, and as a dataset of one video; ground truth of every frame: the first mask"""
    root = str(tmp_path_factory.mktemp('regions'))
    src = os.path.join(HERE, 'golden', 'bike')
    for name in ('bikeA', 'bikeB'):
        img_dir, msk_dir, gt_dir = (os.path.join(root, d, name) for d in ('JPEGImages', 'Annotations', 'GT'))
        for d in (img_dir, msk_dir, gt_dir):
            os.makedirs(d)
        shutil.copy(os.path.join(src, '00000.png'), msk_dir)
        for t in range(4):
            shutil.copy(os.path.join(src, f'0000{t}.jpg'), img_dir)
            shutil.copy(os.path.join(src, '00000.png'), os.path.join(gt_dir, f'0000{t}.png'))
    for d in ('JPEGImages', 'Annotations', 'GT'):
        shutil.copytree(os.path.join(root, d, 'bikeA'), os.path.join(root, 'one', d, 'bikeA'))
    return root


def _run(net, base, out, extra):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out,
                          '--dataset', 'd17-val'] + extra)
    E.check_args(ap, args)
    return E.run_dataset(net, default_config(), args)


@pytest.mark.parametrize('name', ['host', 'device', 'lockstep', 'sizes'])
def test_eval_vos_region_filter(net, dataset, name):
    from cutie_amd.score_masks import score_folders
    root, one = dataset, os.path.join(dataset, 'one')
    base, names, extra = {'host': (one, ['bikeA'], []), 'device': (one, ['bikeA'], ['--egress', 'device']),
                          'lockstep': (root, ['bikeA', 'bikeB'], ['--egress', 'device', '--lockstep', '2']),
                          'sizes': (one, ['bikeA'], ['--egress', 'device', '--sizes', '480', '600'])}[name]
    plain = os.path.join(root, 'plain_' + name)
    _run(net, base, plain, extra)
    files = sorted(os.listdir(os.path.join(plain, 'Annotations', 'bikeA')))
    assert files == [f'0000{t}.png' for t in range(4)]
    raw = {v: [np.array(Image.open(os.path.join(plain, 'Annotations', v, f))) for f in files] for v in names}
    # thresholds from the unfiltered files: one above the smallest object component and the smallest enclosed background component
    island, hole = smallest_components([m for v in names for m in raw[v]], 8)
    min_region, fill_holes = island + 1, (hole + 1 if hole is not None else 0)
    out = os.path.join(root, 'out_' + name)
    res = _run(net, base, out, extra + ['--min-region', str(min_region), '--fill-holes', str(fill_holes), '--tracks', '--score', '--gt', os.path.join(base, 'GT')])
    assert sorted(r['tracks']['video'] for r in res.values()) == names
    for r in res.values():
        video = r['tracks']['video']
        total = np.zeros(4, dtype=np.int64)
        for f, m in zip(files, raw[video]):
            want, counts = R.region_filter(m, min_region, fill_holes, 8)
            total += counts
            assert np.array_equal(np.array(Image.open(os.path.join(out, 'Annotations', video, f))), want), (name, video, f)
        got = r['regions']
        assert [got['islands_removed'], got['pixels_cleared'], got['holes_filled'], got['pixels_filled']] == total.tolist()
        assert got['frames'] == 4 and (got['min_region'], got['fill_holes'], got['connectivity']) == (min_region, fill_holes, 8)
        assert total[0] > 0 and total[1] > 0 and (hole is None or (total[2] > 0 and total[3] > 0))      # a no-op cannot pass
        check_report_against_files(r['tracks'], os.path.join(out, 'Annotations', video))                 # --tracks reads the filtered plane
    # --score counted on the filtered planes: the files of the run = score_masks over the folder it wrote
    score_folders(os.path.join(out, 'Annotations'), os.path.join(base, 'GT'), dataset='d17-val', output=os.path.join(out, 'again'))
    read = lambda d: {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith('.csv') or f == 'scores.json'}
    assert len(read(out)) == 3 and read(out) == read(os.path.join(out, 'again'))
    assert sorted(json.load(open(os.path.join(out, 'scores.json')))['sequences']) == names
