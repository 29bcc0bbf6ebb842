"""The distance transform on the MI355X (PROB_TO_ID flags == 4096, csrc/edt.hip) against the numpy model (tests/edt_ref.py): dist2 word for
word and band byte for byte, with guard bytes around both outputs and the scratch, the plane unchanged and at an aligned and a +1-byte
start, with both outputs, dist2 only and band only -- over the sizes at which the kernels take another path (degenerate rows and columns;
one less than, exactly, one more than and twice plus one the row segment, the column group and the row chunk of the column pass, which is
max(32, ceil(sqrt(limit))) rows), the limits 1, 2, 26, 65026 (radius 255 exactly) and 65536, S = 1, 3 and the maximum, the contents that
can break one of the passes, every refusal of the launcher; and end to end: eval_vos --trimap --dilate-mask --trimap-objects with host
egress, device egress, in lock step and multi-scale, every new PNG against the model applied to the mask PNG written next to it."""
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config

import edt_ref as R
from test_edt_cpu import DENSITIES, LIMITS, SETS3, check_outputs_against_masks, noise

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 256
FILL = 0x5a5a5a5a
T, CW, CH = O.OpList.EDT_ROW_SEGMENT, O.OpList.EDT_COL_GROUP, O.OpList.EDT_ROW_CHUNK


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device(ids, sets, inner, outer, mid, limit, offset=0, outputs=('dist2', 'band')):
    """the stage on one plane -> (dist2 or None, band or None); outputs and scratch sit between guards that must survive, the plane must
    come back unchanged; ``offset``: bytes between a 16-byte boundary and the plane's first pixel"""
    H, W = ids.shape
    S = sets.shape[0]
    room = torch.full((GUARD + 16 + H * W + GUARD,), 0xa5, dtype=torch.uint8, device='cuda')
    assert room.data_ptr() % 16 == 0
    lo = GUARD + offset
    plane = room[lo:lo + H * W].view(H, W)
    plane.copy_(torch.from_numpy(np.ascontiguousarray(ids)))
    assert plane.data_ptr() % 16 == offset
    before = room.clone()
    n = S * H * W
    words = O.OpList.edt_scratch_words(S, H, W)
    sbuf = torch.full((GUARD + words + GUARD,), FILL, dtype=torch.int32, device='cuda')
    dbuf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.int32, device='cuda')
    bbuf = torch.full((GUARD + offset + n + GUARD,), 0x3c, dtype=torch.uint8, device='cuda')      # (band: any alignment)
    dist2 = dbuf[GUARD:GUARD + n].view(S, H, W) if 'dist2' in outputs else None
    band = bbuf[GUARD + offset:GUARD + offset + n].view(S, H, W) if 'band' in outputs else None
    ol = O.OpList()
    ol.edt_band(plane, torch.from_numpy(sets).cuda(), sbuf[GUARD:GUARD + words], band=band, dist2=dist2, inner=inner, outer=outer, mid=mid, limit=limit)
    ol.run()
    torch.cuda.synchronize()
    assert torch.equal(room, before)                                         # read only
    assert bool((sbuf[:GUARD] == FILL).all()) and bool((sbuf[GUARD + words:] == FILL).all())
    assert bool((dbuf[:GUARD] == FILL).all()) and bool((dbuf[GUARD + n:] == FILL).all())
    assert bool((bbuf[:GUARD + offset] == 0x3c).all()) and bool((bbuf[GUARD + offset + n:] == 0x3c).all())
    if dist2 is None:
        assert bool((dbuf == FILL).all())
    if band is None:
        assert bool((bbuf == 0x3c).all())
    return (None if dist2 is None else dist2.cpu().numpy()), (None if band is None else band.cpu().numpy())


def _check(ids, sets, inner, outer, mid, limit, what='', offsets=(0, 1), outputs=(('dist2', 'band'),)):
    want_d, want_b = R.edt_band(ids, sets, inner, outer, mid, limit)         # once per case: every run below shares it
    for offset in offsets:
        for outs in outputs:
            d, b = _device(ids, sets, inner, outer, mid, limit, offset, outs)
            tag = (what, ids.shape, (inner, outer, mid, limit), offset, outs)
            if d is not None:
                assert np.array_equal(d, want_d), (tag, np.argwhere(d != want_d)[:8].tolist())
            if b is not None:
                assert np.array_equal(b, want_b), (tag, np.argwhere(b != want_b)[:8].tolist())
    return want_d, want_b


def _thresholds(limit, k):
    """(inner, outer, mid) below ``limit``, varied with k"""
    return [(0, limit - 1, 255), (limit - 1, 0, 0), (min(4, limit - 1), min(25, limit - 1), 128), ((limit - 1) // 2, (limit - 1) // 3, 7)][k % 4]


def _corners(H, W, inverse):
    """a single set pixel in each corner; inverse: a single unset pixel in each corner of a full frame"""
    ids = np.zeros((H, W), dtype=np.uint8)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        ids[y, x] = 2
    return (2 - ids).astype(np.uint8) if inverse else ids


SIZES = [(1, 1), (1, 37), (37, 1), (7, 5),
         (CH - 1, CW - 1), (CH, CW), (CH + 1, CW + 1), (2 * CH + 1, 2 * CW + 1),         # the column pass: row chunk (small limits), column group
         (CH + 1, T - 1), (CH - 1, T), (7, T + 1), (CH, 2 * T + 1),                      # the row pass: segment
         (254, 5), (255, 7), (256, 3), (257, 4), (513, 2)]                               # the row chunk at limits 65026 (255 rows) and 65536 (256)


@pytest.mark.parametrize('H,W', SIZES)
def test_kernel_equals_the_model(H, W):
    rng = np.random.default_rng(H * 977 + W)
    z = np.zeros((H, W), dtype=np.uint8)
    board = ((np.add.outer(np.arange(H), np.arange(W)) % 2) + 1).astype(np.uint8)
    planes = [('background', z), ('one object', z + 1), ('set corners', _corners(H, W, False)), ('unset corners', _corners(H, W, True)),
              ('checkerboard', board)] + [(f'noise {d}', noise(rng, H, W, d)) for d in DENSITIES]
    for k, (name, ids) in enumerate(planes):
        for limit in (LIMITS[k % 5], LIMITS[(k + 2) % 5]):                   # every limit on four planes of every size
            _check(ids, SETS3, *_thresholds(limit, k + limit), limit, what=name)
    # each output alone
    _check(planes[-3][1], SETS3, 4, 25, 128, 26, what='one output', offsets=(1,), outputs=(('dist2',), ('band',)))


@pytest.mark.parametrize('S', [1, 3, O.OpList.EDT_MAX_SETS])
def test_numbers_of_sets(S):
    rng = np.random.default_rng(S)
    ids = rng.integers(0, 2 * S + 2, size=(CH + 1, T + 1)).astype(np.uint8)
    ids[rng.random(ids.shape) < 0.9] = 0
    sets = R.sets_of(*[range(1 + s, 3 + 2 * s) for s in range(S)])           # overlapping, growing; id 0 in none
    for limit in (26, 65536):
        _check(ids, sets, 4, 25, 128, limit, what=f'S = {S}')


def test_every_id_and_overlapping_sets():
    ids = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16), 8, 0), 8, 1)          # ids 0 .. 255 as 8 x 8 blocks
    sets = R.sets_of(range(1, 101), range(50, 201), range(1, 256, 2), range(1, 256), [255], [])
    d, b = _check(ids, sets, 9, 16, 128, 65536, what='blocks')
    assert d[3][:8, :8].max() == 64 and (d[5] == 65536).all() and (b[5] == 0).all()  # id 0's block is 8 pixels deep; an empty set has no edge


def _sites(H, W, sites, oid=3):
    ids = np.zeros((H, W), dtype=np.uint8)
    for y, x in sites:
        ids[y, x] = oid
    return ids


def test_columns_with_and_without_the_other_class():
    H, W = 2 * CH + 5, 12
    ids = np.zeros((H, W), dtype=np.uint8)
    ids[:, 3] = 1                                # a column of the set alone: its pixels find nothing in their own column
    ids[CH, 5] = 1                               # a column with one set pixel, next to columns with none
    for limit in (26, 65536):
        d, _ = _check(ids, R.sets_of([1]), 0, limit - 1, 255, limit, what='columns')
        assert (d[0][:, 3] == 1).all() and d[0][CH, 5] == 1 and d[0][CH, 9] == 16
        _check((1 - ids).astype(np.uint8), R.sets_of([1]), limit - 1, 0, 0, limit, what='columns, inverse')


def test_three_four_five_across_the_seams():
    sets = R.sets_of([3])
    H, W = 2 * CH + 7, 2 * T + 5
    cases = [('row segment seam', (5, T - 2), (9, T + 1)), ('row chunk seam', (CH - 3, 40), (CH + 1, 43)),
             ('both', (CH + 1, T + 1), (CH - 3, T - 2)), ('column group seam', (20, CW - 2), (16, CW + 1))]
    for name, (py, px), site in cases:
        ids = _sites(H, W, [site])
        for outer, byte in ((24, 0), (25, 128)):
            d, b = _check(ids, sets, 0, outer, 128, 26, what=name)
            assert d[0][py, px] == 25 and b[0][py, px] == byte, (name, outer)
        # seen from the site's side: an unset pixel in a full frame
        d, b = _check((3 - ids).astype(np.uint8), sets, 24, 0, 128, 26, what=name + ', inverse', offsets=(0,))
        assert d[0][py, px] == 25 and b[0][py, px] == 255
    # across a row where g is capped: limit 26 caps g at 6.  (7 rows, 1 column) away is 50, and must not come out as 1 + 36 = 37 below a
    # larger limit; the 3-4-5 site stays 25 under both
    ids = _sites(H, W, [(9, T + 1), (12, T - 1)])
    d, _ = _check(ids, sets, 0, 25, 128, 26, what='capped g')
    assert d[0][5, T - 2] == 25 and d[0][5, T - 1] == 20
    ids = _sites(H, W, [(12, T - 1)])
    for limit, want in ((26, 26), (37, 37), (38, 38), (50, 50), (51, 50)):
        d, _ = _check(ids, sets, 0, limit - 1, 128, limit, what='capped g alone', offsets=(0,))
        assert d[0][5, T - 2] == want, (limit, int(d[0][5, T - 2]))


def test_sites_in_the_halo():
    sets, limit = R.sets_of([3]), 26                                         # ceil(sqrt(26)) = 6
    H, W = 3, 2 * T + 9
    for x in (T - 1, T):                         # the last pixel of a segment looks right, the first looks left
        for sign in (1, -1):
            for dx, want in ((5, 25), (6, 26), (7, 26)):
                ids = _sites(H, W, [(1, x + sign * dx)])
                d, b = _check(ids, sets, 0, 25, 128, limit, what='halo', offsets=(0,))
                assert d[0][1, x] == want and b[0][1, x] == (128 if want == 25 else 0), (x, sign, dx)
    for limit in (65026, 65536):                 # ceil(sqrt) = 255 and 256: the widest halo
        r = int(np.ceil(np.sqrt(limit)))
        for dx in (r - 1, r, r + 1):
            ids = _sites(H, W, [(1, T - 1 + dx)])
            d, _ = _check(ids, sets, 0, limit - 1, 255, limit, what='wide halo', offsets=(0,))
            assert d[0][1, T - 1] == min(dx * dx, limit), (limit, dx)


def test_a_480p_plane():
    H, W = 480, 854
    rng = np.random.default_rng(7)
    ids = noise(rng, H, W, 0.5)
    want_d, want_b = R.edt_band(ids, SETS3, 4, 25, 128, 65536)
    a = _device(ids, SETS3, 4, 25, 128, 65536, offset=1)
    b = _device(ids, SETS3, 4, 25, 128, 65536, offset=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])         # the same bytes twice
    assert np.array_equal(a[0], want_d) and np.array_equal(a[1], want_b)
    _check(noise(rng, H, W, 0.05), SETS3, 9, 25, 128, 26, what='noise 0.05', offsets=(0,))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_launcher():
    H, W, S = 37, 70, 3
    n = S * H * W
    need = (n + 1) // 2
    ids = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    sets = torch.from_numpy(SETS3).cuda()
    scratch = torch.full((need + 1,), -7, dtype=torch.int32, device='cuda')
    dist2 = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    band = torch.full((n,), 9, dtype=torch.uint8, device='cuda')
    odd = torch.zeros(n + 8, dtype=torch.int32, device='cuda').view(torch.uint8)
    good = dict(flags=4096, H=H, W=W, inner=4, outer=25, limit=26, mid=128, hi=0, words=need, S=S, ids=ids, sets=sets, scratch=scratch, dist2=dist2, band=band)
    cases = [(dict(flags=4096 | f), 'unknown flags') for f in [1 << k for k in range(31) if k != 12]]
    cases += [(dict(H=0), 'empty shape'), (dict(W=0), 'empty shape'), (dict(W=-3), 'empty shape'), (dict(H=1 << 16, W=1 << 15), 'exceeds 2^31 pixels'),
              (dict(S=0), '0 sets'), (dict(S=O.OpList.EDT_MAX_SETS + 1), f'{O.OpList.EDT_MAX_SETS + 1} sets'),
              (dict(inner=-1), 'negative threshold'), (dict(outer=-2), 'negative threshold'),
              (dict(limit=25), 'limit 25'), (dict(inner=26), 'limit 26'), (dict(limit=0, inner=0, outer=0), 'limit 0'), (dict(limit=65537), 'limit 65537'),
              (dict(mid=256), 'mid 256'), (dict(mid=-1), 'mid -1'),
              (dict(ids=None), 'the id plane (p2)'), (dict(sets=None), 'the sets (p6)'), (dict(scratch=None), 'the scratch (p5)'),
              (dict(dist2=None, band=None), 'band (p3), dist2 (p7) or both'),
              (dict(scratch=odd[1:]), '4-byte aligned'), (dict(dist2=odd[2:]), '4-byte aligned'),
              (dict(words=need - 1), f'scratch of {need - 1} words'), (dict(words=0), 'scratch of 0 words'), (dict(words=-1), 'scratch of -1 words')]
    lib = _lib.load()
    assert _lib.has_edt_band() and lib.cutie_hip_build_flags() & 64 and lib.cutie_hip_abi_version() == 11
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [0, a['H'], a['W'], a['inner'], a['outer'], a['limit'], a['mid'], a['hi'], a['words'], a['S']], [],
               [None, None, a['ids'], a['band'], None, a['scratch'], a['sets'], a['dist2']])
        arr = ol.finalize()
        assert lib.cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in lib.cutie_hip_last_error().decode(), (change, lib.cutie_hip_last_error().decode())
    torch.cuda.synchronize()
    assert bool((scratch == -7).all()) and bool((dist2 == -7).all()) and bool((band == 9).all()) and bool((ids == 0).all())


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
    root = str(tmp_path_factory.mktemp('edt'))
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


@pytest.mark.parametrize('name', ['host', 'device', 'lockstep', 'sizes'])
def test_eval_vos_trimaps(net, dataset, name):
    root, one = dataset, os.path.join(dataset, 'one')
    base, names, extra = {'host': (one, ['bikeA'], []), 'device': (one, ['bikeA'], ['--egress', 'device']),
                          'lockstep': (root, ['bikeA', 'bikeB'], ['--egress', 'device', '--lockstep', '2']),
                          'sizes': (one, ['bikeA'], ['--egress', 'device', '--sizes', '480', '600'])}[name]
    extra = extra + ['--min-region', '8']
    plain, out = os.path.join(root, 'plain_' + name), os.path.join(root, 'out_' + name)
    _run(net, base, plain, extra)
    _run(net, base, out, extra + ['--trimap', '2', '5', '--dilate-mask', '3', '--trimap-objects'])
    for video in names:
        folder = os.path.join(out, 'Annotations', video)
        files = sorted(f for f in os.listdir(folder) if f.endswith('.png'))
        assert files == [f'0000{t}.png' for t in range(4)]
        for f in files:                          # the mask PNGs are those of the run without the new options
            assert np.array_equal(np.array(Image.open(os.path.join(folder, f))), np.array(Image.open(os.path.join(plain, 'Annotations', video, f))))
        assert not any(os.path.isdir(os.path.join(plain, 'Annotations', video, d)) for d in ('trimap', 'dilated', 'trimap_objects'))
        seen = check_outputs_against_masks(folder, files, trimap=(2, 5), dilate=3, per_object=True)
        assert seen >= {0, 128, 255}             # a no-op cannot pass
