"""The region filter without a GPU: the numpy model of the contract (tests/region_ref.py) against scipy.ndimage.label, the conventions of
the contract on hand-made planes, the descriptor and the argument checks of OpList.region_filter, and the wiring: through the interpreter
(tests/mock_exec_regions.py) every path of a ResultSaver with min_region / fill_holes -- host and device egress, the merged plane, BURST RLE
strings, the overlay, the track report, the scorer -- sees the model applied to the plane of the unfiltered run; the probabilities are
untouched; eval_vos --min-region --fill-holes writes the same files for a clip alone and for two copies of it in lock step."""
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

import region_ref as R
from test_track_report_cpu import check_report_against_files, softmax_planes

HERE = os.path.dirname(os.path.abspath(__file__))
DENSITIES = (0.2, 0.41, 0.5, 0.59, 0.8)         # 0.41 and 0.59: the site-percolation thresholds of the square lattice under 8 and 4 neighbours
STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), dtype=bool)}


# ---- planes ----------------------------------------------------------------------------------------------------------------------------------
def noise(rng, H, W, density):
    """three ids: a pixel is an object's with probability ``density`` -- object 1, or (one in ten) object 2 -- else background"""
    ids = (rng.random((H, W)) < density).astype(np.uint8)
    ids[(ids != 0) & (rng.random((H, W)) < 0.1)] = 2
    return ids


def serpentine(H, W):
    """one object, one pixel wide, through the whole plane: every second row, joined at alternating ends -- the longest chain of labels"""
    ids = np.zeros((H, W), dtype=np.uint8)
    ids[::2, :] = 5
    for k, y in enumerate(range(1, H, 2)):
        ids[y, (W - 1) if k % 2 == 0 else 0] = 5
    return ids


def rings(H, W):
    """nested rings of two objects around a background core, one pixel of background around everything"""
    ids = np.zeros((H, W), dtype=np.uint8)
    for k in range(1, (min(H, W) + 1) // 2):
        ids[k:H - k, k:W - k] = (3, 8, 0)[(k - 1) % 3]
    return ids


# ---- scipy restatement --------------------------------------------------------------------------------------------------------------------
def scipy_filter(ids, min_region, fill_holes, connectivity):
    out = ids.copy()
    counts = [0, 0, 0, 0]
    if min_region >= 2:
        for oid in np.unique(ids[ids != 0]):
            lab, n = ndimage.label(ids == oid, structure=STRUCTURE[connectivity])
            area = np.bincount(lab.ravel(), minlength=n + 1)
            small = (area < min_region)
            small[0] = False
            counts[0] += int(small.sum())
            counts[1] += int(area[small].sum())
            out[small[lab]] = 0
    if fill_holes >= 2:
        src = out.copy()
        H, W = src.shape
        lab, n = ndimage.label(src == 0, structure=STRUCTURE[connectivity])
        area = np.bincount(lab.ravel(), minlength=n + 1)
        is_open = np.zeros(n + 1, dtype=bool)
        for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            is_open[edge] = True
        for k in range(1, n + 1):
            if is_open[k] or area[k] >= fill_holes:
                continue
            first = int(np.flatnonzero(lab.ravel() == k)[0])
            y0, x0 = divmod(first, W)
            assert x0 > 0 and src[y0, x0 - 1] != 0
            out[lab == k] = src[y0, x0 - 1]
            counts[2] += 1
            counts[3] += int(area[k])
    return out, np.array(counts, dtype=np.int32)


def smallest_components(planes, connectivity):
    """(area of the smallest object component, area of the smallest enclosed background component or None) over the planes, by scipy"""
    island, hole = None, None
    for ids in planes:
        for oid in np.unique(ids[ids != 0]):
            lab, n = ndimage.label(ids == oid, structure=STRUCTURE[connectivity])
            a = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            island = int(a.min()) if island is None else min(island, int(a.min()))
        lab, n = ndimage.label(ids == 0, structure=STRUCTURE[connectivity])
        area = np.bincount(lab.ravel(), minlength=n + 1)
        closed = np.ones(n + 1, dtype=bool)
        closed[0] = False
        for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            closed[edge] = False
        if closed.any():
            hole = int(area[closed].min()) if hole is None else min(hole, int(area[closed].min()))
    return island, hole


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('H,W', [(1, 1), (1, 37), (37, 1), (7, 5), (64, 64), (65, 129)])
def test_model_equals_scipy(H, W, connectivity):
    rng = np.random.default_rng(H * 1009 + W)
    changed = np.zeros(4, dtype=np.int64)
    for density in DENSITIES:
        ids = noise(rng, H, W, density)
        for min_region, fill_holes in ((0, 0), (1, 1), (2, 2), (6, 0), (0, 6), (9, 30), (H * W + 1, H * W)):
            got, counts = R.region_filter(ids, min_region, fill_holes, connectivity)
            want, want_counts = scipy_filter(ids, min_region, fill_holes, connectivity)
            assert np.array_equal(got, want) and counts.tolist() == want_counts.tolist(), (density, min_region, fill_holes)
            assert got.dtype == np.uint8 and counts.dtype == np.int32
            changed += counts
    if H * W >= 64 * 64:
        assert (changed > 0).all()
    for ids in (serpentine(H, W), rings(H, W)):
        for thr in ((4, 4), (H * W, H * W)):
            got, counts = R.region_filter(ids, *thr, connectivity)
            want, want_counts = scipy_filter(ids, *thr, connectivity)
            assert np.array_equal(got, want) and counts.tolist() == want_counts.tolist()


def test_roots_are_first_pixels():
    rng = np.random.default_rng(4)
    ids = noise(rng, 40, 70, 0.55)
    for connectivity in (4, 8):
        r = R.roots(np.where(ids != 0, ids.astype(np.int64), -1), connectivity)
        for oid in (1, 2):
            lab, n = ndimage.label(ids == oid, structure=STRUCTURE[connectivity])
            first = ndimage.minimum(np.arange(ids.size).reshape(ids.shape), lab, index=np.arange(1, n + 1)).astype(np.int64)
            assert np.array_equal(r[ids == oid], first[lab[ids == oid] - 1])
        assert (r[ids == 0] == -1).all()


# ---- conventions -------------------------------------------------------------------------------------------------------------------------------
def test_conventions_of_the_contract():
    rng = np.random.default_rng(1)
    ids = noise(rng, 30, 50, 0.5)
    for thr in ((0, 0), (1, 1), (0, 1), (1, 0)):                             # thresholds 0 and 1 do nothing
        got, counts = R.region_filter(ids, *thr)
        assert np.array_equal(got, ids) and counts.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        R.region_filter(ids, -1, 0)
    with pytest.raises(ValueError):
        R.region_filter(ids, 2, 2, connectivity=6)
    # area exactly N - 1 and exactly N
    ids = np.zeros((9, 12), dtype=np.uint8)
    ids[2, 3:8] = 7                                                          # 5 pixels
    ids[5:7, 2:5] = 7                                                        # 6 pixels, another component of the same id
    got, counts = R.region_filter(ids, 6, 0)
    assert (got[2] == 0).all() and np.array_equal(got[5:7], ids[5:7]) and counts.tolist() == [1, 5, 0, 0]
    assert R.region_filter(ids, 5, 0)[1].tolist() == [0, 0, 0, 0] and R.region_filter(ids, 7, 0)[1].tolist() == [2, 11, 0, 0]
    hole = np.full((9, 12), 7, dtype=np.uint8)
    hole[3, 3:8] = 0
    assert R.region_filter(hole, 0, 5)[1].tolist() == [0, 0, 0, 0]
    got, counts = R.region_filter(hole, 0, 6)
    assert (got == 7).all() and counts.tolist() == [0, 0, 1, 5]
    # a hole that touches the border by one pixel is none: each border, each corner (a corner's neighbour inside is the diagonal one)
    H, W = 9, 12
    for y, x in ((0, 5), (H - 1, 5), (4, 0), (4, W - 1), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        yi, xi = min(max(y, 1), H - 2), min(max(x, 1), W - 2)
        ids = np.full((H, W), 4, dtype=np.uint8)
        ids[yi, xi] = ids[y, x] = 0
        corner = yi != y and xi != x
        assert R.region_filter(ids, 0, 100, 8)[1].tolist() == [0, 0, 0, 0]
        assert R.region_filter(ids, 0, 100, 4)[1].tolist() == ([0, 0, 1, 1] if corner else [0, 0, 0, 0])
        ids[y, x] = 4
        assert R.region_filter(ids, 0, 100, 4)[1].tolist() == [0, 0, 1, 1]
    # a diagonal line: one component under 8, one pixel each under 4
    ids = np.zeros((8, 8), dtype=np.uint8)
    ids[np.arange(1, 7), np.arange(1, 7)] = 3
    assert R.region_filter(ids, 6, 0, 8)[1].tolist() == [0, 0, 0, 0] and R.region_filter(ids, 2, 0, 4)[1].tolist() == [6, 6, 0, 0]
    anti = 3 - ids                                                           # the same line as background in object 3: under 8 it is one hole,
    assert R.region_filter(anti, 0, 7, 8)[1].tolist() == [0, 0, 1, 6]        # under 4 six
    assert R.region_filter(anti, 0, 6, 8)[1].tolist() == [0, 0, 0, 0] and R.region_filter(anti, 0, 2, 4)[1].tolist() == [0, 0, 6, 6]
    # two ids that touch are two components
    ids = np.zeros((6, 10), dtype=np.uint8)
    ids[2, 2:5], ids[2, 5:8] = 1, 2
    assert R.region_filter(ids, 4, 0)[1].tolist() == [2, 6, 0, 0]
    # a speck of B inside A becomes A: islands run before holes; the fill is the id left of the hole's first pixel
    ids = np.full((10, 14), 4, dtype=np.uint8)
    ids[:, 7:] = 6
    ids[4:6, 3:5] = 9
    ids[4:6, 9:11] = 9
    got, counts = R.region_filter(ids, 5, 5)
    want = np.full((10, 14), 4, dtype=np.uint8)
    want[:, 7:] = 6
    assert np.array_equal(got, want) and counts.tolist() == [2, 8, 2, 8]
    assert R.region_filter(ids, 5, 0)[1].tolist() == [2, 8, 0, 0] and np.array_equal(R.region_filter(ids, 0, 5)[0], ids)
    # nested rings: the core hole is filled with the innermost ring's id; a thin ring that goes leaves a hole for the ring around it
    ids = np.zeros((15, 15), dtype=np.uint8)
    ids[1:14, 1:14] = 3
    ids[3:12, 3:12] = 8
    ids[5:10, 5:10] = 0
    ids[6:9, 6:9] = 3
    got, counts = R.region_filter(ids, 10, 0)                               # the 3 x 3 core of object 3 goes ...
    assert (got[6:9, 6:9] == 0).all() and counts.tolist() == [1, 9, 0, 0]
    got, counts = R.region_filter(ids, 10, 26)                              # ... and the hole of 25 it leaves becomes the ring of 8
    assert (got[5:10, 5:10] == 8).all() and counts.tolist() == [1, 9, 1, 25]
    assert R.region_filter(ids, 10, 25)[1].tolist() == [1, 9, 0, 0]


# ---- the op --------------------------------------------------------------------------------------------------------------------------------
def test_region_filter_descriptor_and_argument_checks():
    from mock_exec_regions import RegionsMockExecutor
    _lib.set_executor_for_testing(RegionsMockExecutor())
    try:
        assert O.OpList.REGION_TILE_H >= 1 and O.OpList.REGION_TILE_W >= 1 and O.OpList.region_scratch_words(5, 7) >= 70
        ids = torch.zeros((5, 7), dtype=torch.uint8)
        scratch = torch.zeros(O.OpList.region_scratch_words(5, 7) + 3, dtype=torch.int32)
        counts = torch.zeros(4, dtype=torch.int32)
        ol = O.OpList()
        ol.region_filter(ids, scratch, counts)
        ol.region_filter(ids, scratch, counts, min_region=9, fill_holes=4, connectivity=4)
        arr = ol.finalize()
        assert arr['kind'].tolist() == [O.PROB_TO_ID] * 2 and arr['flags'].tolist() == [2048] * 2
        assert arr['i'][0, :10].tolist() == [0, 5, 7, 0, 0, 8, 0, 0, scratch.numel(), 0]
        assert arr['i'][1, :10].tolist() == [0, 5, 7, 9, 4, 4, 0, 0, scratch.numel(), 0]
        assert arr['p'][1, 2] == ids.data_ptr() and arr['p'][1, 5] == scratch.data_ptr() and arr['p'][1, 7] == counts.data_ptr()
        assert [int(arr['p'][1, k]) for k in (0, 1, 3, 4, 6)] == [0] * 5
        good = dict(ids_plane=ids, scratch=scratch, counts=counts)
        for change, msg in ((dict(ids_plane=ids.int()), 'uint8'), (dict(ids_plane=torch.zeros((5, 8), dtype=torch.uint8)[:, :7]), 'contiguous'),
                            (dict(ids_plane=torch.zeros((2, 5, 7), dtype=torch.uint8)), 'uint8'), (dict(ids_plane=torch.zeros((0, 7), dtype=torch.uint8)), 'H, W >= 1'),
                            (dict(min_region=-1), 'not negative'), (dict(fill_holes=-3), 'not negative'), (dict(connectivity=6), 'connectivity 6'),
                            (dict(scratch=scratch[:69]), 'at least 70 words'), (dict(scratch=scratch.float()), 'int32'),
                            (dict(counts=counts.long()), r'int32 \[4\]'), (dict(counts=torch.zeros(5, dtype=torch.int32)), r'int32 \[4\]')):
            with pytest.raises(ValueError, match=msg):
                O.OpList().region_filter(**dict(good, **change))
        # the interpreter runs the model
        plane = torch.from_numpy(rings(12, 17))
        before = plane.numpy().copy()
        big = torch.zeros(O.OpList.region_scratch_words(12, 17), dtype=torch.int32)
        counts.fill_(77)
        ol = O.OpList()
        ol.region_filter(plane, big, counts, min_region=50, fill_holes=50)
        ol.run()
        want, want_counts = R.region_filter(before, 50, 50)
        assert np.array_equal(plane.numpy(), want) and counts.tolist() == want_counts.tolist() and want_counts[0] > 0
    finally:
        _lib.set_executor_for_testing(None)


def test_a_stale_library_is_named(monkeypatch):
    monkeypatch.setattr(_lib, 'has_region_filter', lambda: False)
    _lib.set_executor_for_testing(None)
    with pytest.raises(_lib.HipLibraryError, match='no region filter'):
        O.OpList().region_filter(torch.zeros((5, 7), dtype=torch.uint8), torch.zeros(70, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))


# ---- host wiring -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def regions_executor():
    from mock_exec_regions import RegionsMockExecutor
    ex = RegionsMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    yield ex
    _lib.set_executor_for_testing(None)


def _saver(out, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    om.add_new_objects([5, 3])

    def to_mask(prob, dtype=torch.int64):
        return torch.tensor([0, 5, 3])[prob.argmax(0)].to(dtype)
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om, output_prob_to_mask=to_mask)
    kw.setdefault('dataset', 'generic')
    return ResultSaver(out, 'vid', object_manager=om, use_long_id=False, processor=proc, **kw)


def _frames(T=3, P=3, h=24, w=40):
    """speckled probabilities: blocky planes with single samples flipped, as un-padded views of padded buffers"""
    rng = np.random.default_rng(23)
    out = []
    for t in range(T):
        soft = softmax_planes(rng, P, h // 4, w // 4).repeat(4, 1).repeat(4, 2)
        flip = rng.random((h, w)) < 0.06
        soft[:, flip] = np.roll(soft, 1, axis=0)[:, flip]
        buf = torch.full((P, h + 3, w + 8), 7.0)
        buf[:, 1:1 + h, 2:2 + w] = torch.from_numpy(soft)
        out.append(buf[:, 1:1 + h, 2:2 + w])
    return out


def _pngs(folder):
    return {f: np.array(Image.open(os.path.join(folder, f))) for f in sorted(os.listdir(folder)) if f.endswith('.png')}


THR = dict(min_region=4, fill_holes=4, region_connectivity=4)


def _model(planes):
    """{file: model(plane)}, summed counts"""
    out, total = {}, np.zeros(4, dtype=np.int64)
    for f, m in planes.items():
        out[f], c = R.region_filter(m, THR['min_region'], THR['fill_holes'], THR['region_connectivity'])
        total += c
    return out, total


def _totals(saver):
    r = saver.regions
    return [r['islands_removed'], r['pixels_cleared'], r['holes_filled'], r['pixels_filled']]


@pytest.mark.parametrize('egress', ['host', 'device'])
@pytest.mark.parametrize('resize', [False, True])
def test_saver_writes_the_filtered_plane(tmp_path, regions_executor, egress, resize):
    from cutie_amd.inference.utils.track_report import TrackReport
    probs = _frames()
    shape = (37, 61) if resize else None
    seen = []

    class Scorer:
        def add(self, frame_name, mask):
            seen.append((frame_name, mask.clone().numpy()))

        def finish(self):
            return 'done'
    runs = {}
    for name, kw in (('plain', {}), ('filtered', dict(THR, tracks=TrackReport(), scorer=Scorer()))):
        saver = _saver(str(tmp_path / name), egress=egress, **kw)
        assert saver.egress == egress
        kept = [p.clone() for p in probs]
        for t, p in enumerate(probs):
            saver.process(p, f'{t:05d}.jpg', resize_needed=resize, shape=shape)
        saver.end()
        assert all(torch.equal(a, b) for a, b in zip(kept, probs))           # the probabilities are the model's: untouched
        runs[name] = (saver, _pngs(str(tmp_path / name / 'vid')))
    plain, filtered = runs['plain'][1], runs['filtered'][1]
    want, total = _model(plain)
    assert sorted(filtered) == sorted(plain) == [f'{t:05d}.png' for t in range(3)]
    for f in plain:
        assert np.array_equal(filtered[f], want[f]), f
    assert (total > 0).all() and any(not np.array_equal(plain[f], want[f]) for f in plain)
    saver = runs['filtered'][0]
    assert _totals(saver) == total.tolist() and saver.regions['frames'] == 3
    assert (saver.regions['min_region'], saver.regions['fill_holes'], saver.regions['connectivity']) == (4, 4, 4)
    assert runs['plain'][0].regions is None
    H, W = shape or (24, 40)
    assert regions_executor.region_calls == [(H, W, 4, 4, 4)] * 3           # the plain run issued none
    # the scorer and the track report saw the plane that was written
    assert [n for n, _ in seen] == [f'{t:05d}.jpg' for t in range(3)] and saver.scores == 'done'
    for (n, m) in seen:
        assert np.array_equal(m, want[n[:-4] + '.png'])
    check_report_against_files(saver.tracks.as_dict(), str(tmp_path / 'filtered' / 'vid'))


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_merged_filters_the_merged_plane(tmp_path, regions_executor, egress):
    rng = np.random.default_rng(2)
    frames = []
    for t in range(2):
        base = softmax_planes(rng, 3, 6, 10)
        members = []
        for k in (3, 4):
            soft = base.repeat(k, 1).repeat(k, 2)
            flip = rng.random(soft.shape[1:]) < 0.08
            soft[:, flip] = np.roll(soft, 1, axis=0)[:, flip]
            members.append(torch.from_numpy(soft))
        frames.append(members)
    out = {}
    for name, kw in (('plain', {}), ('filtered', THR)):
        saver = _saver(str(tmp_path / name), egress=egress, **kw)
        for t, members in enumerate(frames):
            saver.process_merged(members, f'{t:05d}.jpg', (31, 47))
        saver.end()
        out[name] = (saver, _pngs(str(tmp_path / name / 'vid')))
    want, total = _model(out['plain'][1])
    for f in want:
        assert np.array_equal(out['filtered'][1][f], want[f]), f
    assert total[1] > 0 and _totals(out['filtered'][0]) == total.tolist()
    assert regions_executor.region_calls == [(31, 47, 4, 4, 4)] * 2


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_burst_strings_and_overlays_come_from_the_filtered_plane(tmp_path, regions_executor, egress):
    from cutie_amd.inference.utils import coco_rle
    probs = _frames(2)
    names = ['00000.jpg', '00001.jpg']
    for t, n in enumerate(names):
        Image.fromarray(np.random.default_rng(t).integers(0, 256, size=(24, 40, 3), dtype=np.uint8)).save(str(tmp_path / n), quality=95)
    runs = {}
    for name, kw in (('plain', {}), ('filtered', THR)):
        init = {'segmentations': [{}, {}], 'annotated_image_paths': names, 'seq_name': 'vid'}
        saver = _saver(str(tmp_path / name), egress=egress, dataset='burst-val', init_json=init, visualize=egress == 'host',
                       visualize_output_root=str(tmp_path / name / 'vis'), **kw)
        assert saver.egress == egress
        for t, p in enumerate(probs):
            saver.process(p, names[t], path_to_image=str(tmp_path / names[t]))
        saver.end()
        runs[name] = (saver, _pngs(str(tmp_path / name / 'vid')))
    want, total = _model(runs['plain'][1])
    assert total[1] > 0
    saver = runs['filtered'][0]
    for t, n in enumerate(names):
        plane = want[n[:-4] + '.png']
        assert np.array_equal(runs['filtered'][1][n[:-4] + '.png'], plane)
        strings = {oid: coco_rle.encode(plane == oid) for oid in (5, 3) if (plane == oid).any()}
        assert {k: v['rle'] for k, v in saver.segmentations[t].items()} == strings
    if egress == 'device':                                                   # (the host overlay needs the ids on the host: egress='host')
        return
    # the overlay of the filtered run = the overlay a plain saver writes for probabilities that argmax to the filtered plane
    ref = _saver(str(tmp_path / 'ref'), visualize=True, visualize_output_root=str(tmp_path / 'ref' / 'vis'))
    for t, n in enumerate(names):
        plane = torch.from_numpy(want[n[:-4] + '.png'].astype(np.int64))
        ref.process(torch.stack([(plane == v).float() for v in (0, 5, 3)]), n, path_to_image=str(tmp_path / n))
    ref.end()
    for n in names:
        a = open(tmp_path / 'filtered' / 'vis' / 'vid' / (n[:-4] + '.jpg'), 'rb').read()
        b = open(tmp_path / 'ref' / 'vis' / 'vid' / (n[:-4] + '.jpg'), 'rb').read()
        assert a == b, n


def test_saver_refusals_and_defaults(tmp_path, regions_executor):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    for kw in (dict(min_region=5), dict(fill_holes=5)):
        with pytest.raises(ValueError, match='use_long_id'):
            ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, processor=object(), **kw)
        with pytest.raises(ValueError, match='processor'):
            ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, **kw)
    with pytest.raises(ValueError, match='negative'):
        _saver(str(tmp_path / 'n'), min_region=-1)
    with pytest.raises(ValueError, match='region_connectivity'):
        _saver(str(tmp_path / 'n'), min_region=5, region_connectivity=6)
    # thresholds below 2: off -- no launch, no totals, and long ids / no processor are fine
    ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, min_region=1, fill_holes=0).end()
    for kw in ({}, dict(min_region=1, fill_holes=1)):
        saver = _saver(str(tmp_path / 'off'), **kw)
        saver.process(_frames(1)[0], '00000.jpg')
        saver.end()
        assert regions_executor.region_calls == [] and saver.regions is None


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
def _args(argv):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(argv)
    E.check_args(ap, args)
    return args


def test_the_switches_and_their_rules(tmp_path, capsys):
    base = ['--images', 'a', '--masks', 'b', '--output', 'c']
    a = _args(base)
    assert (a.min_region, a.fill_holes, a.region_connectivity) == (0, 0, 8)
    a = _args(base + ['--min-region', '30', '--fill-holes', '12', '--region-connectivity', '4'])
    assert (a.min_region, a.fill_holes, a.region_connectivity) == (30, 12, 4)
    for bad in (['--min-region', '-1'], ['--fill-holes', '-2'], ['--region-connectivity', '6']):
        with pytest.raises(SystemExit) as e:
            _args(base + bad)
        assert e.value.code == 2
    capsys.readouterr()
    rgb = tmp_path / 'long' / 'v'
    os.makedirs(rgb)
    Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(rgb / '00000.png')
    with pytest.raises(SystemExit) as e:
        _args(['--images', 'a', '--masks', str(tmp_path / 'long'), '--output', 'c', '--fill-holes', '9'])
    assert e.value.code == 2 and 'long-id' in capsys.readouterr().err
    _args(['--images', 'a', '--masks', str(tmp_path / 'long'), '--output', 'c', '--fill-holes', '1'])      # off: nothing to refuse
    from cutie_amd import process_video as PV
    a = PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c', '--min-region', '7', '--fill-holes', '8', '--region-connectivity', '4'])
    assert (a.min_region, a.fill_holes, a.region_connectivity) == (7, 8, 4)
    a = PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c'])
    assert (a.min_region, a.fill_holes, a.region_connectivity) == (0, 0, 8)


@pytest.fixture(scope='module')
def bike_dataset(tmp_path_factory):
    """the tests/golden/bike frames as two videos of one dataset, and as a dataset of one video"""
    root = str(tmp_path_factory.mktemp('regions'))
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


def test_eval_vos_alone_and_in_lock_step(bike_dataset, capsys):
    """eval_vos --min-region --fill-holes on the bike example (run at --size 48): the files equal the model applied to the files of the run
    without the options, the totals are reported, and two copies of the clip in lock step get the files the clip gets alone."""
    from mock_exec_regions import RegionsMockExecutor
    from cutie_amd import eval_vos as E
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    ex = RegionsMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    try:
        net = CUTIE(default_config())
        net.load_weights(make_state_dict(seed=0))
        root, one = bike_dataset, os.path.join(bike_dataset, 'one')
        common = lambda base, out: ['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out, '--size', '48']
        plain_out = os.path.join(root, 'out_plain')
        E.run_dataset(net, default_config(), _args(common(one, plain_out)))
        assert ex.region_calls == []                                         # off: no launch
        plain = _pngs(os.path.join(plain_out, 'Annotations', 'bikeA'))
        island, hole = smallest_components(list(plain.values()), 8)
        thr = ['--min-region', str(max(island + 1, 40)), '--fill-holes', str(max((hole or 0) + 1, 40))]
        min_region, fill_holes = int(thr[1]), int(thr[3])
        want, total = {}, np.zeros(4, dtype=np.int64)
        for f, m in plain.items():
            want[f], c = R.region_filter(m, min_region, fill_holes, 8)
            total += c
        assert total[0] > 0
        files = {}
        for name, base, extra in (('alone', one, []), ('lockstep', root, ['--lockstep', '2'])):
            out = os.path.join(root, 'out_' + name)
            res = E.run_dataset(net, default_config(), _args(common(base, out) + thr + extra))
            for r in res.values():
                assert r['frames'] == 3
                got = r['regions']
                assert [got['islands_removed'], got['pixels_cleared'], got['holes_filled'], got['pixels_filled']] == total.tolist()
                assert (got['frames'], got['min_region'], got['fill_holes'], got['connectivity']) == (3, min_region, fill_holes, 8)
            for video in os.listdir(os.path.join(out, 'Annotations')):
                files[name, video] = _pngs(os.path.join(out, 'Annotations', video))
        assert sorted(files) == [('alone', 'bikeA'), ('lockstep', 'bikeA'), ('lockstep', 'bikeB')]
        for key, got in files.items():
            assert sorted(got) == sorted(want)
            for f in want:
                assert np.array_equal(got[f], want[f]), (key, f)
        assert len(ex.region_calls) == 9 and all(c == (480, 854, min_region, fill_holes, 8) for c in ex.region_calls)
    finally:
        _lib.set_executor_for_testing(None)
