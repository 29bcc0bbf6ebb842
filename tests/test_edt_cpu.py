"""The distance stage without a GPU: the numpy model of the contract (tests/edt_ref.py) against scipy.ndimage -- the exact transform with
indices, binary dilation and erosion by the disk --, the conventions of the contract on hand-made planes, the descriptor and the argument
checks of OpList.edt_band, and the wiring: through the interpreter (tests/mock_exec_edt.py) every path of a ResultSaver with trimap /
trimap_objects / dilate_mask -- host and device egress, the merged plane, behind the region filter, with target_objects, with an object
that joins mid-video -- writes the model applied to the id plane of the mask PNG next to it, and changes neither the mask PNGs nor the
probabilities; eval_vos and process_video write the same files for a clip alone and for two copies of it in lock step."""
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

import edt_ref as R
import region_ref
from test_track_report_cpu import softmax_planes

HERE = os.path.dirname(os.path.abspath(__file__))
DENSITIES = (0.002, 0.05, 0.5, 0.95, 0.998)
LIMITS = (1, 2, 26, 65026, 65536)                # 65026 = 255^2 + 1: radius 255 exactly
SETS3 = R.sets_of([1], [1, 2], [2])              # ids 1 and 2 are in two sets, id 3 (and 0) in none
SIZES = [(1, 1), (1, 37), (37, 1), (7, 5), (64, 64), (65, 129)]


def noise(rng, H, W, density):
    """three ids: a pixel is an object's with probability ``density`` -- object 1, 2 (three in ten) or 3 (one in ten) -- else background"""
    ids = (rng.random((H, W)) < density).astype(np.uint8)
    pick = rng.random((H, W))
    ids[(ids != 0) & (pick < 0.4)] = 2
    ids[(ids != 0) & (pick < 0.1)] = 3
    return ids


# ---- scipy restatements -----------------------------------------------------------------------------------------------------------------------
def scipy_dist2(F, limit):
    """min(limit, integer squared distance to the nearest pixel of the other class) from the indices of scipy's exact transform"""
    H, W = F.shape
    out = np.full((H, W), limit, dtype=np.int64)
    yy, xx = np.mgrid[:H, :W]
    for cls in (True, False):                    # the pixels of class cls look for the nearest pixel of the other class
        if (F == cls).all() or (F != cls).all():
            continue
        idx = ndimage.distance_transform_edt(F == cls, return_distances=False, return_indices=True)
        d = (idx[0] - yy) ** 2 + (idx[1] - xx) ** 2
        out[F == cls] = np.minimum(d[F == cls], limit)
    return out


def disk(r):
    k = int(np.floor(r))
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return yy * yy + xx * xx <= r * r


@pytest.mark.parametrize('H,W', SIZES)
def test_model_equals_scipy_transform(H, W):
    rng = np.random.default_rng(H * 1009 + W)
    for density in DENSITIES:
        ids = noise(rng, H, W, density)
        for limit in LIMITS:
            dist2, band = R.edt_band(ids, SETS3, min(4, limit - 1), min(25, limit - 1), 128, limit)
            assert dist2.dtype == np.int32 and band.dtype == np.uint8 and dist2.shape == band.shape == (3, H, W)
            for s in range(3):
                F = SETS3[s][ids] != 0
                assert np.array_equal(dist2[s], scipy_dist2(F, limit)), (density, limit, s)
                assert dist2[s].min() >= 1 and dist2[s].max() <= limit


@pytest.mark.parametrize('H,W', SIZES)
def test_model_equals_scipy_morphology(H, W):
    rng = np.random.default_rng(H * 31 + W)
    for density in DENSITIES:
        ids = noise(rng, H, W, density)
        for r in (1.0, 1.5, 2.0, 3.3, 5.0):
            t = int(np.floor(r * r))
            for s in range(3):
                F = SETS3[s][ids] != 0
                dilated = R.edt_band(ids, SETS3[s:s + 1], 0, t, 255, t + 1)[1][0]
                assert np.array_equal(dilated == 255, ndimage.binary_dilation(F, structure=disk(r))) and set(np.unique(dilated)) <= {0, 255}
                eroded = R.edt_band(ids, SETS3[s:s + 1], t, 0, 0, t + 1)[1][0]
                # border_value=1: nothing exists outside the frame, so nothing is eroded from there
                assert np.array_equal(eroded == 255, ndimage.binary_erosion(F, structure=disk(r), border_value=1)) and set(np.unique(eroded)) <= {0, 255}


# ---- conventions -------------------------------------------------------------------------------------------------------------------------------
def test_conventions_of_the_contract():
    rng = np.random.default_rng(1)
    ids = noise(rng, 30, 50, 0.5)
    # an empty and a full set: no pixel of the other class, D = limit
    for limit in (1, 26, 65536):
        d, b = R.edt_band(ids, R.sets_of([], range(256), [9]), 0, 0, 128, limit)
        assert (d == limit).all() and (b[0] == 0).all() and (b[1] == 255).all() and (b[2] == 0).all()
    # inner = 0 erodes nothing, outer = 0 dilates nothing: D >= 1 everywhere
    d, b = R.edt_band(ids, SETS3, 0, 0, 77, 1)
    for s in range(3):
        assert np.array_equal(b[s], np.where(SETS3[s][ids] != 0, 255, 0))
    assert (d == 1).all()                        # limit = 1: every distance is capped to it
    # a 3-4-5 pair
    ids = np.zeros((12, 12), dtype=np.uint8)
    ids[2, 3] = 4
    sets = R.sets_of([4])
    d, b = R.edt_band(ids, sets, 0, 24, 128, 26)
    assert d[0][6, 6] == 25 and b[0][6, 6] == 0 and d[0][2, 3] == 1 and b[0][2, 3] == 255 and d[0][11, 11] == 26
    assert R.edt_band(ids, sets, 0, 25, 128, 26)[1][0][6, 6] == 128
    assert R.edt_band(ids, sets, 0, 24, 128, 25)[0][0][6, 6] == 25          # capped: 25 then means "25 or more"
    # nothing exists outside the frame: an object that fills a border strip is eroded from inside only
    ids = np.zeros((9, 9), dtype=np.uint8)
    ids[:, :4] = 1
    d, b = R.edt_band(ids, R.sets_of([1]), 4, 0, 128, 100)
    assert d[0][:, 0].tolist() == [16] * 9 and d[0][:, 3].tolist() == [1] * 9 and d[0][0, 8] == 25
    assert (b[0][:, :2] == 255).all() and (b[0][:, 2:4] == 128).all() and (b[0][:, 4:] == 0).all()
    # an id in two sets and an id in none
    ids = np.array([[1, 2, 3, 0, 0]], dtype=np.uint8)
    d, b = R.edt_band(ids, SETS3, 0, 1, 128, 10)
    assert d.tolist() == [[[1, 1, 4, 9, 10]], [[4, 1, 1, 4, 9]], [[1, 1, 1, 4, 9]]]
    assert b.tolist() == [[[255, 128, 0, 0, 0]], [[255, 255, 128, 0, 0]], [[128, 255, 128, 0, 0]]]


# ---- the op --------------------------------------------------------------------------------------------------------------------------------
def test_edt_band_descriptor_and_argument_checks():
    from mock_exec_edt import EdtMockExecutor
    _lib.set_executor_for_testing(EdtMockExecutor())
    try:
        assert O.OpList.EDT_MAX_LIMIT == 65536 and O.OpList.EDT_MAX_SETS >= 16 and O.OpList.edt_scratch_words(3, 5, 7) == 53
        ids = torch.zeros((5, 7), dtype=torch.uint8)
        sets = torch.from_numpy(SETS3.copy())
        scratch = torch.zeros(60, dtype=torch.int32)
        band = torch.zeros((3, 5, 7), dtype=torch.uint8)
        dist2 = torch.zeros((3, 5, 7), dtype=torch.int32)
        ol = O.OpList()
        ol.edt_band(ids, sets, scratch, band=band)
        ol.edt_band(ids, sets, scratch, dist2=dist2, band=band, inner=4, outer=25, mid=7, limit=300)
        ol.edt_band(ids, sets, scratch, dist2=dist2, inner=9, outer=3)
        arr = ol.finalize()
        assert arr['kind'].tolist() == [O.PROB_TO_ID] * 3 and arr['flags'].tolist() == [4096] * 3
        assert arr['i'][0, :10].tolist() == [0, 5, 7, 0, 0, 1, 128, 0, 60, 3]                   # limit defaults to max(inner, outer) + 1
        assert arr['i'][1, :10].tolist() == [0, 5, 7, 4, 25, 300, 7, 0, 60, 3]
        assert arr['i'][2, :10].tolist() == [0, 5, 7, 9, 3, 10, 128, 0, 60, 3]
        assert arr['p'][1, 2] == ids.data_ptr() and arr['p'][1, 3] == band.data_ptr() and arr['p'][1, 5] == scratch.data_ptr()
        assert arr['p'][1, 6] == sets.data_ptr() and arr['p'][1, 7] == dist2.data_ptr()
        assert [int(arr['p'][1, k]) for k in (0, 1, 4)] == [0] * 3 and arr['p'][0, 7] == 0 and arr['p'][2, 3] == 0
        good = dict(ids_plane=ids, sets=sets, scratch=scratch, band=band, dist2=dist2, inner=4, outer=25)
        many = torch.zeros((O.OpList.EDT_MAX_SETS + 1, 256), dtype=torch.uint8)
        for change, msg in ((dict(ids_plane=ids.int()), 'uint8'), (dict(ids_plane=torch.zeros((5, 8), dtype=torch.uint8)[:, :7]), 'contiguous'),
                            (dict(ids_plane=torch.zeros((2, 5, 7), dtype=torch.uint8)), 'uint8'), (dict(ids_plane=torch.zeros((0, 7), dtype=torch.uint8)), 'H, W >= 1'),
                            (dict(sets=sets.int()), r'uint8 \[S, 256\]'), (dict(sets=sets[:, :255]), r'uint8 \[S, 256\]'), (dict(sets=sets[0]), r'uint8 \[S, 256\]'),
                            (dict(sets=sets[:0]), '0 sets'), (dict(sets=many), f'{O.OpList.EDT_MAX_SETS + 1} sets'),
                            (dict(inner=-1), 'not negative'), (dict(outer=-3), 'not negative'), (dict(limit=25), 'limit 25'), (dict(inner=26, limit=26), 'limit 26'),
                            (dict(limit=65537), 'limit 65537'), (dict(outer=65536), 'limit 65537'), (dict(mid=256), 'mid 256'), (dict(mid=-1), 'mid -1'),
                            (dict(band=None, dist2=None), 'band, dist2 or both'), (dict(band=band[:2]), 'band is a contiguous'), (dict(band=band.int()), 'band is a contiguous'),
                            (dict(dist2=dist2.float()), 'dist2 is a contiguous'), (dict(dist2=torch.zeros((3, 5, 8), dtype=torch.int32)[:, :, :7]), 'dist2 is a contiguous'),
                            (dict(scratch=scratch[:52]), 'at least 53 words'), (dict(scratch=scratch.float()), 'int32'),
                            (dict(sets=sets.to('meta')), 'is on meta')):
            with pytest.raises(ValueError, match=msg):
                O.OpList().edt_band(**dict(good, **change))
        # the interpreter runs the model
        rng = np.random.default_rng(3)
        plane = noise(rng, 12, 17, 0.3)
        t = torch.from_numpy(plane.copy())
        band, dist2 = torch.zeros((3, 12, 17), dtype=torch.uint8), torch.zeros((3, 12, 17), dtype=torch.int32)
        ol = O.OpList()
        ol.edt_band(t, sets, torch.zeros(O.OpList.edt_scratch_words(3, 12, 17), dtype=torch.int32), band=band, dist2=dist2, inner=1, outer=5, limit=50)
        ol.run()
        want = R.edt_band(plane, SETS3, 1, 5, 128, 50)
        assert np.array_equal(dist2.numpy(), want[0]) and np.array_equal(band.numpy(), want[1]) and np.array_equal(t.numpy(), plane)
    finally:
        _lib.set_executor_for_testing(None)


def test_a_stale_library_is_named(monkeypatch):
    monkeypatch.setattr(_lib, 'has_edt_band', lambda: False)
    _lib.set_executor_for_testing(None)
    with pytest.raises(_lib.HipLibraryError, match='no distance transform'):
        O.OpList().edt_band(torch.zeros((5, 7), dtype=torch.uint8), torch.zeros((1, 256), dtype=torch.uint8), torch.zeros(70, dtype=torch.int32),
                            band=torch.zeros((1, 5, 7), dtype=torch.uint8))


# ---- what the files must hold ------------------------------------------------------------------------------------------------------------------
def check_outputs_against_masks(folder, files, *, trimap=None, dilate=0.0, per_object=False, targets=None, objects=None):
    """Every trimap / dilated / trimap_objects PNG under ``folder`` = the model applied to the id plane of the mask PNG of the same name in
    ``folder``.  ``targets``: the ids of the union (default: every object, i.e. every non-zero id).  ``objects``: {file: the frame's object
    ids} (default: whatever has a folder, which must cover the ids on the plane).  -> the byte values seen in the trimaps."""
    seen = set()
    for f in files:
        plane = np.array(Image.open(os.path.join(folder, f)))
        assert plane.dtype == np.uint8 and plane.ndim == 2
        union = R.sets_of(range(1, 256) if targets is None else targets)
        if trimap is not None:
            inner, outer = int(trimap[0] * trimap[0]), int(trimap[1] * trimap[1])
            img = Image.open(os.path.join(folder, 'trimap', f))
            assert img.mode == 'L'
            got = np.array(img)
            assert np.array_equal(got, R.edt_band(plane, union, inner, outer, 128, max(inner, outer) + 1)[1][0]), ('trimap', f)
            seen |= set(np.unique(got).tolist())
            if per_object:
                base = os.path.join(folder, 'trimap_objects')
                have = sorted(int(d) for d in os.listdir(base) if os.path.exists(os.path.join(base, d, f))) if os.path.isdir(base) else []
                assert set(np.unique(plane).tolist()) - {0} <= set(have)
                if objects is not None:
                    assert have == sorted(objects[f]), (f, have)
                for oid in have:
                    got = np.array(Image.open(os.path.join(base, str(oid), f)))
                    assert np.array_equal(got, R.edt_band(plane, R.sets_of([oid]), inner, outer, 128, max(inner, outer) + 1)[1][0]), ('object', oid, f)
            else:
                assert not os.path.exists(os.path.join(folder, 'trimap_objects'))
        else:
            assert not os.path.exists(os.path.join(folder, 'trimap')) and not os.path.exists(os.path.join(folder, 'trimap_objects'))
        if dilate > 0.0:
            outer = int(dilate * dilate)
            img = Image.open(os.path.join(folder, 'dilated', f))
            got = np.array(img)
            assert img.mode == 'L' and np.array_equal(got, R.edt_band(plane, union, 0, outer, 255, outer + 1)[1][0]), ('dilated', f)
            assert set(np.unique(got).tolist()) <= {0, 255}
        else:
            assert not os.path.exists(os.path.join(folder, 'dilated'))
    return seen


# ---- host wiring -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def edt_executor():
    from mock_exec_edt import EdtMockExecutor
    ex = EdtMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    yield ex
    _lib.set_executor_for_testing(None)


def _saver(out, objects=(5, 3), **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    om.add_new_objects(list(objects))

    def to_mask(prob, dtype=torch.int64):
        lut = [0] * prob.shape[0]
        for t, o in om.tmp_id_to_obj.items():
            lut[t] = o.id
        return torch.tensor(lut)[prob.argmax(0)].to(dtype)
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om, output_prob_to_mask=to_mask)
    kw.setdefault('dataset', 'generic')
    return ResultSaver(out, 'vid', object_manager=om, use_long_id=False, processor=proc, **kw)


def _frames(T=3, P=3, h=24, w=40, seed=23):
    """speckled probabilities: blocky planes with single samples flipped, as un-padded views of padded buffers"""
    rng = np.random.default_rng(seed)
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


NAMES = [f'{t:05d}.png' for t in range(3)]
ON = dict(trimap=(1.5, 2.3), dilate_mask=3.0, trimap_objects=True)
THR = dict(min_region=4, fill_holes=4, region_connectivity=4)


@pytest.mark.parametrize('egress', ['host', 'device'])
@pytest.mark.parametrize('resize', [False, True])
@pytest.mark.parametrize('filtered', [False, True])
def test_saver_writes_the_models_files(tmp_path, edt_executor, egress, resize, filtered):
    probs = _frames()
    shape = (37, 61) if resize else None
    extra = THR if filtered else {}
    runs = {}
    for name, kw in (('plain', {}), ('bands', ON)):
        saver = _saver(str(tmp_path / name), egress=egress, **extra, **kw)
        assert saver.egress == egress
        kept = [p.clone() for p in probs]
        for t, p in enumerate(probs):
            saver.process(p, f'{t:05d}.jpg', resize_needed=resize, shape=shape)
        saver.end()
        assert all(torch.equal(a, b) for a, b in zip(kept, probs))           # the probabilities are untouched
        runs[name] = _pngs(str(tmp_path / name / 'vid'))
        if name == 'plain':
            assert edt_executor.edt_calls == [] and sorted(os.listdir(tmp_path / name / 'vid')) == NAMES      # off: no launch, no folder
    assert sorted(runs['bands']) == NAMES and all(np.array_equal(runs['bands'][f], runs['plain'][f]) for f in NAMES)  # the mask PNGs are the same
    if filtered:                                 # ... and they are the filtered planes: the distances are measured behind the filter
        raw = _saver(str(tmp_path / 'raw'), egress=egress)
        for t, p in enumerate(probs):
            raw.process(p, f'{t:05d}.jpg', resize_needed=resize, shape=shape)
        raw.end()
        raw = _pngs(str(tmp_path / 'raw' / 'vid'))
        assert any(not np.array_equal(raw[f], runs['bands'][f]) for f in NAMES)
        assert all(np.array_equal(region_ref.region_filter(raw[f], 4, 4, 4)[0], runs['bands'][f]) for f in NAMES)
    seen = check_outputs_against_masks(str(tmp_path / 'bands' / 'vid'), NAMES, trimap=ON['trimap'], dilate=3.0, per_object=True,
                                       objects={f: [5, 3] for f in NAMES})
    assert seen == {0, 128, 255}
    H, W = shape or (24, 40)
    assert edt_executor.edt_calls == [(H, W, 3, 2, 5, 6, 128), (H, W, 1, 0, 9, 10, 255)] * 3     # floor(r^2); the union and two objects; the dilation


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_merged_gets_the_files(tmp_path, edt_executor, egress):
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
    for name, kw in (('plain', {}), ('bands', dict(trimap=(2, 1), dilate_mask=1.0))):
        saver = _saver(str(tmp_path / name), egress=egress, **kw)
        for t, members in enumerate(frames):
            saver.process_merged(members, f'{t:05d}.jpg', (31, 47))
        saver.end()
        out[name] = _pngs(str(tmp_path / name / 'vid'))
    assert sorted(out['plain']) == NAMES[:2] and all(np.array_equal(out['plain'][f], out['bands'][f]) for f in NAMES[:2])
    assert check_outputs_against_masks(str(tmp_path / 'bands' / 'vid'), NAMES[:2], trimap=(2, 1), dilate=1.0) == {0, 128, 255}
    assert edt_executor.edt_calls == [(31, 47, 1, 4, 1, 5, 128), (31, 47, 1, 0, 1, 2, 255)] * 2


def test_target_objects_and_single_outputs(tmp_path, edt_executor):
    probs = _frames()
    for name, kw, check in (('targets', dict(trimap=(1, 2), dilate_mask=2.0, target_objects=[3, 99]), dict(trimap=(1, 2), dilate=2.0, targets=[3])),
                            ('none of them', dict(trimap=(1, 2), target_objects=[99]), dict(trimap=(1, 2), targets=[])),
                            ('trimap only', dict(trimap=(0, 2.5)), dict(trimap=(0, 2.5))),
                            ('dilated only', dict(dilate_mask=0.5), dict(dilate=0.5)),
                            ('per object, targets', dict(trimap=(1, 1), trimap_objects=True, target_objects=[5]), dict(trimap=(1, 1), per_object=True, targets=[5]))):
        saver = _saver(str(tmp_path / name), **kw)
        for t, p in enumerate(probs):
            saver.process(p, f'{t:05d}.jpg')
        saver.end()
        seen = check_outputs_against_masks(str(tmp_path / name / 'vid'), NAMES, **check)
        if name == 'none of them':               # a frame without a target object still gets its all-zero files
            assert seen == {0}
    assert np.array_equal(np.array(Image.open(tmp_path / 'dilated only' / 'vid' / 'dilated' / NAMES[0])) != 0,
                          np.array(Image.open(tmp_path / 'dilated only' / 'vid' / NAMES[0])) != 0)         # floor(0.25) = 0 dilates nothing


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_an_object_joins_mid_video(tmp_path, edt_executor, egress):
    saver = _saver(str(tmp_path / 'out'), egress=egress, **ON)
    first, later = _frames(2, P=3), _frames(2, P=4, seed=5)
    objects = {}
    for t, p in enumerate(first + later):
        if t == 2:
            saver.object_manager.add_new_objects([7])
        saver.process(p, f'{t:05d}.jpg')
        objects[f'{t:05d}.png'] = [5, 3] if t < 2 else [5, 3, 7]
    saver.end()
    folder = str(tmp_path / 'out' / 'vid')
    assert check_outputs_against_masks(folder, sorted(objects), trimap=ON['trimap'], dilate=3.0, per_object=True, objects=objects) == {0, 128, 255}
    assert sorted(os.listdir(os.path.join(folder, 'trimap_objects', '7'))) == ['00002.png', '00003.png']
    assert (np.array(Image.open(os.path.join(folder, '00003.png'))) == 7).any()
    assert [c[2] for c in edt_executor.edt_calls] == [3, 1, 3, 1, 4, 1, 4, 1]


def test_more_objects_than_one_op_holds(tmp_path, edt_executor):
    n = O.OpList.EDT_MAX_SETS + 3
    objects = list(range(1, n + 1))
    saver = _saver(str(tmp_path / 'out'), objects=objects, trimap=(1, 1), trimap_objects=True)
    rng = np.random.default_rng(8)
    soft = softmax_planes(rng, n + 1, 5, 8).repeat(2, 1).repeat(2, 2)
    saver.process(torch.from_numpy(soft), '00000.jpg')
    saver.end()
    check_outputs_against_masks(str(tmp_path / 'out' / 'vid'), NAMES[:1], trimap=(1, 1), per_object=True, objects={NAMES[0]: objects})
    assert [c[2] for c in edt_executor.edt_calls] == [O.OpList.EDT_MAX_SETS, n + 1 - O.OpList.EDT_MAX_SETS]


def test_saver_refusals_and_off_switches(tmp_path, edt_executor):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    for kw in (dict(trimap=(1, 2)), dict(dilate_mask=2)):
        with pytest.raises(ValueError, match='use_long_id'):
            ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, processor=object(), **kw)
        with pytest.raises(ValueError, match='processor'):
            ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, **kw)
    for kw, msg in ((dict(trimap=(-1, 2)), '0 .. 255'), (dict(trimap=(1, 255.5)), '0 .. 255'), (dict(dilate_mask=256), '0 .. 255'), (dict(dilate_mask=-0.1), '0 .. 255'),
                    (dict(dilate_mask=float('nan')), '0 .. 255'), (dict(trimap=(1, 2, 3)), r'\(r_in, r_out\)'), (dict(trimap_objects=True), 'needs trimap'),
                    (dict(trimap=(0, 0), trimap_objects=True), 'needs trimap')):
        with pytest.raises(ValueError, match=msg):
            _saver(str(tmp_path / 'n'), **kw)
    # off: no launch, no folder, and long ids / no processor are fine
    ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, trimap=(0, 0), dilate_mask=0.0).end()
    for kw in ({}, dict(trimap=None, dilate_mask=0), dict(trimap=(0.0, 0), trimap_objects=False)):
        saver = _saver(str(tmp_path / 'off'), **kw)
        saver.process(_frames(1)[0], '00000.jpg')
        saver.end()
        assert edt_executor.edt_calls == [] and sorted(os.listdir(tmp_path / 'off' / 'vid')) == NAMES[:1]
    _saver(str(tmp_path / 'edge'), trimap=(255, 255), dilate_mask=255.0).end()          # radius 255: 65025 < the largest limit


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
    assert (a.trimap, a.trimap_objects, a.dilate_mask) == (None, False, 0.0)
    a = _args(base + ['--trimap', '2', '5.5', '--trimap-objects', '--dilate-mask', '3'])
    assert (a.trimap, a.trimap_objects, a.dilate_mask) == ([2.0, 5.5], True, 3.0)
    for bad in (['--trimap', '2'], ['--trimap', '-1', '2'], ['--trimap', '1', '256'], ['--dilate-mask', '-2'], ['--dilate-mask', '300'], ['--trimap-objects'],
                ['--trimap', '0', '0', '--trimap-objects']):
        with pytest.raises(SystemExit) as e:
            _args(base + bad)
        assert e.value.code == 2
    capsys.readouterr()
    rgb = tmp_path / 'long' / 'v'
    os.makedirs(rgb)
    Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(rgb / '00000.png')
    for on in (['--trimap', '1', '2'], ['--dilate-mask', '2']):
        with pytest.raises(SystemExit) as e:
            _args(['--images', 'a', '--masks', str(tmp_path / 'long'), '--output', 'c'] + on)
        assert e.value.code == 2 and 'long-id' in capsys.readouterr().err
    _args(['--images', 'a', '--masks', str(tmp_path / 'long'), '--output', 'c', '--trimap', '0', '0'])      # off: nothing to refuse
    from cutie_amd import process_video as PV
    a = PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c', '--trimap', '1', '2', '--trimap-objects', '--dilate-mask', '4.5'])
    assert (a.trimap, a.trimap_objects, a.dilate_mask) == ([1.0, 2.0], True, 4.5)
    a = PV.arg_parser().parse_args(['-v', 'a', '-m', 'b', '-o', 'c'])
    assert (a.trimap, a.trimap_objects, a.dilate_mask) == (None, False, 0.0)


@pytest.fixture(scope='module')
def bike_dataset(tmp_path_factory):
    """the tests/golden/bike frames as two videos of one dataset, and as a dataset of one video"""
    root = str(tmp_path_factory.mktemp('edt'))
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


def _tree(folder):
    """{relative path: bytes} of every file under ``folder``"""
    out = {}
    for base, _, files in os.walk(folder):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), folder)] = open(os.path.join(base, f), 'rb').read()
    return out


OPTIONS = ['--trimap', '2', '5', '--dilate-mask', '3', '--trimap-objects']


def test_eval_vos_and_process_video_on_the_bike_example(bike_dataset):
    """eval_vos and process_video with --trimap 2 5 --dilate-mask 3 --trimap-objects on the bike example (run at --size 48): every new PNG is
    the model applied to the mask PNG next to it, the mask PNGs are those of the run without the options, which writes none of the new
    folders, and two copies of the clip in lock step get the files the clip gets alone."""
    from mock_exec_edt import EdtMockExecutor
    from cutie_amd import eval_vos as E
    from cutie_amd import process_video as PV
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    ex = EdtMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(ex)
    try:
        net = CUTIE(default_config())
        net.load_weights(make_state_dict(seed=0))
        root, one = bike_dataset, os.path.join(bike_dataset, 'one')
        common = lambda base, out: ['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--output', out, '--size', '48']
        plain_out = os.path.join(root, 'out_plain')
        E.run_dataset(net, default_config(), _args(common(one, plain_out)))
        assert ex.edt_calls == []                                            # off: no launch
        plain = _tree(os.path.join(plain_out, 'Annotations', 'bikeA'))
        assert sorted(plain) == NAMES
        trees = {}
        for name, base, extra in (('alone', one, []), ('lockstep', root, ['--lockstep', '2'])):
            out = os.path.join(root, 'out_' + name)
            res = E.run_dataset(net, default_config(), _args(common(base, out) + OPTIONS + extra))
            assert all(r['frames'] == 3 for r in res.values())
            for video in os.listdir(os.path.join(out, 'Annotations')):
                trees[name, video] = _tree(os.path.join(out, 'Annotations', video))
        assert sorted(trees) == [('alone', 'bikeA'), ('lockstep', 'bikeA'), ('lockstep', 'bikeB')]
        assert trees['lockstep', 'bikeA'] == trees['alone', 'bikeA'] and trees['lockstep', 'bikeB'] == trees['alone', 'bikeA']
        assert {f: trees['alone', 'bikeA'][f] for f in NAMES} == plain
        seen = check_outputs_against_masks(os.path.join(root, 'out_alone', 'Annotations', 'bikeA'), NAMES, trimap=(2, 5), dilate=3.0, per_object=True)
        assert seen == {0, 128, 255}
        assert len(ex.edt_calls) == 18 and all(c[:2] == (480, 854) for c in ex.edt_calls)
        # process_video: the same options on the same frames
        ex.edt_calls.clear()
        names = [f'{t:07d}.png' for t in range(3)]              # (process_video names its files by the frame number, seven digits)
        frames, masks = os.path.join(one, 'JPEGImages', 'bikeA'), os.path.join(one, 'Annotations', 'bikeA')
        cfg = PV.video_config(max_internal_size=48)
        PV.process_video(net, cfg, frames, masks, os.path.join(root, 'pv_plain'))
        assert ex.edt_calls == [] and sorted(os.listdir(os.path.join(root, 'pv_plain'))) == names
        PV.process_video(net, cfg, frames, masks, os.path.join(root, 'pv'), trimap=(2, 5), dilate_mask=3.0, trimap_objects=True)
        got = _tree(os.path.join(root, 'pv'))
        assert {f: got[f] for f in names} == _tree(os.path.join(root, 'pv_plain'))
        assert check_outputs_against_masks(os.path.join(root, 'pv'), names, trimap=(2, 5), dilate=3.0, per_object=True) == {0, 128, 255}
        assert len(ex.edt_calls) == 6
    finally:
        _lib.set_executor_for_testing(None)
