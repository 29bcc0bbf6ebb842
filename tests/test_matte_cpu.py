"""The visualisation modes, soft masks and alpha matte without a GPU (PROB_TO_ID flags == 256 / 512, ABI 11, forms added): the numpy model of the
stages (tests/matte_ref.py) writes the bytes of the reference's torch functions (tests/golden/matte/, tools/make_matte_golden.py), and
saver and driver -- run through the model -- write its frames and planes as the files the issue names."""
import glob
import io
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_enc_ref                                        # noqa: E402
import matte_ref as M                                      # noqa: E402
import png_ref                                             # noqa: E402
from test_jpeg_encode_cpu import OverlayMock              # noqa: E402

from cutie_amd import _lib, ops as O                       # noqa: E402
from cutie_amd.config import default_config               # noqa: E402
from cutie_amd.inference.utils import png as png_container  # noqa: E402
from cutie_amd.inference.utils import results_utils as RU  # noqa: E402
from cutie_amd.inference.utils.results_utils import davis_palette  # noqa: E402
from oracle.weights import make_state_dict                 # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'matte', '*.npz')))
INPUTS = ('frame', 'planes', 'layer', 'table')


def _cases(z):
    for k in z.files:
        if k in INPUTS or k in M.HARD_MODES:
            continue
        mode, *t = k.split('_')
        yield k, mode, ([] if t == ['none'] else [int(v) for v in t])


# ---- the model against the reference's bytes ------------------------------------------------------------------------------------------
def test_fixtures_cover_what_the_issue_lists():
    names = {os.path.basename(f) for f in GOLDEN}
    assert {f'm_{h}x{w}_p{p}.npz' for h, w in ((1, 1), (3, 5), (33, 47), (97, 131)) for p in (2, 4)} | {'m_clamp_9x14_p4.npz'} == names
    seen = set()
    for f in GOLDEN:
        z = np.load(f)
        seen |= {(mode, tuple(t)) for _, mode, t in _cases(z)} | {(k, ()) for k in z.files if k in M.HARD_MODES}
        assert os.path.getsize(f) < 1 << 20
    for mode in ('popup', 'layer', 'rgba'):
        assert {(mode, ()), (mode, (1,)), (mode, (1, 3)), (mode, (1, 2, 3))} <= seen
    assert {('davis', ()), ('light', ()), ('fade', ())} <= seen
    z = np.load([f for f in GOLDEN if 'clamp' in f][0])
    assert (z['planes'].astype(np.float32)[1:].sum(0) > 1).any()


@pytest.mark.parametrize('path', GOLDEN, ids=os.path.basename)
def test_model_equals_the_reference(path):
    z = np.load(path)
    frame, planes, layer = z['frame'], z['planes'].astype(np.float32), z['layer']
    n = 0
    for key, mode, targets in _cases(z):
        if mode == 'rgba':                                 # its first three channels are the frame, the fourth is the matte
            _, a = M.composite('alpha', planes=planes, targets=targets)
            got = np.concatenate([frame, a[..., None]], -1)
        else:
            got, _ = M.composite(mode, frame, planes, targets, layer_rgba=layer)
        assert got.dtype == np.uint8 and np.array_equal(got, z[key]), (key, int((got != z[key]).sum()))
        n += 1
    assert n >= 1


@pytest.mark.parametrize('path', [p for p in GOLDEN if 'clamp' not in p], ids=os.path.basename)
def test_hard_modes_equal_the_reference_on_the_argmax_plane(path):
    """overlay_davis_torch takes the argmax itself; the stage reads the id plane and a colour table: the argmax plane with the
    reference's colour map as an identity table (entry id = the map's colour of id) gives its bytes."""
    z = np.load(path)
    ids = z['planes'].astype(np.float32).argmax(0).astype(np.uint8)
    modes = [k for k in z.files if k in M.HARD_MODES]
    assert modes
    for mode in modes:
        got = M.hard(mode, z['frame'], ids, z['table'])
        assert np.array_equal(got, z[mode]), (mode, int((got != z[mode]).sum()))


def test_matte_with_a_frame_is_the_matte_alone_and_resampling_is_resizes_sample():
    import merge_ref
    rs = np.random.RandomState(4)
    planes = rs.rand(4, 17, 23).astype(np.float32)
    frame = rs.randint(0, 256, (33, 47, 3)).astype(np.uint8)
    out, a = M.composite('popup', frame, planes, [3, 1], out_hw=(33, 47), want_alpha=True)
    assert np.array_equal(a, M.composite('alpha', planes=planes, targets=[3, 1], out_hw=(33, 47))[1])
    full = merge_ref.resize(planes, 33, 47)
    assert np.array_equal(out, M.composite('popup', frame, full, [3, 1])[0])
    assert np.array_equal(M.soft(planes, 33, 47), merge_ref.quantise(full)[1:])      # the truncation of the multi-scale merge
    order = rs.rand(4, 64, 64).astype(np.float32) * np.float32(0.4)
    assert (M.target_sum(order, [3, 1, 2]) != M.target_sum(order, [1, 2, 3])).any()      # the order of the list is part of the result


# ---- the descriptors --------------------------------------------------------------------------------------------------------------------
def test_descriptors_of_the_matte_ops():
    """The slots sit where include/cutie_hip.h says (PROB_TO_ID, ABI 11, forms added)."""
    H, W, P = 21, 37, 4
    big = torch.zeros((H, 40, 3), dtype=torch.uint8)
    frame = big[:, :W]                                                        # a padded row stride
    store = torch.zeros((P, 12, 24))
    planes = store[:, :11, :19]                                               # the un-padded view of padded planes
    ids, colors = torch.zeros((H, W), dtype=torch.uint8), torch.zeros((256, 4), dtype=torch.uint8)
    layer, out = torch.zeros((H, W, 4), dtype=torch.uint8), torch.zeros((H, W, 3), dtype=torch.uint8)
    matte, softs = torch.zeros((H, W), dtype=torch.uint8), torch.zeros((P - 1, H, W), dtype=torch.uint8)
    ol = O.OpList()
    ol.matte_composite('fade', out, out_hw=(H, W), frame=frame, ids=ids, colors=colors)
    ol.matte_composite('layer', out, out_hw=(H, W), frame=frame, planes=planes, targets=[3, 1], layer=layer, matte=matte)
    ol.matte_composite('alpha', None, out_hw=(H, W), planes=planes, targets=[], matte=matte)
    ol.matte_soft(planes, softs, out_hw=(H, W))
    recs = ol.finalize()
    assert [int(r['kind']) for r in recs] == [O.PROB_TO_ID] * 4 and [int(r['flags']) for r in recs] == [256, 256, 256, 512]
    geo = (P, 11, 19, 12 * 24, 24, H, W)
    i, p = recs[0]['i'], [int(v) for v in recs[0]['p']]
    assert tuple(i[:7]) == (0, 0, 0, 0, 0, H, W) and (i[7], i[8], i[9]) == (120, 2, 0) and not i[10:].any()
    assert p[:8] == [0, 0, frame.data_ptr(), out.data_ptr(), 0, ids.data_ptr(), colors.data_ptr(), 0] and not any(p[8:])
    i, p = recs[1]['i'], [int(v) for v in recs[1]['p']]
    assert tuple(i[:7]) == geo and (i[7], i[8], i[9]) == (120, 4, 2) and not i[10:].any()
    assert p[0] == planes.data_ptr() and p[2:8] == [frame.data_ptr(), out.data_ptr(), matte.data_ptr(), 0, 0, layer.data_ptr()]
    import ctypes
    assert list((ctypes.c_int32 * 2).from_address(p[1])) == [3, 1]            # the target list: host memory, read by the launcher
    i, p = recs[2]['i'], [int(v) for v in recs[2]['p']]
    assert tuple(i[:7]) == geo and (i[7], i[8], i[9]) == (0, 5, 0) and p[:8] == [planes.data_ptr(), 0, 0, 0, matte.data_ptr(), 0, 0, 0]
    i, p = recs[3]['i'], [int(v) for v in recs[3]['p']]
    assert tuple(i[:7]) == geo and not i[7:].any() and p[:3] == [planes.data_ptr(), 0, softs.data_ptr()] and not any(p[3:])
    assert O.OpList.MATTE_MODES == M.MODE_CODES
    for bad in (dict(mode='rgba'), dict(targets=[4]), dict(targets=[-1]), dict(targets=[1] * 256), dict(planes=planes.double()),
                dict(frame=frame.float()), dict(layer=layer[:, :5]), dict(matte=matte[:, :5]), dict(layer=None)):
        kw = dict(mode='layer', out=out, out_hw=(H, W), frame=frame, planes=planes, targets=[1], layer=layer, matte=matte)
        kw.update(bad)
        with pytest.raises(ValueError):
            ol.matte_composite(kw.pop('mode'), kw.pop('out'), **kw)
    with pytest.raises(ValueError):
        ol.matte_composite('davis', out, out_hw=(H, W), frame=frame, ids=ids, colors=colors, matte=matte)
    with pytest.raises(ValueError):
        ol.matte_composite('davis', out, out_hw=(H, W), frame=frame, ids=None, colors=colors)
    with pytest.raises(ValueError):
        ol.matte_soft(planes, softs[:2], out_hw=(H, W))
    assert len(ol) == 4
    src = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'cutie_hip.h')).read()
    assert 'flags == 256' in src and 'flags == 512' in src and 'ABI 11, forms added' in src


# ---- saver arguments --------------------------------------------------------------------------------------------------------------------
def _saver(tmp_path, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    om = ObjectManager()
    om.add_new_objects([5, 3])
    if kw.pop('with_processor', True):
        kw['processor'] = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om)
    kw.setdefault('use_long_id', False)
    return RU.ResultSaver(str(tmp_path), 'vid', dataset='generic', object_manager=om, **kw)


def test_saver_arguments(tmp_path):
    assert RU.VIS_MODES == ('davis', 'light', 'fade', 'popup', 'layer')
    for kw in (dict(vis_modes=('popup',)), dict(soft_masks=True), dict(alpha_matte=True)):
        with pytest.raises(ValueError, match='use_long_id'):
            _saver(tmp_path, use_long_id=True, **kw)
        with pytest.raises(ValueError, match='processor'):
            _saver(tmp_path, with_processor=False, **kw)
    with pytest.raises(ValueError, match='vis_modes'):
        _saver(tmp_path, vis_modes=('rgba',))
    with pytest.raises(ValueError, match='vis_modes'):
        _saver(tmp_path, vis_modes=('fade', 'fade'))
    with pytest.raises(ValueError, match='layer'):
        _saver(tmp_path, vis_modes=('layer',))
    s = _saver(tmp_path, use_long_id=True)                                     # the defaults: nothing new is on
    try:
        assert s.vis_modes == () and not s.soft_masks and not s.alpha_matte
    finally:
        s.end()


def test_process_video_parser(capsys):
    from cutie_amd.process_video import arg_parser
    base = ['-v', 'v', '-m', 'm', '-o', 'o']
    a = arg_parser().parse_args(base)
    assert a.vis == [] and not a.soft_masks and not a.alpha and a.target_objects is None and a.layer is None
    a = arg_parser().parse_args(base + ['--vis', 'popup', 'layer', 'fade', '--soft-masks', '--alpha', '--target-objects', '2', '1', '--layer', 'l.png'])
    assert a.vis == ['popup', 'layer', 'fade'] and a.soft_masks and a.alpha and a.target_objects == [2, 1] and a.layer == 'l.png'
    for bad in (['--vis', 'rgba'], ['--vis'], ['--target-objects', 'one'], ['--target-objects'], ['--layer']):
        with pytest.raises(SystemExit):
            arg_parser().parse_args(base + bad)
    capsys.readouterr()


# ---- saver and driver through the model -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def matte_net():
    from cutie_amd.model.cutie import CUTIE
    mx = OverlayMock()
    mx.per_sample_conv = True
    mm = M.MatteExecutor(mx)
    _lib.set_executor_for_testing(jpeg_enc_ref.EncodeExecutor(mm))
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net, mm
    _lib.set_executor_for_testing(None)


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    from cutie_amd.utils.synth import SyntheticClip
    root = str(tmp_path_factory.mktemp('matte'))
    c = SyntheticClip(64, 96, 2, 3, seed=5)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(3):
        arr = (c.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(c.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    rs = np.random.RandomState(8)
    Image.fromarray(rs.randint(0, 256, (40, 50, 4)).astype(np.uint8), 'RGBA').save(os.path.join(root, 'layer.png'))
    return root


def _files(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), 'rb').read()
    return out


def _jpg(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', quality=75)
    return b.getvalue()


def _png(plane):
    return png_container.assemble(png_ref.encode(plane)[0], plane.shape[0], plane.shape[1], None)


def _expected(log, n, vis, soft, alpha, objects):
    """The files of n frames from the model's log: per frame one entry per mode, the matte alone when no soft mode carries it, the soft planes."""
    alone = alpha and not any(m in ('popup', 'layer') for m in vis)
    per = len(vis) + (1 if alone else 0) + (1 if soft else 0)
    assert len(log) == n * per
    want = {}
    for t in range(n):
        entries, name = log[t * per:(t + 1) * per], f'{t:07d}'
        mattes = 0
        for mode, e in zip(vis, entries):
            assert e[0] == mode and e[1] is not None
            want[f'visualization/{mode}/{name}.jpg'] = _jpg(e[1])
            if e[2] is not None:
                want[f'alpha/{name}.png'] = _png(e[2])
                mattes += 1
        rest = entries[len(vis):]
        if alone:
            assert rest[0][0] == 'alpha' and rest[0][1] is None
            want[f'alpha/{name}.png'] = _png(rest[0][2])
            mattes += 1
            rest = rest[1:]
        assert mattes == (1 if alpha else 0)
        if soft:
            assert rest[0][0] == 'soft' and len(rest[0][1]) == len(objects)
            for oid, plane in zip(objects, rest[0][1]):
                want[f'soft_masks/{oid}/{name}.png'] = _png(plane)
    return want


def _run(matte_net, clip, out, **kw):
    from cutie_amd.process_video import process_video, video_config
    net, mm = matte_net
    mm.log.clear()
    r = process_video(net, video_config(mem_every=2), os.path.join(clip, 'frames'), os.path.join(clip, 'masks'), out, **kw)
    assert r['frames'] == 3
    return r, list(mm.log)


@pytest.fixture(scope='module')
def plain(matte_net, clip):
    """A run with none of the new arguments: the mask PNGs and nothing else."""
    out = os.path.join(clip, 'plain')
    r, log = _run(matte_net, clip, out)
    files = _files(out)
    assert sorted(files) == [f'{t:07d}.png' for t in range(3)] and not log and 'folders' not in r
    return files


@pytest.mark.parametrize('ingest', ['host', 'device'])
@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_video_writes_the_models_files(matte_net, clip, plain, ingest, egress):
    out = os.path.join(clip, f'all_{ingest}_{egress}')
    vis = ('popup', 'layer', 'fade')
    r, log = _run(matte_net, clip, out, ingest=ingest, egress=egress, vis_modes=vis, soft_masks=True, alpha_matte=True,
                  layer=os.path.join(clip, 'layer.png'))
    files = _files(out)
    want = _expected(log, 3, vis, True, True, (1, 2))
    masks = {k: v for k, v in files.items() if os.sep not in k}
    assert {k: v for k, v in files.items() if os.sep in k} == want and len(want) == 3 * (3 + 2 + 1)
    assert sorted(masks) == sorted(plain)
    if egress == 'host':
        assert masks == plain                                                 # the existing files, byte for byte
    else:
        assert all(np.array_equal(np.array(Image.open(io.BytesIO(masks[k]))), np.array(Image.open(io.BytesIO(plain[k])))) for k in plain)
    assert r['folders'] == [os.path.join(out, 'visualization', m) for m in vis] + [os.path.join(out, 'soft_masks'), os.path.join(out, 'alpha')]
    assert all(e[3] == [1, 2] for e in log if e[0] in ('popup', 'layer'))      # default targets: every object, as plane indices
    for k, v in want.items():                                                 # every .png decodes to the model's plane
        if k.endswith('.png'):
            im = Image.open(io.BytesIO(files[k]))
            assert im.mode == 'L' and im.size == (96, 64)
    t0 = log[0]
    assert t0[0] == 'popup' and t0[1].shape == (64, 96, 3) and np.array_equal(np.array(Image.open(io.BytesIO(files['alpha/0000000.png']))), t0[2])


def test_targets_modes_alone_and_ingest_agree(matte_net, clip, plain):
    """--target-objects picks the planes (in the order given, unknown ids left out); the hard modes alone read no planes; the matte
    alone is a launch of its own; host and device ingest hand the stage the same uint8 frame."""
    a, log_a = _run(matte_net, clip, os.path.join(clip, 't_host'), ingest='host', vis_modes=('davis', 'light'), alpha_matte=True, target_objects=[2, 7, 1])
    b, log_b = _run(matte_net, clip, os.path.join(clip, 't_dev'), ingest='device', vis_modes=('davis', 'light'), alpha_matte=True, target_objects=[2, 7, 1])
    fa, fb = _files(os.path.join(clip, 't_host')), _files(os.path.join(clip, 't_dev'))
    assert fa == fb
    want = _expected(log_a, 3, ('davis', 'light'), False, True, ())
    assert {k: v for k, v in fa.items() if os.sep in k} == want and {k: v for k, v in fa.items() if os.sep not in k} == plain
    assert all(e[3] == [2, 1] for e in log_a if e[0] == 'alpha') and [e[0] for e in log_a[:3]] == ['davis', 'light', 'alpha']
    assert a['folders'] == [os.path.join(clip, 't_host', 'visualization', 'davis'), os.path.join(clip, 't_host', 'visualization', 'light'),
                            os.path.join(clip, 't_host', 'alpha')]
    c, log_c = _run(matte_net, clip, os.path.join(clip, 't_soft'), soft_masks=True)
    assert {k: v for k, v in _files(os.path.join(clip, 't_soft')).items() if os.sep in k} == _expected(log_c, 3, (), True, False, (1, 2))


def test_overflow_is_encoded_on_the_host(matte_net, clip, plain, monkeypatch, caplog):
    monkeypatch.setattr(O.OpList, 'jpeg_enc_capacity', classmethod(lambda cls, H, W, worst=False: 64))
    out = os.path.join(clip, 'tiny')
    with caplog.at_level(logging.WARNING):
        r, log = _run(matte_net, clip, out, ingest='device', vis_modes=('popup', 'fade'))
    files = _files(out)
    assert {k: v for k, v in files.items() if os.sep in k} == _expected(log, 3, ('popup', 'fade'), False, False, ())
    warned = [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(warned) == 1 and 'device JPEG encoder' in warned[0].getMessage()


def _small_clip(root, h, w):
    from cutie_amd.utils.synth import SyntheticClip
    c = SyntheticClip(h, w, 2, 3, seed=7)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(3):
        arr = (c.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.png'))
    png = Image.fromarray(c.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    Image.fromarray(np.random.RandomState(8).randint(0, 256, (40, 50, 4)).astype(np.uint8), 'RGBA').save(os.path.join(root, 'layer.png'))
    return root


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_several_modes_on_a_size_whose_frames_are_no_multiple_of_16_bytes(matte_net, tmp_path, egress):
    """33 x 47 x 3 = 4653 bytes: frames packed behind each other would start at odd addresses, which the launcher refuses (and the
    model executor checks as the launcher does) -- every mode composes into a 16-byte aligned frame of its own."""
    root = _small_clip(str(tmp_path), 33, 47)
    vis = ('popup', 'fade', 'layer', 'davis', 'light')
    r, log = _run(matte_net, root, os.path.join(root, 'out'), ingest='device', egress=egress, vis_modes=vis, soft_masks=True, alpha_matte=True,
                  layer=os.path.join(root, 'layer.png'))
    files = _files(os.path.join(root, 'out'))
    want = _expected(log, 3, vis, True, True, (1, 2))
    assert {k: v for k, v in files.items() if os.sep in k} == want and len(want) == 3 * (5 + 2 + 1)
    assert log[0][1].shape == (33, 47, 3) and sorted(k for k in files if os.sep not in k) == [f'{t:07d}.png' for t in range(3)]
