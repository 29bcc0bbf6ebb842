"""Device ingest on CPU (VideoReader(ingest='device') + device_ingest.to_device + the RESIZE flags 2 / 4 of ABI 5): the float64
reference of the antialiased resize against torch, the product's tap table against the reference's, and the whole driver wiring
under the torch interpreter of the descriptors -- device-ingest records and PNGs equal the host path's bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.utils.results_utils import davis_palette
from oracle.weights import make_state_dict

import aa_ref64
from mock_exec import MockExecutor, U8, F32, view

# (H, W, OH, OW): 1080p / 720p landscape and portrait to 480, scale ~1.002, odd -> 300, exact scale 4, a 17 x 9 source, an upscale
GEOMS = [(1080, 1920, 480, 853), (720, 1280, 480, 853), (1280, 720, 853, 480), (481, 640, 480, 638), (767, 1023, 300, 400),
         (480, 640, 120, 160), (9, 17, 4, 8), (9, 17, 20, 37)]


class IngestMock(MockExecutor):
    """The interpreter with RESIZE flags 2 / 4: CPU ToTensor (as VideoReader does it) + CPU F.interpolate(antialias=True)."""

    def _op_37(self, flags, i, f, p):
        if not flags & 6:
            return super()._op_37(flags, i, f, p)
        assert not flags & 1
        C, H, W, OH, OW, plane, ldrow = i[:7]
        if flags & 4:
            x = view(p[0], U8, (H, W, C), (ldrow, C, 1)).permute(2, 0, 1).float().div_(255.0)
        else:
            x = view(p[0], F32, (C, H, W), (plane, ldrow, 1)).clone()
        if flags & 2:
            x = F.interpolate(x[None], size=(OH, OW), mode='bilinear', align_corners=False, antialias=True)[0]
        else:
            assert (OH, OW) == (H, W)
        view(p[1], F32, (C, OH, OW)).copy_(x)


@pytest.fixture(scope='module')
def ingest_net():
    from cutie_amd.model.cutie import CUTIE
    mx = IngestMock()
    mx.per_sample_conv = True
    _lib.set_executor_for_testing(mx)
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net
    _lib.set_executor_for_testing(None)


@pytest.fixture
def mock_exec():
    _lib.set_executor_for_testing(IngestMock())
    yield
    _lib.set_executor_for_testing(None)


def _make_video(root, name, n=3, h=64, w=96, ids=(1, 3), seed=9):
    from cutie_amd.utils.synth import SyntheticClip
    clip = SyntheticClip(h, w, len(ids), n, seed=seed)
    os.makedirs(os.path.join(root, 'JPEGImages', name)); os.makedirs(os.path.join(root, 'Annotations', name))
    for t in range(n):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'JPEGImages', name, f'{t:05d}.jpg'), quality=95)
    lut = np.zeros(256, dtype=np.uint8)
    for k, oid in enumerate(ids):
        lut[k + 1] = oid
    png = Image.fromarray(lut[clip.first_mask().numpy()].astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'Annotations', name, '00000.png'))


def _dataset(root, **kw):
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    return VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False, **kw)


# ---- the float64 reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '%dx%d_%dx%d' % g)
def test_reference_bounds_torch(geom):
    H, W, OH, OW = geom
    g = torch.Generator().manual_seed(H * W)
    x = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g).float().div_(255.0)
    t = F.interpolate(x[None], size=(OH, OW), mode='bilinear', align_corners=False, antialias=True)[0].double().numpy()
    ref, bound = aa_ref64.resize_aa64(x.numpy(), OH, OW)
    assert float(bound.max()) <= aa_ref64.CEILING
    err = np.abs(t - ref)
    assert (err <= bound).all(), (float(err.max()), float(bound[err > bound].min()))


def test_reference_catches_a_shifted_tap():
    """The bound is tight enough to see a tap range off by one (what a wrong rounding of center / support does)."""
    x = torch.rand(3, 120, 160, generator=torch.Generator().manual_seed(1))
    ref, bound = aa_ref64.resize_aa64(x.numpy(), 50, 67)
    first, count, w = aa_ref64.taps(160, 67)
    A = np.zeros((67, 160))
    for i in range(67):
        lo = min(first[i] + 1, 160 - count[i])             # every range one column to the right
        A[i, lo:lo + count[i]] = w[i, :count[i]]
    Ay, _ = aa_ref64.matrix(120, 50)
    bad = np.einsum('yh,chw->cyw', Ay, x.double().numpy() @ A.T)
    assert (np.abs(bad - ref) > bound).mean() > 0.5


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '%dx%d_%dx%d' % g)
def test_product_tap_table_is_the_reference_filter(geom):
    H, W, OH, OW = geom
    tab = O.resize_aa_table(H, W, OH, OW)
    for rows, (n_in, n_out) in ((tab[:OW], (W, OW)), (tab[OW:], (H, OH))):
        first, count, w = aa_ref64.taps(n_in, n_out)
        assert np.array_equal(rows[:, 0], first) and np.array_equal(rows[:, 1], count)
        K = w.shape[1]
        assert np.array_equal(rows[:, 2:2 + K].view(np.float32), w) and not rows[:, 2 + K:].any()


def test_resize_arguments():
    ol = O.OpList(prio=False)
    with pytest.raises(ValueError):
        ol.resize(0, 0, C=3, H=4, W=4, OH=2, OW=2, plane=16, ldrow=4, nearest=True, antialias=True)
    with pytest.raises(ValueError):
        ol.resize(0, 0, C=3, H=4, W=4, OH=2, OW=2, plane=16, ldrow=4, antialias=True)
    tab = torch.from_numpy(O.resize_aa_table(4, 4, 2, 2))
    ol.resize(1, 2, C=3, H=4, W=4, OH=2, OW=2, plane=0, ldrow=12, antialias=True, src_u8=True, taps=tab, scratch=3)
    ol.resize(1, 2, C=3, H=4, W=4, OH=4, OW=4, plane=0, ldrow=12, src_u8=True)
    ol.resize(1, 2, C=3, H=4, W=4, OH=2, OW=2, plane=16, ldrow=4)
    arr = ol.finalize()
    assert arr['flags'].tolist() == [6, 4, 0] and arr['i'][0, 7] == tab.shape[1] - 2 and arr['p'][0, 2] == tab.data_ptr()


# ---- reader + to_device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [-1, 48])
def test_device_records_equal_host_records(tmp_path, mock_exec, size):
    from cutie_amd.inference.data.device_ingest import to_device
    _make_video(str(tmp_path), 'v', n=3, h=64, w=96)
    host = next(iter(_dataset(str(tmp_path), size=size).get_datasets()))
    dev = next(iter(_dataset(str(tmp_path), size=size, ingest='device').get_datasets()))
    assert host.ingest == 'host' and dev.ingest == 'device'
    for t in range(len(host)):
        h, d = host[t], dev[t]
        assert 'rgb' not in d and d['rgb_u8'].dtype == np.uint8 and d['rgb_u8'].shape == (64, 96, 3)
        assert d['info']['rgb_shape'] == tuple(h['rgb'].shape[-2:])
        d = to_device(d, 'cpu')
        assert set(d) == set(h) and set(d['info']) == set(h['info'])
        assert d['rgb'].dtype == torch.float32 and d['rgb'].is_contiguous()
        assert torch.equal(d['rgb'], h['rgb']), t
        for k in ('mask', 'valid_labels'):
            assert (k in d) == (k in h) and (k not in d or torch.equal(d[k], h[k]))
        assert d['info'] == h['info']
        assert dev.get(t, ingest='host')['rgb'].equal(h['rgb'])
    if size > 0:
        assert tuple(host[0]['rgb'].shape) == (3, 48, 72)


def test_invalid_ingest_raises(tmp_path):
    from cutie_amd.eval_vos import process_video
    from cutie_amd.inference.data.video_reader import VideoReader
    _make_video(str(tmp_path), 'v', n=2)
    root = str(tmp_path)
    with pytest.raises(ValueError):
        VideoReader('v', os.path.join(root, 'JPEGImages', 'v'), os.path.join(root, 'Annotations', 'v'), ingest='gpu')
    with pytest.raises(ValueError):
        _dataset(root, ingest='cuda')
    rd = next(iter(_dataset(root).get_datasets()))
    with pytest.raises(ValueError):
        rd.get(0, ingest='both')
    from cutie_amd.process_video import process_video as pv
    with pytest.raises(ValueError):
        pv(None, None, root, root, root, ingest='pinned')
    with pytest.raises(ValueError):
        process_video(_Net(), default_config(), rd, os.path.join(root, 'o'), ingest='Device')


class _Net:
    device = torch.device('cpu')


def test_lockstep_key_is_the_same_in_both_modes(tmp_path):
    from cutie_amd.eval_vos import lockstep_key
    _make_video(str(tmp_path), 'a', n=2, h=64, w=96, ids=(1, 3))
    _make_video(str(tmp_path), 'b', n=2, h=80, w=60, ids=(2,))
    for size in (-1, 48):
        keys = {m: [lockstep_key(rd) for rd in _dataset(str(tmp_path), size=size, ingest=m).get_datasets()] for m in ('host', 'device')}
        assert keys['host'] == keys['device']
    assert keys['device'] == [((48, 72), 2, False), ((64, 48), 1, False)]


# ---- the drivers ---------------------------------------------------------------------------------------------------------------
def _pngs(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), 'rb').read()
    return out


@pytest.mark.parametrize('size', [-1, 48])
def test_eval_driver_device_ingest_writes_the_host_pngs(tmp_path, ingest_net, size):
    from cutie_amd.eval_vos import process_video, process_videos_lockstep
    root = str(tmp_path)
    _make_video(root, 'vA', n=4, ids=(1, 2), seed=21)
    _make_video(root, 'vB', n=3, ids=(4, 9), seed=22)
    cfg = default_config(mem_every=2)
    with torch.inference_mode():
        for mode in ('host', 'device'):
            rds = list(_dataset(root, size=size, ingest=mode).get_datasets())
            for rd in rds:
                r = process_video(ingest_net, cfg, rd, os.path.join(root, 'alone_' + mode))
                assert r['frames'] == len(rd)
            process_videos_lockstep(ingest_net, cfg, rds, os.path.join(root, 'ls_' + mode))
        # the keyword overrides the reader's mode
        rd = next(iter(_dataset(root, size=size).get_datasets()))
        process_video(ingest_net, cfg, rd, os.path.join(root, 'kw'), ingest='device')
    host = _pngs(os.path.join(root, 'alone_host'))
    assert len(host) == 7
    assert _pngs(os.path.join(root, 'alone_device')) == host
    assert _pngs(os.path.join(root, 'ls_host')) == _pngs(os.path.join(root, 'ls_device'))
    assert _pngs(os.path.join(root, 'kw')) == {k: v for k, v in host.items() if k.startswith('vA')}


def test_process_video_device_ingest_writes_the_host_pngs(tmp_path, ingest_net):
    from cutie_amd.process_video import process_video, video_config
    from cutie_amd.utils.synth import SyntheticClip
    root = str(tmp_path)
    clip = SyntheticClip(64, 96, 2, 4, seed=5)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(4):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(clip.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    cfg = video_config(mem_every=2)
    out = {}
    for mode in ('host', 'device'):
        r = process_video(ingest_net, cfg, os.path.join(root, 'frames'), os.path.join(root, 'masks'), os.path.join(root, mode),
                          ingest=mode)
        assert r['frames'] == 4
        out[mode] = _pngs(os.path.join(root, mode))
    assert len(out['host']) == 4 and out['device'] == out['host']
