"""The device overlay of --visualize on the MI355X (PROB_TO_ID flags == 128, ABI 11, csrc/jpeg_enc.hip): the kernel's entropy-coded
segment, wrapped, is PIL's file byte for byte; overlays equal PIL's encode of the host blend; overflow, refusals; the drivers write
the host overlay's .jpg bytes."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_enc_ref as R                                   # noqa: E402
from test_jpeg_encode_cpu import SIZES, content, pil_bytes   # noqa: E402

from cutie_amd import _lib, ops as O                       # noqa: E402
from cutie_amd.config import default_config               # noqa: E402
from cutie_amd.inference.utils import jpeg_writer as JW    # noqa: E402
from cutie_amd.inference.utils import results_utils as RU  # noqa: E402
from oracle.weights import make_state_dict                 # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, FILL = 4096, 0xA5


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _qt(quality):
    qt = JW.quant_tables(quality)
    return qt, torch.from_numpy(qt.view(np.int16)).cuda()


def _encode(frame, quality=75, ids=None, ctab=None, cap=None, pad=0):
    """-> (stream buffer with guards, stream, status) after the stage ran on its own.  pad: extra bytes per frame row."""
    H, W = frame.shape[:2]
    cap = O.OpList.jpeg_enc_capacity(H, W, worst=True) if cap is None else cap
    buf = torch.full((cap + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    stream = buf[GUARD:GUARD + cap]
    status = torch.full((4,), -1, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.jpeg_enc_scratch_words(H, W), dtype=torch.int32, device='cuda')
    if pad:
        rows = torch.full((H, 3 * W + pad), 0x5A, dtype=torch.uint8, device='cuda')
        dev = rows.as_strided((H, W, 3), (3 * W + pad, 3, 1))
        dev.copy_(torch.from_numpy(frame))
    else:
        dev = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    ol = O.OpList()
    ol.jpeg_encode(dev, None if ids is None else torch.from_numpy(ids).cuda(), None if ctab is None else torch.from_numpy(ctab).cuda(),
                   _qt(quality)[1], stream, status, scratch, H=H, W=W)
    ol.run()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), stream.cpu().numpy(), status.cpu().numpy()


def _check(frame, quality=75, want=None, **kw):
    H, W = frame.shape[:2]
    buf, stream, status = _encode(frame, quality, **kw)
    n = int(status[0])
    want = pil_bytes(frame, quality) if want is None else want
    assert status.tolist()[1:] == [0, 0, 0] and n == len(want) - JW.HEADER_BYTES - 2
    assert JW.wrap(stream[:n].tobytes(), H, W, JW.quant_tables(quality)) == want
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all()      # nothing in front of the stream, nothing behind its bytes
    return stream[:n].tobytes()


# ---- bytes against PIL ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['noise', 'smooth', 'flat'])
@pytest.mark.parametrize('H,W', SIZES + [(200, 264)], ids=lambda v: str(v))
def test_stream_is_pils(H, W, kind):
    _check(content(kind, H, W))


@pytest.mark.parametrize('H,W', [(480, 854), (1080, 1920)], ids=lambda v: str(v))
def test_video_sizes(H, W):
    y, x = np.mgrid[0:H, 0:W]
    rs = np.random.RandomState(H)
    a = np.stack([(y // 3 + x // 2) % 256, (x * y // 512) % 256, (y + 2 * x) // 7 % 256], -1).astype(np.uint8)
    a[H // 4:H // 2, W // 3:W // 2] = rs.randint(0, 256, (H // 2 - H // 4, W // 2 - W // 3, 3))     # a textured region inside smooth content
    _check(a)


def test_noise_at_quality_100():
    """Many 0xFF bytes and the largest categories."""
    a = content('noise', 200, 264, seed=5)
    seg = _check(a, 100)
    assert seg.count(b'\xff\x00') > 100


def test_flat_but_for_one_block():
    a = content('flat', 200, 264)
    a[96:104, 136:144] = content('noise', 8, 8)
    _check(a)


def test_stripes_code_long_zero_runs():
    a = content('stripes', 33, 47)
    assert R.has_zrl(a, JW.quant_tables(30))
    _check(a, 30)
    _check(content('noise', 21, 37), 30)


def test_golden_bike_frames():
    d = os.path.join(HERE, 'golden', 'bike')
    names = sorted(f for f in os.listdir(d) if f.endswith('.jpg'))
    assert names
    for f in names:
        _check(np.array(Image.open(os.path.join(d, f)).convert('RGB')))


# ---- overlays -------------------------------------------------------------------------------------------------------------------------
def _host_blend(image_np, out_mask, all_obj_ids, colors):
    rgb_mask = np.zeros((*out_mask.shape, 3), dtype=np.uint8)                # results_utils.py _writer
    for oid in all_obj_ids:
        rgb_mask[out_mask == oid] = colors[oid % len(colors)]
    alpha = ((out_mask == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
    return (image_np * alpha + rgb_mask * (1 - alpha)).astype(np.uint8)


@pytest.mark.parametrize('H,W', [(21, 37), (120, 200)], ids=lambda v: str(v))
def test_overlay_is_pils_encode_of_the_host_blend(H, W):
    rs = np.random.RandomState(H)
    frame = content('smooth', H, W)
    ids = np.repeat(np.repeat(rs.choice(np.array([0, 0, 1, 3, 9, 255], dtype=np.uint8), size=(-(-H // 5), -(-W // 7))), 5, 0), 7, 1)[:H, :W].copy()
    objs = [1, 3, 255]                                                        # 9 is in the plane and not an object
    want = pil_bytes(_host_blend(frame, ids, objs, RU.davis_palette_np))
    _check(frame, ids=ids, ctab=JW.color_table(RU.davis_palette_np, objs), want=want)


def test_padded_row_stride_and_null_id_plane():
    frame = content('noise', 33, 47, seed=2)
    a = _check(frame, pad=13)
    assert a == _check(frame)                                                 # (ids None: the frame as it is)


def test_two_runs_give_the_same_bytes():
    frame = content('noise', 200, 264, seed=8)
    assert _check(frame) == _check(frame)


def test_capacity_overflow_and_exact_fit():
    frame = content('noise', 120, 200, seed=4)
    need = len(pil_bytes(frame)) - JW.HEADER_BYTES - 2
    for cap in (need - 1, 64, 0):
        buf, stream, status = _encode(frame, cap=cap)
        assert status.tolist() == [need, 0, 1, 0]
        assert (buf == FILL).all()                                            # guards and stream untouched
    buf, stream, status = _encode(frame, cap=need)
    assert status.tolist() == [need, 0, 0, 0]
    assert JW.wrap(stream.tobytes(), 120, 200, JW.quant_tables(75)) == pil_bytes(frame)
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + need:] == FILL).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw(flags=128, **over):
    """One descriptor with valid slots for a 16 x 24 frame, then `over` (i<k>= / p<k>=) applied; runs it."""
    H, W = 16, 24
    t = dict(frame=torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda'), ids=torch.zeros((H, W), dtype=torch.uint8, device='cuda'),
             stream=torch.zeros(4096, dtype=torch.uint8, device='cuda'), status=torch.zeros(8, dtype=torch.int32, device='cuda'),
             scratch=torch.zeros(O.OpList.jpeg_enc_scratch_words(H, W) + 8, dtype=torch.int32, device='cuda'),
             colors=torch.zeros((257, 4), dtype=torch.uint8, device='cuda'), qt=_qt(75)[1].flatten().repeat(2))
    ints = [0, H, W, 0, 3 * W, 0, 0, 4096, O.OpList.jpeg_enc_scratch_words(H, W)]
    ptrs = [t['frame'].data_ptr(), 0, t['ids'].data_ptr(), t['stream'].data_ptr(), t['status'].data_ptr(), t['scratch'].data_ptr(),
            t['colors'].data_ptr(), t['qt'].data_ptr()]
    for k, v in over.items():
        if k[0] == 'i':
            ints[int(k[1:])] = v
        else:
            ptrs[int(k[1:])] = v(ptrs[int(k[1:])]) if callable(v) else v
    ol = O.OpList()
    ol.add(O.PROB_TO_ID, flags, ints, [], ptrs)
    ol.keep.extend(t.values())
    ol.run()
    torch.cuda.synchronize()
    return t


REFUSALS = [(dict(i1=0), 'empty shape'), (dict(i2=0), 'empty shape'), (dict(i1=65536), 'at most 65535'), (dict(i2=70000), 'at most 65535'),
            (dict(i1=65535, i2=40000, i4=120000), 'exceeds 2\\^31 pixels'), (dict(i7=-1), 'negative capacity'),
            (dict(p0=0), 'needs the frame'), (dict(p3=0), 'needs the frame'), (dict(p4=0), 'needs the frame'), (dict(p5=0), 'needs the frame'),
            (dict(p7=0), 'needs the frame'), (dict(p6=0), 'needs the frame'),
            (dict(p4=lambda a: a + 2), 'aligned'), (dict(p5=lambda a: a + 8), 'aligned'), (dict(p6=lambda a: a + 2), 'aligned'),
            (dict(p7=lambda a: a + 1), 'aligned'), (dict(i4=3 * 24 - 1), 'row stride'),
            (dict(i8=O.OpList.jpeg_enc_scratch_words(16, 24) - 1), 'scratch of')]


@pytest.mark.parametrize('over,msg', REFUSALS, ids=[f'{"_".join(o)}-{m.split()[0]}' for o, m in REFUSALS])
def test_launcher_refusals(over, msg):
    with pytest.raises(RuntimeError, match=msg):
        _raw(**over)


def test_128_combines_with_no_other_flag():
    for f in (1, 2, 4, 8, 16, 32, 64):
        with pytest.raises(RuntimeError, match='unknown flags'):
            _raw(flags=128 | f)
    t = _raw()                                                                # and the same slots alone run
    assert t['status'][:4].tolist()[1:] == [0, 0, 0] and int(t['status'][0]) > 0


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.model.cutie import CUTIE
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


def _files(root, ext):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), 'rb').read()
            for dp, _, fs in os.walk(root) for f in fs if f.endswith(ext)}


def _decoded(files):
    out = {}
    for k, v in files.items():
        im = Image.open(io.BytesIO(v))
        out[k] = (im.mode, im.getpalette(), np.array(im).tolist())
    return out


@pytest.fixture(scope='module')
def videos(tmp_path_factory, gpu_net):
    """Two 4-frame 120 x 200 videos and what overlay='host', egress='host' writes for them (once)."""
    from cutie_amd.eval_vos import process_video
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from test_ingest_cpu import _make_video
    root = str(tmp_path_factory.mktemp('overlay'))
    _make_video(root, 'v0', n=4, h=120, w=200, ids=(1, 2), seed=3)
    _make_video(root, 'v1', n=4, h=120, w=200, ids=(4, 7), seed=5)
    ds = lambda **kw: list(VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False, **kw).get_datasets())
    with torch.inference_mode():
        for rd in ds():
            process_video(gpu_net, default_config(), rd, os.path.join(root, 'host', 'm'), visualize=True,
                          visualize_output_root=os.path.join(root, 'host', 'v'))
    host = (_files(os.path.join(root, 'host', 'm'), '.png'), _files(os.path.join(root, 'host', 'v'), '.jpg'))
    assert len(host[0]) == 8 and len(host[1]) == 8
    return root, ds, host


def _compare(out, host, egress, only=None):
    masks, jpgs = _files(os.path.join(out, 'm'), '.png'), _files(os.path.join(out, 'v'), '.jpg')
    want_m = {k: v for k, v in host[0].items() if only is None or k.startswith(only)}
    want_j = {k: v for k, v in host[1].items() if only is None or k.startswith(only)}
    assert jpgs == want_j and len(jpgs) > 0                                   # the .jpg files byte for byte
    if egress == 'host':
        assert masks == want_m
    else:
        assert _decoded(masks) == _decoded(want_m)


@pytest.mark.parametrize('ingest', [None, 'device', 'device-decode'])
@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_video_device_overlay_writes_the_host_files(videos, gpu_net, egress, ingest):
    from cutie_amd.eval_vos import process_video
    root, ds, host = videos
    out = os.path.join(root, f'pv_{egress}_{ingest}')
    with torch.inference_mode():
        r = process_video(gpu_net, default_config(), ds()[0], os.path.join(out, 'm'), visualize=True, visualize_output_root=os.path.join(out, 'v'),
                          overlay='device', egress=egress, ingest=ingest)
    assert r['frames'] == 4
    _compare(out, host, egress, only='v0')


def test_lockstep_group_device_overlay(videos, gpu_net):
    from cutie_amd.eval_vos import process_videos_lockstep
    root, ds, host = videos
    out = os.path.join(root, 'ls')
    with torch.inference_mode():
        process_videos_lockstep(gpu_net, default_config(), ds(ingest='device'), os.path.join(out, 'm'), visualize=True,
                                visualize_output_root=os.path.join(out, 'v'), overlay='device', egress='device')
        process_videos_lockstep(gpu_net, default_config(), ds(ingest='device'), os.path.join(out, 'ref', 'm'), visualize=True,
                                visualize_output_root=os.path.join(out, 'ref', 'v'))
    ref = (_files(os.path.join(out, 'ref', 'm'), '.png'), _files(os.path.join(out, 'ref', 'v'), '.jpg'))
    assert len(ref[1]) == 8
    _compare(out, ref, 'device')


def test_merged_scales_device_overlay(videos, gpu_net):
    from cutie_amd.eval_vos import process_video_multiscale
    root, ds, host = videos
    runs = {}
    with torch.inference_mode():
        # (one ingest mode for all three runs: the resized member's frames come from another resize on the host path, and so may its masks)
        for name, kw in (('ref', {}), ('dev', dict(overlay='device', egress='device')), ('devhost', dict(overlay='device'))):
            out = os.path.join(root, 'ms_' + name)
            rds = [ds(size=sz)[0] for sz in (-1, 96)]
            process_video_multiscale(gpu_net, default_config(), rds, os.path.join(out, 'm'), visualize=True,
                                     visualize_output_root=os.path.join(out, 'v'), ingest='device', **kw)
            runs[name] = (_files(os.path.join(out, 'm'), '.png'), _files(os.path.join(out, 'v'), '.jpg'))
    assert len(runs['ref'][1]) == 4
    _compare(os.path.join(root, 'ms_dev'), runs['ref'], 'device')
    _compare(os.path.join(root, 'ms_devhost'), runs['ref'], 'host')
