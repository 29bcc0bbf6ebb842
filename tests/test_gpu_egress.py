"""Device egress on the MI355X (PROB_TO_ID flags 4 / 8, ABI 7): the fused resample + argmax kernel against the library's own RESIZE ->
PROB_TO_ID chain (equal ids) and against a float64 bilinear + argmax, the PNG deflate kernels against the numpy model (tests/png_ref.py:
equal bytes) with guard bytes around the stream, and the drivers end to end with egress='host' and 'device' (equal images)."""
import io
import os
import shutil
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.utils import png as C
from cutie_amd.inference.utils import results_utils as RU
from oracle.weights import make_state_dict

import png_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = R.corpus(os.path.join(HERE, 'golden'))
GUARD = 4096


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


# ---- fused resample + argmax ------------------------------------------------------------------------------------------------------
def _lut(P, dtype):
    hi = 250 if dtype == torch.uint8 else 70000
    return torch.tensor([0] + [hi - 3 * k for k in range(1, P)], dtype=torch.int32, device='cuda')


def _chain(prob, lut, OH, OW, dtype):
    P, h, w = prob.shape
    full = torch.empty((P, OH, OW), dtype=torch.float32, device='cuda')
    out = torch.empty((OH, OW), dtype=dtype, device='cuda')
    ol = O.OpList()
    ol.resize(prob, full, C=P, H=h, W=w, OH=OH, OW=OW, plane=prob.stride(0), ldrow=prob.stride(1))
    ol.prob_to_id(full, lut, out, P=P, H=OH, W=OW, plane=OH * OW, ldrow=OW)
    ol.run()
    return out


def _fused(prob, lut, OH, OW, dtype):
    P, h, w = prob.shape
    buf = torch.full((OH * OW + 2 * GUARD,), 77, dtype=dtype, device='cuda')
    out = buf[GUARD:GUARD + OH * OW].view(OH, OW)
    ol = O.OpList()
    ol.prob_to_id(prob, lut, out, P=P, H=h, W=w, plane=prob.stride(0), ldrow=prob.stride(1), out_hw=(OH, OW))
    ol.run()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 77).all()) and bool((buf[-GUARD:] == 77).all())
    return out


def _probs(P, h, w, seed, smooth=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, h, w, generator=g)
    if smooth:                                               # object-like: low-frequency logits, sharpened
        x = F.interpolate(torch.randn(1, P, max(h // 16, 2), max(w // 16, 2), generator=g), size=(h, w), mode='bicubic', align_corners=False)[0] * 4 + x * 0.3
    return torch.softmax(x, 0).cuda()


GEOMS = [((480, 854), (1080, 1920)), ((480, 854), (720, 1280)), ((480, 853), (1079, 1917)), ((37, 53), (101, 149)), ((30, 40), (31, 41)),
         ((120, 214), (60, 107)), ((97, 131), (40, 77)), ((48, 64), (48, 64)), ((5, 7), (1, 1)), ((1, 1), (9, 13)), ((33, 47), (33, 90))]


@pytest.mark.parametrize('src,dst', GEOMS, ids=[f'{a[0]}x{a[1]}to{b[0]}x{b[1]}' for a, b in GEOMS])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32], ids=['u8', 'i32'])
def test_fused_equals_the_two_launch_chain(src, dst, dtype):
    prob = _probs(4, *src, seed=src[0] + dst[1])
    lut = _lut(4, dtype)
    assert torch.equal(_fused(prob, lut, *dst, dtype), _chain(prob, lut, *dst, dtype))


@pytest.mark.parametrize('P', range(1, 9))
def test_fused_plane_counts(P):
    prob = _probs(P, 60, 90, seed=P, smooth=False)
    for dtype in (torch.uint8, torch.int32):
        lut = _lut(P, dtype)
        assert torch.equal(_fused(prob, lut, 133, 201, dtype), _chain(prob, lut, 133, 201, dtype))


def test_fused_reads_the_strided_unpadded_view_in_place():
    big = torch.softmax(torch.randn(3, 96, 144, generator=torch.Generator().manual_seed(5)), 0).cuda()
    view = big[:, 3:3 + 85, 7:7 + 131]                        # what `step` returns: rows and planes of the padded tensor
    assert not view.is_contiguous()
    lut = _lut(3, torch.uint8)
    got = _fused(view, lut, 170, 262, torch.uint8)
    assert torch.equal(got, _chain(view.contiguous(), lut, 170, 262, torch.uint8))
    assert torch.equal(got, _chain(view, lut, 170, 262, torch.uint8))


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32], ids=['u8', 'i32'])
def test_fused_writes_a_misaligned_output_element_by_element(dtype):
    """OW % 4 == 0 but the output starts 1 / 2 / 3 elements behind an aligned address: no packed stores, the same ids, nothing outside."""
    prob = _probs(4, 60, 90, seed=21)
    lut = _lut(4, dtype)
    OH, OW = 96, 144
    want = _chain(prob, lut, OH, OW, dtype)
    for off in (1, 2, 3):
        buf = torch.full((OH * OW + 2 * GUARD + 4,), 77, dtype=dtype, device='cuda')
        out = buf[GUARD + off:GUARD + off + OH * OW].view(OH, OW)
        ol = O.OpList()
        ol.prob_to_id(prob, lut, out, P=4, H=60, W=90, plane=prob.stride(0), ldrow=prob.stride(1), out_hw=(OH, OW))
        ol.run()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert bool((buf[:GUARD + off] == 77).all()) and bool((buf[GUARD + off + OH * OW:] == 77).all())


def test_identity_is_plain_prob_to_id():
    prob = _probs(5, 71, 93, seed=9)
    lut = _lut(5, torch.uint8)
    out = torch.empty((71, 93), dtype=torch.uint8, device='cuda')
    ol = O.OpList()
    ol.prob_to_id(prob, lut, out, P=5, H=71, W=93, plane=prob.stride(0), ldrow=prob.stride(1))
    ol.run()
    assert torch.equal(_fused(prob, lut, 71, 93, torch.uint8), out)
    assert torch.equal(out.long(), lut.long()[prob.argmax(0)])


def test_exact_ties_go_to_the_first_maximum():
    P, h, w = 4, 24, 36
    prob = torch.full((P, h, w), 0.25)                        # every sample of every plane is exactly 0.25: all tie -> plane 0
    prob[2, :, 18:] = 0.5                                      # planes 2 and 3 tie above the rest on the right -> plane 2
    prob[3, :, 18:] = 0.5
    prob[1, 12:, :6] = 0.75                                    # and a plain winner
    prob = prob.cuda()
    lut = torch.tensor([11, 22, 33, 44], dtype=torch.int32, device='cuda')
    for dst in ((48, 72), (24, 36), (61, 95)):
        got = _fused(prob, lut, *dst, torch.uint8)
        assert torch.equal(got, _chain(prob, lut, *dst, torch.uint8))
        full = F.interpolate(prob[None], size=dst, mode='bilinear', align_corners=False)[0]
        flat = (full[0] == full[1]) & (full[1] == full[2]) & (full[2] == full[3])
        assert bool((got[flat] == 11).all()) and int(flat.sum()) > 0
    got = _fused(prob, lut, 48, 72, torch.uint8)
    assert bool((got[:, 40:] == 33).all()) and bool((got[30:, :8] == 22).all())


def _bilinear64(prob, OH, OW):
    """float64 bilinear, align_corners=False, the source index as F.interpolate defines it."""
    P, h, w = prob.shape
    p = prob.astype(np.float64)

    def axis(n_in, n_out):
        f = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(f.astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), f - i0
    y0, y1, ly = axis(h, OH)
    x0, x1, lx = axis(w, OW)
    top = p[:, y0][:, :, x0] * (1 - lx) + p[:, y0][:, :, x1] * lx
    bot = p[:, y1][:, :, x0] * (1 - lx) + p[:, y1][:, :, x1] * lx
    return top * (1 - ly)[None, :, None] + bot * ly[None, :, None]


F64_CASES = [(4, (120, 214), (270, 480), 0), (4, (120, 214), (270, 480), 1), (3, (97, 131), (211, 301), 2), (8, (60, 90), (40, 77), 3),
             (4, (480, 854), (720, 1280), 4)]


def _f64_check(ids, prob, OH, OW):
    ref = _bilinear64(prob, OH, OW)
    arg = ref.argmax(0)
    diff = ids != arg
    srt = np.sort(ref, axis=0)
    gap = srt[-1] - srt[-2] if ref.shape[0] > 1 else np.ones_like(srt[-1])
    print(f'float64 check: {int(diff.sum())} of {diff.size} pixels differ, largest top-2 gap among them {float(gap[diff].max()) if diff.any() else 0.0:.3e}')
    assert bool((gap[diff] <= 1e-6).all())
    assert diff.sum() <= 0.001 * diff.size


@pytest.mark.parametrize('P,src,dst,seed', F64_CASES)
def test_fused_against_float64(P, src, dst, seed):
    """Ids may differ from the float64 argmax only where its two largest values lie within 1e-6, and on at most 0.1 % of the pixels (a
    condition, not a measurement).  Seeds 0..4 of F64_CASES were checked on the CPU: torch's own fp32 F.interpolate + argmax stays inside
    the same condition on these inputs (test_torch_fp32_stays_inside_the_float64_condition repeats that check wherever this file runs)."""
    prob = _probs(P, *src, seed=seed)
    got = _fused(prob, torch.arange(P, dtype=torch.int32, device='cuda'), *dst, torch.int32).cpu().numpy()
    _f64_check(got, prob.cpu().numpy(), *dst)


@pytest.mark.parametrize('P,src,dst,seed', F64_CASES)
def test_torch_fp32_stays_inside_the_float64_condition(P, src, dst, seed):
    prob = _probs(P, *src, seed=seed).cpu()
    ids = F.interpolate(prob[None], size=dst, mode='bilinear', align_corners=False)[0].argmax(0).numpy()
    _f64_check(ids, prob.numpy(), *dst)


# ---- PNG deflate ----------------------------------------------------------------------------------------------------------------
def _deflate(ids, cap=None):
    """-> (stream buffer with guards, stream view, status) after the stage ran on its own."""
    H, W = ids.shape
    cap = O.OpList.png_capacity(H, W) if cap is None else cap
    buf = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    stream = buf[GUARD:GUARD + cap]
    status = torch.full((4,), -1, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device='cuda')
    ol = O.OpList()
    ol.png_deflate(torch.from_numpy(ids).cuda(), stream, status, scratch, H=H, W=W)
    ol.run()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), stream.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('name', sorted(CORPUS))
def test_deflate_equals_the_model(name):
    ids = CORPUS[name]
    H, W = ids.shape
    want, adler = R.encode(ids)
    buf, stream, status = _deflate(ids)
    n = int(status[0])
    assert int(status[2]) == 0 and n == len(want) and (int(status[1]) & 0xffffffff) == adler
    got = stream[:n].tobytes()
    assert got == want
    assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
    R.check_stream(got, ids)
    assert zlib.decompress(got) == R.filtered(ids).tobytes()
    for pal in (RU.davis_palette, None):
        im = Image.open(io.BytesIO(C.assemble(got, H, W, pal)))
        assert im.mode == ('P' if pal is not None else 'L') and np.array_equal(np.array(im), ids)
        if pal is not None:
            assert bytes(im.getpalette()) == RU.davis_palette
    if name.startswith('golden/') and H == 480:
        assert n <= H * W // 32


def test_deflate_1080p_upscaled_mask():
    ids = np.kron(CORPUS['golden/bike/00000.png'], np.ones((3, 3), np.uint8))[:1080, :1920]
    want, adler = R.encode(ids)
    _, stream, status = _deflate(ids)
    assert int(status[2]) == 0 and stream[:int(status[0])].tobytes() == want


def test_small_capacity_sets_the_overflow_bit_and_writes_nothing_behind_the_buffer():
    ids = CORPUS['noise256']
    need = len(R.encode(ids)[0])
    for cap in (need - 1) // 4 * 4, 64, 0:
        buf, stream, status = _deflate(ids, cap=cap)
        assert int(status[2]) & 1 and int(status[0]) == need
        assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + cap:] == 0xA5).all()
    cap = (need + 3) // 4 * 4                                   # and the smallest capacity that fits
    buf, stream, status = _deflate(ids, cap=cap)
    assert int(status[2]) == 0 and stream[:need].tobytes() == R.encode(ids)[0]
    assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + cap:] == 0xA5).all()


def test_argmax_and_deflate_in_one_op():
    prob = _probs(4, 120, 214, seed=11)
    lut = _lut(4, torch.uint8)
    for dst in (None, (270, 481)):
        H, W = dst or (120, 214)
        ids = torch.empty((H, W), dtype=torch.uint8, device='cuda')
        stream = torch.empty(O.OpList.png_capacity(H, W), dtype=torch.uint8, device='cuda')
        status = torch.empty(4, dtype=torch.int32, device='cuda')
        scratch = torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device='cuda')
        ol = O.OpList()
        ol.prob_to_id(prob, lut, ids, P=4, H=120, W=214, plane=prob.stride(0), ldrow=prob.stride(1), out_hw=dst, png=(stream, status, scratch))
        ol.run()
        torch.cuda.synchronize()
        assert torch.equal(ids, _chain(prob, lut, H, W, torch.uint8))
        want, _ = R.encode(ids.cpu().numpy())
        assert int(status[2]) == 0 and stream[:int(status[0])].cpu().numpy().tobytes() == want


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.model.cutie import CUTIE
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


def _images(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith('.png'):
                im = Image.open(os.path.join(dp, f))
                out[os.path.relpath(os.path.join(dp, f), root)] = (im.mode, im.getpalette(), np.array(im))
    return out


def _same(a, b):
    assert sorted(a) == sorted(b) and len(a) > 0
    for k in a:
        assert a[k][0] == b[k][0] and a[k][1] == b[k][1] and np.array_equal(a[k][2], b[k][2]), k


def _no_pil_bytes(root):
    """The device files are this project's container (one IDAT with the fixed-code stream), not PIL's."""
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith('.png'):
                data = open(os.path.join(dp, f), 'rb').read()
                o = data.index(b'IDAT') + 4
                assert data[o:o + 2] == b'\x78\x01' and (data[o + 2] & 7) == 3


@pytest.mark.parametrize('clip', ['bike', 'judo'])
def test_examples_host_and_device_egress_write_equal_images(gpu_net, tmp_path, clip):
    from cutie_amd.eval_vos import process_video
    from cutie_amd.inference.data.video_reader import VideoReader
    src = os.path.join(HERE, 'golden', clip)
    img_dir, msk_dir = os.path.join(tmp_path, 'JPEGImages', clip), os.path.join(tmp_path, 'Annotations', clip)
    os.makedirs(img_dir); os.makedirs(msk_dir)
    for f in sorted(os.listdir(src)):
        shutil.copy(os.path.join(src, f), img_dir if f.endswith('.jpg') else msk_dir)
    with torch.inference_mode():
        for name, kw in (('host', dict(egress='host')), ('device', dict(egress='device')),
                         ('both', dict(egress='device', ingest='device-decode'))):
            rd = VideoReader(clip, img_dir, msk_dir, ingest=kw.get('ingest', 'host'))
            r = process_video(gpu_net, default_config(), rd, os.path.join(tmp_path, name), dataset='d17-val', **kw)
            assert r['frames'] == len(rd)
    host = _images(os.path.join(tmp_path, 'host'))
    assert len(host) == len(os.listdir(img_dir))
    _same(_images(os.path.join(tmp_path, 'device')), host)
    _same(_images(os.path.join(tmp_path, 'both')), host)
    _no_pil_bytes(os.path.join(tmp_path, 'device'))


def test_720p_size_480_lockstep_and_clips_in_flight(tmp_path):
    """--size 480 on 1280 x 720 frames (the fused resample + argmax runs), alone, in lock step and with three clips in flight."""
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    from cutie_amd.eval_vos import process_video, process_videos_lockstep
    from cutie_amd.parallel import run_concurrent
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from test_gpu_ingest import _make_720p_video
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(S.decisive_state_dict())
    root = str(tmp_path)
    for k, ids in enumerate(((1, 2), (3, 7), (2, 5))):
        _make_720p_video(root, 'v' + 'ABC'[k], 6, ids, 41 + k)
    rds = list(VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False, size=480,
                              ingest='device').get_datasets())
    assert len(rds) == 3 and all(rd[1]['info']['resize_needed'] for rd in rds)
    cfg = default_config(mem_every=3)
    with torch.inference_mode():
        for eg in ('host', 'device'):
            for rd in rds:
                process_video(net, cfg, rd, os.path.join(root, 'alone_' + eg), egress=eg)
            process_videos_lockstep(net, cfg, rds, os.path.join(root, 'ls_' + eg), egress=eg)
        run_concurrent(net, range(3), lambda view, c: process_video(view, cfg, rds[c], os.path.join(root, 'cc_device'), egress='device'),
                       streams=3)
    torch.cuda.synchronize()
    host = _images(os.path.join(root, 'alone_host'))
    assert len(host) == 18 and all(v[2].shape == (720, 1280) for v in host.values())
    _same(_images(os.path.join(root, 'alone_device')), host)
    _same(_images(os.path.join(root, 'ls_device')), _images(os.path.join(root, 'ls_host')))
    _same(_images(os.path.join(root, 'cc_device')), host)
    _no_pil_bytes(os.path.join(root, 'cc_device'))


def _files(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(root) for f in fs}


def test_fall_backs_write_the_host_files(gpu_net, tmp_path):
    """visualize and use_long_id savers run the host path whatever `egress` says: the same bytes."""
    from cutie_amd.eval_vos import process_video
    from cutie_amd.inference.data.video_reader import VideoReader
    from test_ingest_cpu import _make_video
    root = str(tmp_path)
    _make_video(root, 'v0', n=4, h=120, w=200, ids=(1, 2), seed=3)
    img, msk = os.path.join(root, 'JPEGImages', 'v0'), os.path.join(root, 'Annotations', 'v0')
    long_dir = os.path.join(root, 'Annotations_long', 'v0')
    os.makedirs(long_dir)
    for f in os.listdir(msk):                                  # the same masks as RGB (long-id) files
        a = np.array(Image.open(os.path.join(msk, f)))
        Image.fromarray(np.stack([a, np.zeros_like(a), np.zeros_like(a)], -1).astype(np.uint8)).save(os.path.join(long_dir, f))
    with torch.inference_mode():
        for eg in ('host', 'device'):
            rd = VideoReader('v0', img, msk)
            process_video(gpu_net, default_config(), rd, os.path.join(root, 'vis_' + eg, 'm'), visualize=True,
                          visualize_output_root=os.path.join(root, 'vis_' + eg, 'v'), egress=eg)
            rd = VideoReader('v0', img, long_dir)
            assert rd.use_long_id
            np.random.seed(7)                                  # (long ids get colours from numpy's global stream: the same draw for both runs)
            process_video(gpu_net, default_config(), rd, os.path.join(root, 'long_' + eg), egress=eg)
    assert _files(os.path.join(root, 'vis_device')) == _files(os.path.join(root, 'vis_host'))
    assert len(_files(os.path.join(root, 'vis_host'))) == 8
    assert _files(os.path.join(root, 'long_device')) == _files(os.path.join(root, 'long_host'))
    assert all(v[0] == 'RGB' for v in _images(os.path.join(root, 'long_device')).values())


def test_save_scores_next_to_the_device_mask(gpu_net, tmp_path):
    from cutie_amd.eval_vos import process_video
    from cutie_amd.inference.data.video_reader import VideoReader
    from test_ingest_cpu import _make_video
    root = str(tmp_path)
    _make_video(root, 'v0', n=3, h=120, w=200, ids=(1, 2), seed=4)
    img, msk = os.path.join(root, 'JPEGImages', 'v0'), os.path.join(root, 'Annotations', 'v0')
    with torch.inference_mode():
        for eg in ('host', 'device'):
            process_video(gpu_net, default_config(save_scores=True), VideoReader('v0', img, msk), os.path.join(root, eg, 'm'), save_scores=True,
                          score_output_root=os.path.join(root, eg, 's'), egress=eg)
    _same(_images(os.path.join(root, 'device')), _images(os.path.join(root, 'host')))
    for f in ('00000.npz', '00002.npz'):
        a, b = np.load(os.path.join(root, 'host', 's', 'v0', f)), np.load(os.path.join(root, 'device', 's', 'v0', f))
        assert np.array_equal(a['prob'], b['prob'])
