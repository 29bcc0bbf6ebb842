"""The visualisation modes, the alpha matte and the soft masks on the MI355X (PROB_TO_ID flags == 256 / 512, ABI 11, forms added, csrc/matte.hip):
the kernels' bytes equal the numpy model's (tests/matte_ref.py, which equals the reference's torch functions: tests/test_matte_cpu.py)
at every size, stride, plane count, target list and mode; guard rows stay intact; refusals; process_video writes the model's files."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import matte_ref as M                                      # noqa: E402
import png_ref                                             # noqa: E402

from cutie_amd import _lib, ops as O                       # noqa: E402
from cutie_amd.config import default_config               # noqa: E402
from cutie_amd.inference.utils import jpeg_writer as JW    # noqa: E402
from cutie_amd.inference.utils import png as png_container  # noqa: E402
from cutie_amd.inference.utils import results_utils as RU  # noqa: E402
from oracle.weights import make_state_dict                 # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 4096, 0xA5
SIZES = [(1, 1), (3, 5), (33, 47), (8, 63), (8, 64), (8, 65), (97, 131), (480, 854)]


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


class Guarded:
    """A uint8 device buffer between two guard regions (the payload starts 16-byte aligned)."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == FILL).all() and (b[GUARD + self.n:] == FILL).all()
        return b[GUARD:GUARD + self.n].reshape(tuple(self.t.shape))


def _inputs(OH, OW, P, hw=None, seed=0):
    rs = np.random.RandomState(seed + 1000 * OH + OW + 7 * P)
    h, w = hw or (OH, OW)
    planes = rs.rand(P, h, w).astype(np.float32)
    planes /= planes.sum(0, keepdims=True)                                    # object-like: a distribution over the planes ...
    planes[:, rs.rand(h, w) < 0.1] = np.eye(P, dtype=np.float32)[rs.randint(0, P)][:, None]      # ... with saturated pixels (exact 0 and 1)
    frame = rs.randint(0, 256, (OH, OW, 3)).astype(np.uint8)
    layer = rs.randint(0, 256, (OH, OW, 4)).astype(np.uint8)
    layer[rs.rand(OH, OW) < 0.2, 3] = 255
    layer[rs.rand(OH, OW) < 0.2, 3] = 0
    ids = rs.choice(np.array([0, 0, 1, 2, 3, 7, 200, 255], dtype=np.uint8), size=(OH, OW))     # 7 and 200 are in no table: colour 0
    table = rs.randint(0, 256, (256, 4)).astype(np.uint8)
    table[[7, 200]] = 0
    return planes, frame, layer, ids, table


def _dev_planes(planes, view):
    """view: the planes as the un-padded view of a larger store (plane and row strides, a base that is not 16-byte aligned)."""
    P, h, w = planes.shape
    if not view:
        return torch.from_numpy(planes).cuda()
    store = torch.full((P, h + 3, w + 5), float('nan'), device='cuda')
    v = store[:, 1:h + 1, 3:w + 3]
    v.copy_(torch.from_numpy(planes))
    return v


def _dev_frame(frame, pad, off):
    """pad: extra bytes per row; off: bytes in front of the first pixel (an odd one: no dword of the frame is aligned)."""
    H, W = frame.shape[:2]
    if not pad and not off:
        return torch.from_numpy(frame).cuda()
    rows = torch.full((off + H * (3 * W + pad),), 0x5A, dtype=torch.uint8, device='cuda')
    v = rows[off:].as_strided((H, W, 3), (3 * W + pad, 3, 1))
    v.copy_(torch.from_numpy(frame))
    return v


def composite(mode, planes, frame, layer, ids, table, out_hw, targets=(), want_alpha=False, view=False, pad=0, off=0):
    OH, OW = out_hw
    soft = mode in ('popup', 'layer', 'alpha')
    out = Guarded((OH, OW, 3)) if mode != 'alpha' else None
    matte = Guarded((OH, OW)) if (want_alpha or mode == 'alpha') else None
    ol = O.OpList()
    ol.matte_composite(mode, out.t if out else None, out_hw=out_hw, frame=_dev_frame(frame, pad, off) if out else None,
                       planes=_dev_planes(planes, view) if soft else None, targets=targets,
                       ids=None if soft else torch.from_numpy(ids).cuda(), colors=None if soft else torch.from_numpy(table).cuda(),
                       layer=torch.from_numpy(layer).cuda() if mode == 'layer' else None, matte=matte.t if matte else None)
    ol.run()
    torch.cuda.synchronize()
    return (out.get() if out else None), (matte.get() if matte else None)


def soft_planes(planes, out_hw, view=False):
    P = planes.shape[0]
    out = Guarded((max(P - 1, 0), *out_hw)) if P > 1 else Guarded((1, *out_hw))
    ol = O.OpList()
    ol.matte_soft(_dev_planes(planes, view), out.t if P > 1 else out.t[:0], out_hw=out_hw)
    ol.run()
    torch.cuda.synchronize()
    got = out.get()
    if P == 1:
        assert (got == FILL).all()                                            # no object plane: nothing written
        return got[:0]
    return got


def check_all(planes, frame, layer, ids, table, out_hw, target_lists, **kw):
    """Every mode, the matte with and without a frame and the soft planes against the model, byte for byte."""
    for mode in ('davis', 'light', 'fade'):
        got, _ = composite(mode, planes, frame, layer, ids, table, out_hw, pad=kw.get('pad', 0), off=kw.get('off', 0))
        want, _ = M.composite(mode, frame, ids=ids, table=table)
        assert np.array_equal(got, want), (mode, int((got != want).sum()))
    for targets in target_lists:
        _, alone = composite('alpha', planes, frame, layer, ids, table, out_hw, targets, view=kw.get('view', False))
        for mode in ('popup', 'layer'):
            got, a = composite(mode, planes, frame, layer, ids, table, out_hw, targets, want_alpha=True, **kw)
            want, wa = M.composite(mode, frame, planes, targets, layer_rgba=layer, out_hw=out_hw, want_alpha=True)
            assert np.array_equal(got, want), (mode, targets, int((got != want).sum()))
            assert np.array_equal(a, wa) and np.array_equal(alone, wa), (mode, targets)
            got2, a2 = composite(mode, planes, frame, layer, ids, table, out_hw, targets, **kw)      # without the matte: the same frame
            assert np.array_equal(got2, want) and a2 is None
    got = soft_planes(planes, out_hw, view=kw.get('view', False))
    assert np.array_equal(got, M.soft(planes, *out_hw))


def _lists(P):
    return [[], [1], [P - 1, 1], list(range(1, P))] if P > 1 else [[], [0]]


# ---- bytes against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('OH,OW', SIZES, ids=lambda v: str(v))
def test_planes_at_the_output_size(OH, OW):
    planes, frame, layer, ids, table = _inputs(OH, OW, 4)
    check_all(planes, frame, layer, ids, table, (OH, OW), _lists(4) if OH < 400 else [[3, 1]])


@pytest.mark.parametrize('hw,out_hw', [((30, 40), (97, 131)), ((17, 23), (33, 47)), ((64, 80), (33, 47))], ids=lambda v: 'x'.join(map(str, v)))
@pytest.mark.parametrize('view', [False, True], ids=['contiguous', 'view'])
def test_planes_resampled(hw, out_hw, view):
    planes, frame, layer, ids, table = _inputs(*out_hw, 4, hw=hw, seed=3)
    check_all(planes, frame, layer, ids, table, out_hw, _lists(4), view=view)


@pytest.mark.parametrize('OH,OW', [(33, 47), (8, 64)], ids=lambda v: str(v))
def test_strided_planes_and_frames(OH, OW):
    planes, frame, layer, ids, table = _inputs(OH, OW, 4, seed=5)
    check_all(planes, frame, layer, ids, table, (OH, OW), [[3, 1]], view=True)            # plane and row strides of an un-padded view
    check_all(planes, frame, layer, ids, table, (OH, OW), [[3, 1]], pad=4)                # a padded frame row, still dword-aligned
    check_all(planes, frame, layer, ids, table, (OH, OW), [[3, 1]], pad=7, off=1)         # an odd row stride and an odd base


@pytest.mark.parametrize('P', [1, 2, 4, 8])
def test_plane_counts_and_target_lists(P):
    planes, frame, layer, ids, table = _inputs(33, 47, P, seed=9)
    check_all(planes, frame, layer, ids, table, (33, 47), _lists(P))
    if P > 2:                                                                 # the order of the list is part of the result
        big = np.random.RandomState(P).rand(P, 64, 64).astype(np.float32) * np.float32(0.4)
        fr, la = np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 4), np.uint8)
        fwd, rev = list(range(1, P)), [P - 1] + list(range(1, P - 1))
        assert (M.target_sum(big, fwd) != M.target_sum(big, rev)).any()
        for t in (fwd, rev):
            _, a = composite('alpha', big, fr, la, None, None, (64, 64), t)
            assert np.array_equal(a, M.composite('alpha', planes=big, targets=t)[1])


def test_sums_above_one_are_clamped_and_golden_bytes():
    """The reference's own bytes (tests/golden/matte/, the case built to pass 1) from the kernel."""
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'matte', 'm_clamp_9x14_p4.npz'))
    planes, frame, layer = z['planes'].astype(np.float32), z['frame'], z['layer']
    n = 0
    for key in z.files:
        mode, *t = key.split('_')
        if key in ('frame', 'planes', 'layer', 'table') or mode not in ('layer', 'rgba'):
            continue
        t = [int(v) for v in t]
        if mode == 'layer':
            got, _ = composite('layer', planes, frame, layer, None, None, (9, 14), t)
            assert np.array_equal(got, z[key])
        else:
            _, a = composite('alpha', planes, frame, layer, None, None, (9, 14), t)
            assert np.array_equal(a, z[key][..., 3]) and (a == 255).any()
        n += 1
    assert n == 6


def test_two_runs_give_the_same_bytes():
    planes, frame, layer, ids, table = _inputs(97, 131, 4, hw=(30, 40), seed=11)
    a = [composite('layer', planes, frame, layer, ids, table, (97, 131), [3, 1], want_alpha=True) for _ in range(2)]
    assert np.array_equal(a[0][0], a[1][0]) and np.array_equal(a[0][1], a[1][1])
    s = [soft_planes(planes, (97, 131)) for _ in range(2)]
    assert np.array_equal(s[0], s[1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw(flags=256, mode=4, **over):
    """One descriptor with valid slots (16 x 24 output, 4 planes of 8 x 12, two targets), then `over` (i<k>= / p<k>=) applied; runs it."""
    OH, OW, P, H, W = 16, 24, 4, 8, 12
    t = dict(planes=torch.rand((P, H, W), device='cuda'), frame=torch.zeros((OH, OW, 3), dtype=torch.uint8, device='cuda'),
             out=torch.zeros((OH * OW * 3 + 64,), dtype=torch.uint8, device='cuda'), matte=torch.zeros((OH * OW + 64,), dtype=torch.uint8, device='cuda'),
             ids=torch.zeros((OH * OW + 8,), dtype=torch.uint8, device='cuda'), colors=torch.zeros((257, 4), dtype=torch.uint8, device='cuda'),
             layer=torch.zeros((OH * OW * 4 + 64,), dtype=torch.uint8, device='cuda'), soft=torch.zeros(((P - 1) * OH * OW + 64,), dtype=torch.uint8, device='cuda'))
    tg = np.array([3, 1] + [0] * 300, dtype=np.int32)
    ints = [P, H, W, H * W, W, OH, OW, 3 * OW, mode, 2]
    hard = mode <= 2
    if flags == 512:
        ints[7:] = [0, 0, 0]
        ptrs = [t['planes'].data_ptr(), 0, t['soft'].data_ptr()]
    else:
        ptrs = [0 if hard else t['planes'].data_ptr(), 0 if hard else tg.ctypes.data, 0 if mode == 5 else t['frame'].data_ptr(), 0 if mode == 5 else t['out'].data_ptr(),
                0 if hard else t['matte'].data_ptr(), t['ids'].data_ptr() if hard else 0, t['colors'].data_ptr() if hard else 0,
                t['layer'].data_ptr() if mode == 4 else 0]
    for k, v in over.items():
        if k == 'tg':
            tg[:len(v)] = v
        elif k[0] == 'i':
            ints[int(k[1:])] = v
        else:
            ptrs[int(k[1:])] = v(ptrs[int(k[1:])]) if callable(v) else v
    ol = O.OpList()
    ol.add(O.PROB_TO_ID, flags, ints, [], ptrs)
    ol.keep.extend(list(t.values()) + [tg])
    ol.run()
    torch.cuda.synchronize()
    return t


COMPOSITE_REFUSALS = [
    (dict(i5=0), 'empty output'), (dict(i6=0), 'empty output'), (dict(i1=0), 'empty planes'), (dict(i2=0), 'empty planes'),
    (dict(i5=40000, i6=40000), 'exceeds 2\\^31 bytes'), (dict(i1=50000, i2=50000, i4=50000), 'exceed 2\\^31 pixels'),
    (dict(i0=200, i5=4000, i6=4000, i7=12000), 'exceed 2\\^31 samples'),
    (dict(i0=0), '1 <= P <= 256'), (dict(i0=257), '1 <= P <= 256'),
    (dict(tg=[4]), 'target 0 is plane 4'), (dict(tg=[3, -1]), 'target 1 is plane -1'), (dict(i9=256), '256 targets'), (dict(i9=-1), '-1 targets'),
    (dict(i8=6), 'unknown mode 6'), (dict(i8=-1), 'unknown mode -1'),
    (dict(p0=0), 'needs the planes'), (dict(p0=lambda a: a + 2), 'planes \\(p0\\) 4-byte aligned'),
    (dict(p1=0), 'needs the target list'), (dict(p1=lambda a: a + 2), 'target list \\(p1\\) 4-byte aligned'),
    (dict(p2=0), 'needs the frame'), (dict(p3=0), 'needs the frame'), (dict(p3=lambda a: a + 8), 'output frame \\(p3\\) 16-byte aligned'),
    (dict(p4=lambda a: a + 4), 'matte plane \\(p4\\) 16-byte aligned'), (dict(p7=0), 'mode layer needs the layer'),
    (dict(p7=lambda a: a + 4), 'layer \\(p7\\) 16-byte aligned'), (dict(i7=3 * 24 - 1), 'frame row stride'), (dict(i4=11), 'a row stride of 11'),
    (dict(mode=5, p4=0), 'mode alpha needs the matte'),
    (dict(mode=0, p5=0), 'need the id plane'), (dict(mode=2, p6=0), 'need the id plane'), (dict(mode=1, p5=lambda a: a + 1), '\\(p5\\) and colour table \\(p6\\) 4-byte'),
    (dict(mode=0, p6=lambda a: a + 2), '\\(p5\\) and colour table \\(p6\\) 4-byte'), (dict(mode=0, p4=4096), 'needs a soft mode')]


@pytest.mark.parametrize('over,msg', COMPOSITE_REFUSALS, ids=[f'{"_".join(o)}-{m.split()[0]}' for o, m in COMPOSITE_REFUSALS])
def test_composite_refusals(over, msg):
    with pytest.raises(RuntimeError, match='matte composite: .*' + msg):
        _raw(**over)


SOFT_REFUSALS = [(dict(i5=0), 'empty output'), (dict(i2=0), 'empty planes'), (dict(i0=257), '1 <= P <= 256'), (dict(i0=0), '1 <= P <= 256'),
                 (dict(p0=0), 'needs the planes'), (dict(p2=0), 'needs the output planes'), (dict(p2=lambda a: a + 4), 'output planes \\(p2\\) 16-byte aligned'),
                 (dict(i0=200, i5=4000, i6=4000), 'exceed 2\\^31 samples'), (dict(i4=11), 'a row stride of 11')]


@pytest.mark.parametrize('over,msg', SOFT_REFUSALS, ids=[f'{"_".join(o)}-{m.split()[0]}' for o, m in SOFT_REFUSALS])
def test_soft_refusals(over, msg):
    with pytest.raises(RuntimeError, match='matte soft: .*' + msg):
        _raw(flags=512, **over)


def test_the_new_flags_combine_with_no_other_flag():
    for base in (256, 512):
        for f in (1, 2, 4, 8, 16, 32, 64, 128, 768 - base):
            with pytest.raises(RuntimeError, match='unknown flags'):
                _raw(flags=base | f)
    _raw()                                                                    # and the same slots alone run
    _raw(flags=512)
    for mode in (0, 1, 2, 3, 5):
        _raw(mode=mode)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.model.cutie import CUTIE
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    from cutie_amd.utils.synth import SyntheticClip
    root = str(tmp_path_factory.mktemp('matte'))
    c = SyntheticClip(120, 200, 2, 3, seed=5)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(3):
        arr = (c.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(c.first_mask().numpy().astype(np.uint8))
    png.putpalette(RU.davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    Image.fromarray(np.random.RandomState(8).randint(0, 256, (40, 50, 4)).astype(np.uint8), 'RGBA').save(os.path.join(root, 'layer.png'))
    return root


def _files(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(root) for f in fs}


def _jpg(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', quality=75)
    return b.getvalue()


def _png(plane):
    return png_container.assemble(png_ref.encode(plane)[0], plane.shape[0], plane.shape[1], None)


@pytest.mark.parametrize('ingest', ['host', 'device'])
def test_process_video_writes_the_models_files(gpu_net, clip, ingest, monkeypatch):
    """The files of `--vis popup layer fade --soft-masks --alpha` are the model's frames and planes -- made from the probabilities and
    the uint8 frame the saver was handed -- through PIL's JPEG encoder and the PNG model; the mask PNGs are those of a run without
    the new options."""
    from cutie_amd.process_video import process_video, video_config
    seen = []
    real = RU.ResultSaver.process

    def spy(self, prob, frame_name, *a, **kw):
        if kw.get('image_u8') is not None:
            seen.append((frame_name, prob.detach().clone().cpu().numpy(), kw['image_u8'].clone().cpu().numpy()))
        return real(self, prob, frame_name, *a, **kw)
    monkeypatch.setattr(RU.ResultSaver, 'process', spy)
    cfg = video_config(mem_every=2)
    args = (os.path.join(clip, 'frames'), os.path.join(clip, 'masks'))
    plain = os.path.join(clip, f'plain_{ingest}')
    out = os.path.join(clip, f'all_{ingest}')
    vis = ('popup', 'layer', 'fade')
    r0 = process_video(gpu_net, cfg, *args, plain, ingest=ingest)
    assert not seen and 'folders' not in r0
    r = process_video(gpu_net, cfg, *args, out, ingest=ingest, vis_modes=vis, soft_masks=True, alpha_matte=True, layer=os.path.join(clip, 'layer.png'))
    assert r['frames'] == 3 and len(seen) == 3
    files, base = _files(out), _files(plain)
    assert sorted(base) == [f'{t:07d}.png' for t in range(3)]
    assert {k: v for k, v in files.items() if os.sep not in k} == base          # the existing mask PNGs, byte for byte
    H, W = 120, 200
    layer = np.array(Image.open(os.path.join(clip, 'layer.png')).convert('RGBA').resize((W, H)))
    pal = (RU.davis_palette_np.astype(np.float32) * 1.5).clip(0, 255).astype(np.uint8)
    table = JW.color_table(pal, [1, 2])
    want = {}
    for name, prob, u8 in seen:
        stem = name[:-4]
        assert prob.shape == (3, H, W) and u8.shape == (H, W, 3)
        # the frame the stage reads is the decoded file: uploaded as it is (device), or recovered from the float frame (host)
        assert np.array_equal(u8, np.array(Image.open(os.path.join(clip, 'frames', stem + '.jpg')).convert('RGB'))), ingest
        ids = prob.argmax(0).astype(np.uint8)                                 # (object ids 1, 2 = their plane indices here)
        popup, a = M.composite('popup', u8, prob, [1, 2], want_alpha=True)
        want[f'visualization/popup/{stem}.jpg'] = _jpg(popup)
        want[f'visualization/layer/{stem}.jpg'] = _jpg(M.composite('layer', u8, prob, [1, 2], layer_rgba=layer)[0])
        want[f'visualization/fade/{stem}.jpg'] = _jpg(M.composite('fade', u8, ids=ids, table=table)[0])
        want[f'alpha/{stem}.png'] = _png(a)
        for q, plane in enumerate(M.soft(prob, H, W)):
            want[f'soft_masks/{q + 1}/{stem}.png'] = _png(plane)
    got = {k: v for k, v in files.items() if os.sep in k}
    assert sorted(got) == sorted(want)
    assert [k for k in want if got[k] != want[k]] == []
    assert r['folders'] == [os.path.join(out, 'visualization', m) for m in vis] + [os.path.join(out, 'soft_masks'), os.path.join(out, 'alpha')]


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_several_modes_on_a_size_whose_frames_are_no_multiple_of_16_bytes(gpu_net, tmp_path, egress, monkeypatch):
    """33 x 47 x 3 = 4653 bytes per frame: every mode composes into a 16-byte aligned frame of its own (the launcher refuses any other),
    and the files are the model's."""
    from cutie_amd.process_video import process_video, video_config
    from cutie_amd.utils.synth import SyntheticClip
    root, (H, W) = str(tmp_path), (33, 47)
    c = SyntheticClip(H, W, 2, 3, seed=7)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(3):
        Image.fromarray((c.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(os.path.join(root, 'frames', f'{t:07d}.png'))
    png = Image.fromarray(c.first_mask().numpy().astype(np.uint8))
    png.putpalette(RU.davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    Image.fromarray(np.random.RandomState(8).randint(0, 256, (40, 50, 4)).astype(np.uint8), 'RGBA').save(os.path.join(root, 'layer.png'))
    seen, real = [], RU.ResultSaver.process

    def spy(self, prob, frame_name, *a, **kw):
        seen.append((frame_name, prob.detach().clone().cpu().numpy(), kw['image_u8'].clone().cpu().numpy()))
        return real(self, prob, frame_name, *a, **kw)
    monkeypatch.setattr(RU.ResultSaver, 'process', spy)
    vis = ('popup', 'fade', 'layer', 'davis', 'light')
    out = os.path.join(root, 'out')
    r = process_video(gpu_net, video_config(mem_every=2), os.path.join(root, 'frames'), os.path.join(root, 'masks'), out, ingest='device', egress=egress,
                      vis_modes=vis, soft_masks=True, alpha_matte=True, layer=os.path.join(root, 'layer.png'))
    assert r['frames'] == 3 and len(seen) == 3
    layer = np.array(Image.open(os.path.join(root, 'layer.png')).convert('RGBA').resize((W, H)))
    table = JW.color_table((RU.davis_palette_np.astype(np.float32) * 1.5).clip(0, 255).astype(np.uint8), [1, 2])
    want = {}
    for name, prob, u8 in seen:
        stem, ids = name[:-4], prob.argmax(0).astype(np.uint8)
        assert prob.shape == (3, H, W) and np.array_equal(u8, np.array(Image.open(os.path.join(root, 'frames', stem + '.png')).convert('RGB')))
        popup, a = M.composite('popup', u8, prob, [1, 2], want_alpha=True)
        want[f'visualization/popup/{stem}.jpg'] = _jpg(popup)
        want[f'visualization/layer/{stem}.jpg'] = _jpg(M.composite('layer', u8, prob, [1, 2], layer_rgba=layer)[0])
        for mode in ('fade', 'davis', 'light'):
            want[f'visualization/{mode}/{stem}.jpg'] = _jpg(M.composite(mode, u8, ids=ids, table=table)[0])
        want[f'alpha/{stem}.png'] = _png(a)
        for q, plane in enumerate(M.soft(prob, H, W)):
            want[f'soft_masks/{q + 1}/{stem}.png'] = _png(plane)
    got = {k: v for k, v in _files(out).items() if os.sep in k}
    assert sorted(got) == sorted(want) and [k for k in want if got[k] != want[k]] == []
