"""Redacted frames on the MI355X (PROB_TO_ID flags == 65536, csrc/redact.hip) against the model (tests/redact_ref.py): the bytes are equal --
at one pixel, a single row, a single column and sizes that straddle the wave and the tile widths, for every radius and cell class, fill,
the invert bit in each mode, and every kind of weight plane; guard regions around the output and the scratch survive, the frame and the
weight plane come back unchanged, at odd addresses with padded rows whose padding keeps its sentinel; the scratch's content means nothing;
a second run is bit-identical.  The launcher's refusals, the feature bit, and process_video --redact on the bike frames."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import redact_cases as RC                                  # noqa: E402
import redact_ref as R                                     # noqa: E402

from cutie_amd import _lib, ops as O                       # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, FILL, PAD = 4096, 0x5a, 0xa5


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device(frame, weight, mode, strength=0, color=(0, 0, 0), invert=False, *, shift=0, pad=0, scratch_fill=FILL):
    """The stage on one case -> the output bytes [H, W, 3].  ``shift``: the frame and the weight plane start ``shift`` bytes behind a
    16-byte aligned address; ``pad``: extra bytes per row of both, holding a sentinel that must survive.  The output (pre-filled with a
    pattern) and the scratch (pre-filled with ``scratch_fill``) sit between guards that must survive; the inputs stay as they were."""
    H, W = weight.shape
    froom = torch.full((shift + H * (3 * W + pad) + 16,), PAD, dtype=torch.uint8, device='cuda')
    f = froom[shift:shift + H * (3 * W + pad)].view(H, 3 * W + pad)[:, :3 * W].view(H, W, 3)
    f.copy_(torch.from_numpy(frame))
    wroom = torch.full((shift + H * (W + pad) + 16,), PAD, dtype=torch.uint8, device='cuda')
    w = wroom[shift:shift + H * (W + pad)].view(H, W + pad)[:, :W]
    w.copy_(torch.from_numpy(weight))
    assert froom.data_ptr() % 16 == 0 and wroom.data_ptr() % 16 == 0 and f.data_ptr() % 16 == shift % 16 and w.data_ptr() % 16 == shift % 16
    before = froom.clone(), wroom.clone()
    words = O.OpList.redact_scratch_words(mode, H, W, strength)
    obuf = torch.full((GUARD + 3 * H * W + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    out = obuf[GUARD:GUARD + 3 * H * W].view(H, W, 3)
    out.copy_(((torch.arange(3 * H * W, device='cuda') * 7 + 3) % 251).to(torch.uint8).view(H, W, 3))       # a sentinel pattern, not the answer
    sbuf = torch.full((GUARD + 4 * words + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    sbuf[GUARD:GUARD + 4 * words] = scratch_fill
    ol = O.OpList()
    ol.redact(f, w, out, sbuf[GUARD:GUARD + 4 * words].view(torch.int32), mode=mode, strength=strength, color=color, invert=invert)
    ol.run()
    torch.cuda.synchronize()
    assert torch.equal(froom, before[0]) and torch.equal(wroom, before[1])                            # read only, padding included
    for buf, size in ((obuf, 3 * H * W), (sbuf, 4 * words)):
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + size:] == FILL).all())
    return out.cpu().numpy()


_EFFECTS = {}


def _want(frame_key, frame, weight, mode, strength, color, invert):
    """The model's bytes; the effect of a (frame, mode, strength) is computed once and shared by the cases that blend it."""
    key = (frame_key, mode, strength, tuple(color))
    if key not in _EFFECTS:
        _EFFECTS[key] = R.effect(frame, mode, strength, color)
    return R.blend(frame, _EFFECTS[key], weight, invert)


def _check(kind, H, W, mode, strength=0, color=(0, 0, 0), invert=False, **kw):
    frame, weight = RC.make(kind, H, W)
    want = _want((H, W), frame, weight, mode, strength, color, invert)
    got = _device(frame, weight, mode, strength, color, invert, **kw)
    diff = np.flatnonzero(got != want)
    print(kind, (H, W), mode, strength, color, 'invert', invert, kw, 'differing bytes', diff.size)
    assert diff.size == 0, (kind, H, W, mode, strength, invert, kw, 'first difference at', np.unravel_index(diff[0], want.shape), int(got.flat[diff[0]]), int(want.flat[diff[0]]))
    return frame, weight, got


def test_form_is_announced():
    lib = _lib.load()
    assert lib.cutie_hip_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.cutie_hip_build_flags() & 1024 and _lib.has_redact()


@pytest.mark.parametrize('H,W', RC.SIZES, ids=str)
def test_blur(H, W):
    n = RC.SIZES.index((H, W))
    for k, r in enumerate(RC.RADII):                           # 2 r + 1 beyond the frame in one direction and in both among them
        _check(RC.WEIGHTS[2 + (n + k) % 2], H, W, 'blur', r, invert=bool((n + k) % 3 == 0))


@pytest.mark.parametrize('H,W', RC.SIZES, ids=str)
def test_pixelate(H, W):
    n = RC.SIZES.index((H, W))
    for k, c in enumerate(RC.CELLS):                           # c > W, and last partial cells of one pixel (65 = 4 * 16 + 1 = 32 * 2 + 1)
        _check(RC.WEIGHTS[2 + (n + k) % 2], H, W, 'pixelate', c, invert=bool((n + k) % 3 == 1))


@pytest.mark.parametrize('H,W', RC.SIZES, ids=str)
def test_fill(H, W):
    _check('noise', H, W, 'fill', color=(255, 0, 77))
    _check('blob', H, W, 'fill', color=(1, 254, 128), invert=True)


@pytest.mark.parametrize('mode,strength', [('blur', 7), ('pixelate', 3), ('fill', 0)])
def test_weight_planes_and_the_invert_bit(mode, strength):
    H, W = 65, 129
    for kind in RC.WEIGHTS:
        for invert in (False, True):
            frame, weight, got = _check(kind, H, W, mode, strength, (9, 200, 31), invert)
            keeps = (kind == 'zero' and not invert) or (kind == 'full' and invert)
            takes = (kind == 'full' and not invert) or (kind == 'zero' and invert)
            if keeps:
                assert np.array_equal(got, frame)              # w' == 0: the frame, exactly
            if takes:
                assert np.array_equal(got, R.effect(frame, mode, strength, (9, 200, 31)))
    const = np.full((H, W, 3), 201, np.uint8)                  # a constant frame comes back under blur and pixelate for every w
    if mode != 'fill':
        assert np.array_equal(_device(const, RC.weight('noise', H, W), mode, strength), const)


@pytest.mark.parametrize('mode,strength', [('blur', 2), ('blur', 31), ('blur', 64), ('pixelate', 2), ('pixelate', 17), ('fill', 0)])
def test_odd_addresses_and_padded_rows(mode, strength):
    for H, W in ((63, 65), (131, 200), (7, 17)):
        _check('noise', H, W, mode, strength, (5, 6, 7), shift=1, pad=7)
        _check('blob', H, W, mode, strength, (5, 6, 7), invert=True, shift=3, pad=1)


@pytest.mark.parametrize('mode,strength', [('blur', 7), ('blur', 64), ('pixelate', 3), ('pixelate', 256)])
def test_the_scratch_means_nothing_and_a_second_run_is_bit_identical(mode, strength):
    H, W = 131, 200
    frame, weight = RC.make('noise', H, W)
    a = _device(frame, weight, mode, strength, scratch_fill=0xff)
    b = _device(frame, weight, mode, strength, scratch_fill=0)
    c = _device(frame, weight, mode, strength, scratch_fill=0)
    assert np.array_equal(a, b) and np.array_equal(b, c) and np.array_equal(a, _want((H, W), frame, weight, mode, strength, (0, 0, 0), False))


def test_480p():
    H, W = 480, 854
    frame, weight = RC.make('blob', H, W)
    for mode, s in (('blur', 12), ('pixelate', 16)):
        assert np.array_equal(_device(frame, weight, mode, s), R.model(frame, weight, mode, s))


def test_launcher_refuses():
    H, W = 6, 10
    frame = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    weight = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    words = max(O.OpList.redact_scratch_words(m, H, W) for m in ('blur', 'pixelate', 'fill'))
    scratch = torch.zeros(words + 4, dtype=torch.int32, device='cuda')
    out.fill_(FILL)

    def run(ints, ptrs, flags=65536):
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, flags, ints, [], ptrs)
        ol.run()

    def ints(**kw):
        v = dict(H=H, W=W, s=3, ldf=3 * W, ldw=W, mode=0, hi=0, words=words, inv=0, color=0)
        v.update(kw)
        return [0, v['H'], v['W'], v['s'], v['ldf'], v['ldw'], v['mode'], v['hi'], v['words'], v['inv'], v['color']]

    good_p = [None, None, frame, out, None, scratch, weight]
    for mode, s in ((0, 1), (0, 64), (1, 2), (1, 256), (2, 0)):    # the limits are inside
        run(ints(mode=mode, s=s), good_p)
    torch.cuda.synchronize()
    out.fill_(FILL)

    def bad(match, i=None, p=None, **kw):
        with pytest.raises(Exception, match=match):
            run(ints() if i is None else i, good_p if p is None else p, **kw)

    bad('unknown flags', flags=65536 | 8)
    bad('unknown flags', flags=65536 | 32768)
    bad('H, W >= 1', i=ints(H=0))
    bad('H, W >= 1', i=ints(W=0))
    bad('H \\* W < 2\\^31', i=ints(H=1 << 16, W=1 << 15, ldf=3 << 15, ldw=1 << 15))
    bad('unknown mode 3', i=ints(mode=3))
    bad('unknown mode -1', i=ints(mode=-1))
    bad('blur radius 0', i=ints(s=0))
    bad('blur radius 65', i=ints(s=65))
    bad('pixelate cell 1', i=ints(mode=1, s=1))
    bad('pixelate cell 257', i=ints(mode=1, s=257))
    bad('invert bit', i=ints(inv=2))
    bad('invert bit', i=ints(color=1 << 24))
    for k in (2, 3, 5, 6):                                         # a null frame, out, scratch, weight
        p = list(good_p)
        p[k] = None
        bad('needs the frame', p=p)
    bad('frame row stride', i=ints(ldf=3 * W - 1))
    bad('weight row stride', i=ints(ldw=W - 1))
    bad('4-byte aligned', p=[None, None, frame, out, None, scratch.view(torch.uint8)[1:], weight])
    bad('negative scratch', i=ints(words=-1))
    bad('negative scratch', i=ints(hi=-1))
    bad('scratch of', i=ints(words=O.OpList.redact_scratch_words('blur', H, W) - 1))
    bad('scratch of', i=ints(mode=1, s=2, words=O.OpList.redact_scratch_words('pixelate', H, W, 2) - 1))
    bad('scratch of', i=ints(mode=2, words=0))
    bad('overlap', p=[None, None, frame, frame.view(-1), None, scratch, weight])
    bad('overlap', p=[None, None, frame, weight.view(-1)[H * W - 1:], None, scratch, weight])       # the output's first byte is the weight's last
    bad('overlap', p=[None, None, frame, scratch.view(torch.uint8), None, scratch, weight])
    bad('overlap', p=[None, None, scratch.view(torch.uint8)[8:], out, None, scratch, weight])
    bad('overlap', p=[None, None, frame, out, None, scratch, scratch.view(torch.uint8)[16:]])
    torch.cuda.synchronize()
    assert bool((out == FILL).all())                               # no refused descriptor launched anything


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.config import default_config
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


@pytest.fixture(scope='module')
def bike(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('redact'))
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(2):
        shutil.copy(os.path.join(HERE, 'golden', 'bike', f'{t:05d}.jpg'), os.path.join(root, 'frames', f'{t:07d}.jpg'))
    shutil.copy(os.path.join(HERE, 'golden', 'bike', '00000.png'), os.path.join(root, 'masks', '0000000.png'))
    return root


def _jpeg_file(rgb):
    import jpeg_enc_ref
    from cutie_amd.inference.utils import jpeg_writer
    qt = jpeg_writer.quant_tables(jpeg_writer.QUALITY)
    return jpeg_writer.wrap(jpeg_enc_ref.encode(rgb, qt=qt), rgb.shape[0], rgb.shape[1], qt)


@pytest.mark.parametrize('case', ['blur_grow', 'pixelate_background_matte'])
def test_process_video_redacts(gpu_net, bike, case):
    """--redact blur --redact-grow 2 (host egress) and --redact pixelate --redact-background --redact-edge matte --alpha (device egress) on
    two bike frames: every redacted JPEG decodes and is, byte for byte, the JPEG model's file of the redaction model's frame under the
    weight plane built from the run's own mask PNG (dilated by the distance model) or its own alpha PNG."""
    import edt_ref
    from cutie_amd.process_video import arg_parser, process_video, redact_args, video_config
    ap = arg_parser()
    base = ['-v', 'v', '-m', 'm', '-o', 'o']
    if case == 'blur_grow':
        args = ap.parse_args(base + ['--redact', 'blur', '--redact-grow', '2'])
        kw = dict(egress='host')
    else:
        args = ap.parse_args(base + ['--redact', 'pixelate', '--redact-background', '--redact-edge', 'matte', '--alpha'])
        kw = dict(egress='device', alpha_matte=True)
    redact = redact_args(ap, args)
    out = os.path.join(bike, case)
    r = process_video(gpu_net, video_config(mem_every=2), os.path.join(bike, 'frames'), os.path.join(bike, 'masks'), out, ingest='device', redact=redact, **kw)
    assert r['frames'] == 2 and os.path.join(out, 'redacted') in r['folders']
    assert sorted(os.listdir(os.path.join(out, 'redacted'))) == ['0000000.jpg', '0000001.jpg']
    changed = 0
    for t in range(2):
        stem = f'{t:07d}'
        frame = np.array(Image.open(os.path.join(bike, 'frames', stem + '.jpg')).convert('RGB'))
        got = Image.open(os.path.join(out, 'redacted', stem + '.jpg'))
        assert got.format == 'JPEG' and got.mode == 'RGB' and got.size == (frame.shape[1], frame.shape[0])
        got.load()                                             # decodes
        if case == 'blur_grow':
            ids = np.array(Image.open(os.path.join(out, stem + '.png')))
            sets = np.zeros((1, 256), np.uint8)
            sets[0, [int(v) for v in np.unique(np.array(Image.open(os.path.join(bike, 'masks', '0000000.png')))) if v]] = 1
            weight = edt_ref.edt_band(ids, sets, 0, 4, 255, 5)[1][0]
            want = R.model(frame, weight, 'blur', 12)
        else:
            weight = np.array(Image.open(os.path.join(out, 'alpha', stem + '.png')))
            want = R.model(frame, weight, 'pixelate', 16, invert=True)
        changed += int(not np.array_equal(want, frame))
        assert open(os.path.join(out, 'redacted', stem + '.jpg'), 'rb').read() == _jpeg_file(want), (case, stem)
    assert changed > 0                                         # the effect changed something
