"""The colour guided filter on the MI355X (PROB_TO_ID flags == 32768, csrc/guided.hip) against the model (tests/guided_ref.py): the bytes
are equal -- at every size around the kernels' tile dimensions, every radius class, eps, plane count and content; guard regions around the
output and the scratch survive, the guide and the planes come back unchanged, at aligned addresses and at +1 byte, with padded row strides;
a second run is bit-identical.  The launcher's refusals, the feature bit, and process_video on the bike frames with --refine-matte."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import guided_cases as GC                                  # noqa: E402
import guided_ref as G                                     # noqa: E402

from cutie_amd import _lib, ops as O                       # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, FILL = 4096, 0x5a
TX, TY, T = O.OpList.GUIDED_TILE_X, O.OpList.GUIDED_TILE_Y, O.OpList.GUIDED_THREADS


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device(guide, planes, r, eps, *, shift=0, pad=0, split_last=False):
    """The stage on one case -> the output bytes [S, H, W].  ``shift``: the guide and the planes start ``shift`` bytes behind a 16-byte
    aligned address; ``pad``: extra bytes per row of the guide and of the planes (and 5 rows between planes); ``split_last``: the last
    plane travels in a tensor of its own (p7).  Output and scratch sit between guards that must survive; the inputs stay as they were."""
    S, H, W = planes.shape
    groom = torch.full((shift + H * (3 * W + pad) + 16,), 0xa5, dtype=torch.uint8, device='cuda')
    g = groom[shift:shift + H * (3 * W + pad)].view(H, 3 * W + pad)[:, :3 * W].view(H, W, 3)
    g.copy_(torch.from_numpy(guide))
    S0 = S - 1 if split_last else S
    ldp, rows = W + pad, H + (5 if pad else 0)
    proom = torch.full((shift + max(S0, 1) * rows * ldp + 16,), 0xa5, dtype=torch.uint8, device='cuda')
    p = proom[shift:shift + max(S0, 1) * rows * ldp].view(max(S0, 1), rows, ldp)[:S0, :H, :W]
    p.copy_(torch.from_numpy(planes[:S0]))
    last = torch.from_numpy(planes[S - 1].copy()).cuda() if split_last else None
    assert groom.data_ptr() % 16 == 0 and proom.data_ptr() % 16 == 0 and g.data_ptr() % 16 == shift % 16
    before = groom.clone(), proom.clone(), (last.clone() if last is not None else None)
    words = O.OpList.guided_scratch_words(S, H, W)
    obuf = torch.full((GUARD + S * H * W + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    sbuf = torch.full((GUARD + 4 * words + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    out = obuf[GUARD:GUARD + S * H * W].view(S, H, W)
    ol = O.OpList()
    ol.guided_filter(g, p if S0 else None, out, sbuf[GUARD:GUARD + 4 * words].view(torch.int32), radius=r, eps=eps, last=last)
    ol.run()
    torch.cuda.synchronize()
    assert torch.equal(groom, before[0]) and torch.equal(proom, before[1]) and (last is None or torch.equal(last, before[2]))    # read only
    for buf, size in ((obuf, S * H * W), (sbuf, 4 * words)):
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + size:] == FILL).all())
    return out.cpu().numpy()


def _check(kind, H, W, S, r, eps, **kw):
    guide, planes = GC.make(kind, H, W, S)
    want = G.model(guide, planes, r, eps)
    got = _device(guide, planes, r, eps, **kw)
    diff = np.flatnonzero(got != want)
    print(kind, (H, W), 'S', S, 'r', r, 'eps', eps, kw, 'differing bytes', diff.size)
    assert diff.size == 0, (kind, H, W, S, r, eps, kw, 'first difference at', np.unravel_index(diff[0], want.shape), int(got.flat[diff[0]]), int(want.flat[diff[0]]))
    return guide, planes, got


def test_form_is_announced():
    lib = _lib.load()
    assert lib.cutie_hip_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.cutie_hip_build_flags() & 512 and _lib.has_guided_filter()


# one less than, exactly, one more than and twice plus one of every exported tile dimension, on both axes; 1 x 1, 1 x W, H x 1
AROUND = sorted({d + k for d in (TX, TY, T) for k in (-1, 0, 1)} | {2 * d + 1 for d in (TX, TY, T)})
SHAPES = [(1, 1), (1, 37), (41, 1), (1, 2 * TX + 1), (2 * TY + 1, 1)] + [(n, 19) for n in AROUND] + [(11, n) for n in AROUND]


@pytest.mark.parametrize('H,W', SHAPES, ids=lambda v: str(v))
def test_shapes_around_the_tiles(H, W):
    n = SHAPES.index((H, W))
    _check('noise', H, W, 3, 5, 1e-4, shift=n % 2, pad=(7 if n % 3 == 0 else 0), split_last=bool(n % 4 == 1))
    _check('noise', H, W, 1, 64, 1e-6)


@pytest.mark.parametrize('r', list(dict.fromkeys([1, 2, TY - 1, TY, 64, 40])))
def test_radii(r):
    if r == 40:
        _check('noise', 23, 31, 2, r, 1e-4, shift=1)          # a radius beyond both H and W: every window is the frame
    else:
        _check('noise', 97, 131, 2, r, 1e-4, shift=1, pad=3)
        _check('edge', 2 * TY + 1, TX + 1, 1, r, 1e-4)


@pytest.mark.parametrize('eps', [1e-6, 1e-4, 1e-2, 1.0])
def test_eps(eps):
    _check('noise', 97, 131, 2, 7, eps)
    _check('grey_guide', 97, 131, 2, 7, eps, shift=1, pad=1)


@pytest.mark.parametrize('S', [1, 3, 16])
def test_plane_counts(S):
    _check('noise', 70, 140, S, 6, 1e-4)
    _check('noise', 70, 140, S, 6, 1e-4, split_last=True, shift=1)


@pytest.mark.parametrize('kind', GC.CONTENTS)
def test_contents(kind):
    r = 64 if kind == 'all255' else 9                          # all-255 at r = 64: the largest sums
    guide, planes, got = _check(kind, 2 * TY + 3, 2 * TX + 5, 2, r, 1e-6 if kind in ('grey_guide', 'constant_channel') else 1e-4)
    if kind in ('constant_plane', 'all255', 'zero'):
        assert np.array_equal(got, planes)                     # a constant plane comes back exactly
    if kind == 'edge':
        before, after = GC.edge_slopes(guide, planes[0], got[0])
        print('rise across the guide\'s edge: input', before, 'refined', after)
        assert after > before


def test_a_second_run_is_bit_identical_and_480p():
    guide, planes = GC.make('noise', 480, 854, 2)
    want = G.model(guide, planes, 16, 1e-4)
    a = _device(guide, planes, 16, 1e-4)
    b = _device(guide, planes, 16, 1e-4, split_last=True)
    assert np.array_equal(a, want) and np.array_equal(b, want)


def test_launcher_refuses():
    H, W, S = 6, 10, 2
    guide = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    planes = torch.zeros((S, H, W), dtype=torch.uint8, device='cuda')
    last = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    out = torch.zeros((S + 1, H, W), dtype=torch.uint8, device='cuda')
    words = O.OpList.guided_scratch_words(S + 1, H, W)
    scratch = torch.zeros(words + 4, dtype=torch.int32, device='cuda')

    def run(ints, ptrs, flags=32768, eps=1e-4):
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, flags, ints, [eps], ptrs)
        ol.run()

    def ints(**kw):
        v = dict(H=H, W=W, r=3, ldg=3 * W, ldp=W, ps=H * W, hi=0, words=words, S0=S, ldl=W)
        v.update(kw)
        return [0, v['H'], v['W'], v['r'], v['ldg'], v['ldp'], v['ps'], v['hi'], v['words'], v['S0'], v['ldl']]

    good_p = [None, None, guide, out, None, scratch, planes, last]
    run(ints(), good_p)
    torch.cuda.synchronize()

    def bad(match, i=None, p=None, **kw):
        with pytest.raises(Exception, match=match):
            run(ints() if i is None else i, good_p if p is None else p, **kw)

    bad('unknown flags', flags=32768 | 8)
    bad('unknown flags', flags=32768 | 16384)
    bad('H, W >= 1', i=ints(H=0))
    bad('H \\* W < 2\\^31', i=ints(H=1 << 16, W=1 << 15, ldg=3 << 15, ldp=1 << 15, ldl=1 << 15))
    bad('radius 0', i=ints(r=0))
    bad('radius 65', i=ints(r=65))
    bad('eps', eps=5e-7)
    bad('eps', eps=1.5)
    bad('eps', eps=float('nan'))
    bad('17 planes', i=ints(S0=16))
    bad('-1 planes', i=ints(S0=-1))
    bad('0 planes', i=ints(S0=0), p=[None, None, guide, out, None, scratch, planes, None])
    bad('needs the guide', p=[None, None, None, out, None, scratch, planes, last])
    bad('needs the guide', p=[None, None, guide, None, None, scratch, planes, last])
    bad('needs the guide', p=[None, None, guide, out, None, None, planes, last])
    bad('needs the guide', p=[None, None, guide, out, None, scratch, None, last])
    bad('guide row stride', i=ints(ldg=3 * W - 1))
    bad('plane strides', i=ints(ldp=W - 1))
    bad('plane strides', i=ints(ps=H * W - 1))
    bad('plane strides', i=ints(ldl=W - 1))
    bad('4-byte aligned', p=[None, None, guide, out, None, scratch.view(torch.uint8)[1:], planes, last])
    bad('negative scratch', i=ints(words=-1))
    bad('scratch of', i=ints(words=words - 1))
    bad('overlap', p=[None, None, guide, planes.view(-1)[H * W - 1:], None, scratch, planes, last])        # the output's first byte is the planes' last
    bad('overlap', p=[None, None, guide, guide.view(-1), None, scratch, planes, last])
    bad('overlap', p=[None, None, guide, last.view(-1), None, scratch, planes, last])
    bad('overlap', p=[None, None, guide, scratch.view(torch.uint8), None, scratch, planes, last])
    torch.cuda.synchronize()


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
    root = str(tmp_path_factory.mktemp('guided'))
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(3):
        shutil.copy(os.path.join(HERE, 'golden', 'bike', f'{t:05d}.jpg'), os.path.join(root, 'frames', f'{t:07d}.jpg'))
    shutil.copy(os.path.join(HERE, 'golden', 'bike', '00000.png'), os.path.join(root, 'masks', '0000000.png'))
    return root


def _files(root):
    return {os.path.relpath(os.path.join(dp, f), root).replace(os.sep, '/'): os.path.join(dp, f) for dp, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize('egress', ['host', 'device'])
def test_process_video_refines_the_mattes(gpu_net, bike, egress):
    """--alpha --cutout --soft-masks --refine-matte 8 on the bike frames: every refined file holds the model applied to the file of a run
    without the switch, with the decoded frame as the guide; the id masks keep their bytes, and so does the unrefined run's alpha
    against a second unrefined run (png_codes fixed)."""
    from cutie_amd.process_video import process_video, video_config
    cfg = video_config(mem_every=2)
    args = (os.path.join(bike, 'frames'), os.path.join(bike, 'masks'))
    kw = dict(ingest='device', egress=egress, soft_masks=True, alpha_matte=True, cutout=True, png_codes='fixed')

    def run(tag, **more):
        out = os.path.join(bike, f'{tag}_{egress}')
        assert process_video(gpu_net, cfg, *args, out, **kw, **more)['frames'] == 3
        return _files(out)
    plain, again, fine = run('plain'), run('again'), run('fine', matte_refine=(8, 1e-4))
    assert sorted(plain) == sorted(fine) == sorted(again) and any(k.startswith('alpha/') for k in plain) and any(k.startswith('soft_masks/') for k in plain)
    checked = 0
    for name in sorted(plain):
        raw = lambda files: open(files[name], 'rb').read()
        if '/' not in name:                                                       # the id masks: the same bytes with and without the switch
            assert raw(plain) == raw(fine) == raw(again), name
            continue
        assert raw(plain) == raw(again), name                                     # without the switch: the bytes of any other such run
        frame = np.array(Image.open(os.path.join(bike, 'frames', os.path.basename(name)[:-4] + '.jpg')).convert('RGB'))
        a, b = np.array(Image.open(plain[name])), np.array(Image.open(fine[name]))
        if name.startswith('cutout/'):
            assert np.array_equal(b[..., :3], frame) and np.array_equal(a[..., :3], frame)
            assert np.array_equal(b[..., 3], np.array(Image.open(fine['alpha/' + os.path.basename(name)])))
            continue
        want = G.model(frame, a[None], 8, 1e-4)[0]
        assert np.array_equal(b, want), name
        checked += int(not np.array_equal(a, b))
    assert checked > 0                                                            # the filter changed something
