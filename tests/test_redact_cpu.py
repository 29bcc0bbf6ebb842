"""Redacted frames (PROB_TO_ID flags == 65536) without a GPU: the numpy model of the contract (tests/redact_ref.py) against its brute-force
restatement, its exact properties, OpList.redact and the descriptor through tests/mock_exec_redact.py, ResultSaver(redact=...) over the
frames of tests/png_photo_saver_case.py, and the parser of process_video.  The stage adds no host-side C++ (csrc/redact.hip holds kernels
and their launcher only), so there is nothing for a sanitizer build to run.

On the commit before the stage existed the OpList.redact tests (test_descriptor_*, test_refusal, test_a_stale_library_is_named), the saver
tests (test_saver_*, test_bad_saver_arguments) and the parser test fail: the names do not exist."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.inference.utils import jpeg_writer
from cutie_amd.inference.utils import results_utils as RU

import edt_ref
import jpeg_enc_ref
import matte_ref as M
import redact_cases as RC
import redact_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the model against loops over windows and cells ---------------------------------------------------------------------------------------
BRUTE_SIZES = [(1, 1), (1, 7), (6, 1), (2, 3), (5, 4), (9, 11)]


@pytest.mark.parametrize('H,W', BRUTE_SIZES, ids=str)
def test_model_against_brute_force(H, W):
    frame, w = RC.make('noise', H, W, seed=2)
    for r in (1, 2, 5):                                        # r = 5 >= H or W for most sizes: the window is the whole row or column
        assert np.array_equal(R.box_pass(frame, r), R.brute_box_pass(frame, r))
        for inv in (False, True):
            assert np.array_equal(R.model(frame, w, 'blur', r, invert=inv), R.brute_model(frame, w, 'blur', r, invert=inv)), (r, inv)
    for c in (2, 3, 4, 16):                                    # dividing, not dividing, larger than the frame
        assert np.array_equal(R.pixelate(frame, c), R.brute_pixelate(frame, c))
        for inv in (False, True):
            assert np.array_equal(R.model(frame, w, 'pixelate', c, invert=inv), R.brute_model(frame, w, 'pixelate', c, invert=inv)), (c, inv)
    for inv in (False, True):
        assert np.array_equal(R.model(frame, w, 'fill', color=(7, 200, 255), invert=inv), R.brute_model(frame, w, 'fill', color=(7, 200, 255), invert=inv))


def test_one_pass_is_one_rounding_not_two():
    """A rounded row mean followed by a rounded column mean differs from the contract's single rounding somewhere on noise."""
    frame = RC.frame(9, 11, seed=5)
    a = frame.astype(np.int64)
    r, (H, W) = 1, frame.shape[:2]
    rows = np.zeros_like(a)
    for x in range(W):
        lo, hi = max(0, x - r), min(W - 1, x + r) + 1
        n = hi - lo
        rows[:, x] = (2 * a[:, lo:hi].sum(1) + n) // (2 * n)
    two = np.zeros_like(a)
    for y in range(H):
        lo, hi = max(0, y - r), min(H - 1, y + r) + 1
        n = hi - lo
        two[y] = (2 * rows[lo:hi].sum(0) + n) // (2 * n)
    assert not np.array_equal(two.astype(np.uint8), R.box_pass(frame, r))


# ---- exact properties -------------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    rng = np.random.default_rng(11)
    H, W = 23, 31
    frame, noise = RC.make('noise', H, W, seed=3)
    zero, full = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    for mode, s in (('blur', 1), ('blur', 7), ('blur', 64), ('pixelate', 2), ('pixelate', 5), ('pixelate', 256), ('fill', 0)):
        assert np.array_equal(R.model(frame, zero, mode, s, (9, 8, 7)), frame)                               # w == 0: the frame
        assert np.array_equal(R.model(frame, full, mode, s, (9, 8, 7), invert=True), frame)
        assert np.array_equal(R.model(frame, full, mode, s, (9, 8, 7)), R.effect(frame, mode, s, (9, 8, 7)))  # w == 255: the effect
        assert np.array_equal(R.model(frame, noise, mode, s, (9, 8, 7), invert=True), R.model(frame, 255 - noise, mode, s, (9, 8, 7)))
        e, out = R.effect(frame, mode, s, (9, 8, 7)), R.model(frame, noise, mode, s, (9, 8, 7))
        assert (out >= np.minimum(e, frame)).all() and (out <= np.maximum(e, frame)).all()                   # the blend stays between e and f
    assert np.array_equal(R.model(frame, full, 'fill', color=(1, 2, 3)), np.broadcast_to(np.array([1, 2, 3], np.uint8), frame.shape))
    for v in (0, 1, 128, 254, 255):                                                                           # a constant frame comes back
        const = np.full((H, W, 3), v, np.uint8)
        const[..., 1] = 255 - v
        for mode, s in (('blur', 3), ('blur', 64), ('pixelate', 4), ('pixelate', 7)):
            w = rng.integers(0, 256, (H, W), dtype=np.uint8)
            assert np.array_equal(R.model(const, w, mode, s), const), (v, mode, s)
    for r in (1, 4, 40):                                                                                      # blur commutes with flips
        for ax in (0, 1):
            a = R.model(np.ascontiguousarray(np.flip(frame, ax)), np.ascontiguousarray(np.flip(noise, ax)), 'blur', r)
            assert np.array_equal(np.flip(a, ax), R.model(frame, noise, 'blur', r))
    for c in (31, 32, 256):                                                                                   # one cell: the rounded mean of the image
        n = H * W
        mean = (2 * frame.astype(np.int64).sum((0, 1)) + n) // (2 * n)
        assert np.array_equal(R.pixelate(frame, c), np.broadcast_to(mean.astype(np.uint8), frame.shape))
    assert np.array_equal(R.blur(frame, 31), R.blur(frame, 64))                                              # r >= max(H, W) - 1: every window is the frame
    assert len(np.unique(R.blur(frame, 31).reshape(-1, 3), axis=0)) == 1


# ---- descriptor and arguments -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def executor():
    from mock_exec_redact import RedactMockExecutor
    ex = RedactMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(jpeg_enc_ref.EncodeExecutor(M.MatteExecutor(ex)))
    yield ex
    _lib.set_executor_for_testing(None)


def _tensors(H=9, W=13, pad=5):
    frame_np, w_np = RC.make('noise', H, W)
    room = torch.zeros((H, 3 * W + pad), dtype=torch.uint8)
    frame = room[:, :3 * W].view(H, W, 3)
    frame.copy_(torch.from_numpy(frame_np))
    wroom = torch.zeros((H, W + 3), dtype=torch.uint8)
    weight = wroom[:, :W]
    weight.copy_(torch.from_numpy(w_np))
    out = torch.zeros((H, W, 3), dtype=torch.uint8)
    scratch = torch.zeros(max(O.OpList.redact_scratch_words(m, H, W) for m in ('blur', 'pixelate', 'fill')), dtype=torch.int32)
    return frame_np, w_np, room, frame, wroom, weight, out, scratch


def test_descriptor_through_the_mock(executor):
    frame_np, w_np, room, frame, wroom, weight, out, scratch = _tensors()
    H, W = w_np.shape
    for mode, s, color, inv in (('blur', 3, (0, 0, 0), False), ('blur', 64, (0, 0, 0), True), ('pixelate', 2, (0, 0, 0), False),
                                ('pixelate', 256, (0, 0, 0), True), ('fill', 0, (255, 1, 128), False), ('fill', 0, (3, 4, 5), True)):
        ol = O.OpList()
        ol.redact(frame, weight, out, scratch, mode=mode, strength=s, color=color, invert=inv)
        ol.run()
        assert executor.redact_calls[-1] == (H, W, R.MODES[mode], s, color, int(inv))
        assert np.array_equal(out.numpy(), R.model(frame_np, w_np, mode, s, color, inv))
    rec = ol.finalize()[0]
    assert int(rec['kind']) == O.PROB_TO_ID and int(rec['flags']) == 65536
    assert [int(v) for v in rec['i'][:11]] == [0, H, W, 0, 3 * W + 5, W + 3, 2, 0, scratch.numel(), 1, 3 | 4 << 8 | 5 << 16]
    assert [int(v) for v in rec['p'][:7]] == [0, 0, frame.data_ptr(), out.data_ptr(), 0, scratch.data_ptr(), weight.data_ptr()]
    ol = O.OpList()                                                                             # 65536 is a stage on its own
    ol.add(O.PROB_TO_ID, 65536 | 8, [0, H, W, 3, 3 * W, W, 0, 0, scratch.numel(), 0, 0], [], [None, None, frame, out, None, scratch, weight])
    with pytest.raises(Exception):
        ol.run()


def test_constants_and_sources():
    assert (O.OpList.REDACT_MAX_RADIUS, O.OpList.REDACT_MAX_CELL) == (R.MAX_RADIUS, R.MAX_CELL) == (64, 256)
    assert O.OpList.REDACT_MODES == R.MODES
    assert O.OpList.redact_scratch_words('blur', 5, 7) == 2 * 27 and O.OpList.redact_scratch_words(0, 5, 7) == 54
    assert O.OpList.redact_scratch_words('pixelate', 5, 7, 3) == 2 * 21 + 5 and O.OpList.redact_scratch_words('fill', 5, 7) == 1
    assert all(O.OpList.redact_scratch_words('pixelate', 37, 53) >= O.OpList.redact_scratch_words('pixelate', 37, 53, c) for c in range(2, 257))
    with pytest.raises(ValueError, match='redact_scratch_words'):
        O.OpList.redact_scratch_words('sharpen', 5, 7)
    src = open(os.path.join(HERE, '..', 'include', 'cutie_hip.h')).read()
    assert 'flags == 65536' in src and 'bit 10 (value 1024)' in src and 'CUTIE_REDACT_MAX_RADIUS 64' in src and 'CUTIE_REDACT_MAX_CELL 256' in src
    kern = open(os.path.join(HERE, '..', 'cutie_amd', 'csrc', 'redact.hip')).read()
    assert f'#define RD_T {O.OpList.REDACT_THREADS} ' in kern and '#define RD_RMAX 64 ' in kern and '#define RD_CMAX 256 ' in kern
    assert f'#define RD_TY_SMALL {O.OpList.REDACT_TILE_Y[0]} ' in kern and f'#define RD_TY_LARGE {O.OpList.REDACT_TILE_Y[1]} ' in kern
    assert f'#define RD_R_SMALL {O.OpList.REDACT_SMALL_RADIUS}\n' in kern
    assert 'int launch_redact' in kern and 'redact.hip' in open(os.path.join(HERE, '..', 'cutie_amd', 'csrc', 'Makefile')).read()
    assert '65536' in open(os.path.join(HERE, '..', 'INTEGRATION.md')).read()
    assert callable(_lib.has_redact)


def _refusals(frame_np, w_np, room, frame, wroom, weight, out, scratch):
    H, W = w_np.shape
    return [
        ('frame is uint8', dict(frame=frame.float())),
        ('frame is uint8', dict(frame=torch.zeros((H, W, 4), dtype=torch.uint8))),
        ('H, W >= 1', dict(frame=torch.zeros((0, W, 3), dtype=torch.uint8))),
        ('mode is one of', dict(mode='sharpen')),
        ('strength is an integer', dict(strength=2.5)),
        ('blur radius 0', dict(strength=0)),
        ('blur radius 65', dict(strength=65)),
        ('pixelate cell 1', dict(mode='pixelate', strength=1)),
        ('pixelate cell 257', dict(mode='pixelate', strength=257)),
        ('color is three bytes', dict(mode='fill', color=(1, 2))),
        ('color is three bytes', dict(mode='fill', color=(1, 2, 256))),
        ('frame row stride', dict(ldrow=3 * W - 1)),
        ('weight is a uint8', dict(weight=weight.int())),
        ('weight is a uint8', dict(weight=weight[:, :W - 1])),
        ('weight is a uint8', dict(weight=torch.zeros((H, 2 * W), dtype=torch.uint8)[:, ::2])),
        ('weight row stride', dict(ldw=W - 1)),
        ('out is a contiguous', dict(out=out.int())),
        ('out is a contiguous', dict(out=torch.zeros((H, W + 1, 3), dtype=torch.uint8)[:, :W])),
        ('scratch is a contiguous int32', dict(scratch=scratch[:5])),
        ('scratch is a contiguous int32', dict(scratch=scratch.float())),
        ('out overlaps frame', dict(out=room.view(-1)[:H * W * 3].view(H, W, 3))),
        ('out overlaps weight', dict(out=torch.zeros(4 * H * W, dtype=torch.uint8), weight=None, _alias='weight in out')),
        ('scratch overlaps frame', dict(scratch=None, _alias='frame in scratch')),
        ('scratch overlaps out', dict(scratch=None, _alias='out in scratch')),
    ]


@pytest.mark.parametrize('n', range(24))
def test_refusal(n):
    """One refusal of OpList.redact per case, by its message."""
    frame_np, w_np, room, frame, wroom, weight, out, scratch = tensors = _tensors()
    H, W = w_np.shape
    cases = _refusals(*tensors)
    assert len(cases) == 24
    match, bad = cases[n]
    kw = dict(frame=frame, weight=weight, out=out, scratch=scratch, mode='blur', strength=3)
    alias = bad.pop('_alias', None)
    kw.update(bad)
    if alias == 'weight in out':
        big = kw['out']
        kw['out'], kw['weight'] = big[:3 * H * W].view(H, W, 3), big[3 * H * W - 1:][:H * W].view(H, W)
    elif alias == 'frame in scratch':
        big = torch.zeros(2 * scratch.numel(), dtype=torch.int32)
        kw['scratch'], kw['frame'] = big, big.view(torch.uint8)[8:8 + 3 * H * W].view(H, W, 3)
    elif alias == 'out in scratch':
        big = torch.zeros(2 * scratch.numel(), dtype=torch.int32)
        kw['scratch'], kw['out'] = big, big.view(torch.uint8)[4:4 + 3 * H * W].view(H, W, 3)
    with pytest.raises(ValueError, match='redact: .*' + match):
        O.OpList().redact(kw.pop('frame'), kw.pop('weight'), kw.pop('out'), kw.pop('scratch'), **kw)


def test_a_stale_library_is_named(monkeypatch):
    monkeypatch.setattr(_lib, '_executor', None)
    monkeypatch.setattr(_lib, 'has_redact', lambda: False)
    with pytest.raises(_lib.HipLibraryError, match='65536'):
        O.OpList().redact(torch.zeros((2, 2, 3), dtype=torch.uint8), None, None, None, mode='fill')


# ---- saver ------------------------------------------------------------------------------------------------------------------------------------
def _jpeg_file(rgb):
    H, W = rgb.shape[:2]
    qt = jpeg_writer.quant_tables(jpeg_writer.QUALITY)
    return jpeg_writer.wrap(jpeg_enc_ref.encode(rgb, qt=qt), H, W, qt)


def _union(plane, targets):
    sets = np.zeros((1, 256), np.uint8)
    sets[0, list(targets)] = 1
    return sets


@pytest.mark.parametrize('egress', ['host', 'device'])
@pytest.mark.parametrize('grow', [0.0, 2.5])
def test_saver_writes_redacted_frames_under_the_dilated_mask(tmp_path, executor, egress, grow):
    import png_photo_saver_case as S
    cfg = dict(mode='blur', strength=3, grow=grow)
    files = S.run(str(tmp_path / 'r'), 'cpu', egress=egress, redact=cfg)
    assert sorted(files) == sorted([f'vid/{t:05d}.png' for t in range(3)] + [f'vid/redacted/{t:05d}.jpg' for t in range(3)])
    assert executor.redact_calls == [(S.H, S.W, 0, 3, (0, 0, 0), 0)] * 3 and len(executor.redact_log) == 3
    outer = int(grow * grow)
    for t, fr in enumerate(S.frames()):
        ids = np.array(Image.open(files[f'vid/{t:05d}.png']))                      # the id plane the mask PNG was written from
        want_w = edt_ref.edt_band(ids, _union(ids, (5, 3)), 0, outer, 255, outer + 1)[1][0]
        frame, weight, out = executor.redact_log[t]
        assert np.array_equal(frame, fr) and np.array_equal(weight, want_w) and set(np.unique(weight)) <= {0, 255}
        if grow == 0.0:
            assert np.array_equal(weight != 0, ids != 0)
        else:
            assert (weight != 0).sum() > (ids != 0).sum()
        want = R.model(fr, want_w, 'blur', 3)
        assert np.array_equal(out, want)
        data = open(files[f'vid/redacted/{t:05d}.jpg'], 'rb').read()
        assert data == _jpeg_file(want)                                            # header, tables and the entropy segment of the model's frame
        im = Image.open(files[f'vid/redacted/{t:05d}.jpg'])
        assert im.size == (S.W, S.H) and im.mode == 'RGB' and im.format == 'JPEG'


def test_saver_targets_background_and_the_other_modes(tmp_path, executor):
    import png_photo_saver_case as S
    files = S.run(str(tmp_path / 'p'), 'cpu', redact=dict(mode='pixelate', strength=8, targets=[3, 99], background=True))
    assert executor.redact_calls == [(S.H, S.W, 1, 8, (0, 0, 0), 1)] * 3
    for t, fr in enumerate(S.frames()):
        ids = np.array(Image.open(files[f'vid/{t:05d}.png']))
        frame, weight, out = executor.redact_log[t]
        assert np.array_equal(weight != 0, ids == 3)                               # the target alone; an id that is not there is ignored
        assert open(files[f'vid/redacted/{t:05d}.jpg'], 'rb').read() == _jpeg_file(R.model(fr, weight, 'pixelate', 8, invert=True))
    executor.redact_calls.clear(); executor.redact_log.clear()
    files = S.run(str(tmp_path / 'f'), 'cpu', egress='device', redact=dict(mode='fill', color=(255, 0, 128), grow=1))
    assert executor.redact_calls == [(S.H, S.W, 2, 0, (255, 0, 128), 0)] * 3
    for t, fr in enumerate(S.frames()):
        assert open(files[f'vid/redacted/{t:05d}.jpg'], 'rb').read() == _jpeg_file(R.model(fr, executor.redact_log[t][1], 'fill', color=(255, 0, 128)))
    s = S.saver(str(tmp_path / 'd'), 'cpu', redact=dict(mode='blur'))              # the defaults
    try:
        assert s.redact == dict(mode='blur', strength=12, color=(0, 0, 0), grow=0.0, edge='mask', background=False, targets=None)
    finally:
        s.end()
    s = S.saver(str(tmp_path / 'd'), 'cpu', redact=dict(mode='pixelate'))
    try:
        assert s.redact['strength'] == 16
    finally:
        s.end()


@pytest.mark.parametrize('with_alpha', [True, False])
def test_saver_under_the_matte(tmp_path, executor, with_alpha):
    """edge='matte': the weight plane is the targets' matte -- the alpha file of the same run, or the plane composed for the stage alone."""
    import png_photo_saver_case as S
    plain = S.run(str(tmp_path / 'a'), 'cpu', alpha_matte=True, target_objects=[3])
    kw = dict(alpha_matte=True, target_objects=[3]) if with_alpha else {}
    files = S.run(str(tmp_path / 'b'), 'cpu', redact=dict(mode='blur', strength=5, edge='matte', targets=[3], background=True), **kw)
    for t, fr in enumerate(S.frames()):
        alpha = np.array(Image.open(plain[f'vid/alpha/{t:05d}.png']))
        frame, weight, out = executor.redact_log[t]
        assert np.array_equal(weight, alpha) and len(np.unique(weight)) > 16       # a soft plane
        assert open(files[f'vid/redacted/{t:05d}.jpg'], 'rb').read() == _jpeg_file(R.model(fr, alpha, 'blur', 5, invert=True))
        if with_alpha:
            assert open(files[f'vid/alpha/{t:05d}.png'], 'rb').read() == open(plain[f'vid/alpha/{t:05d}.png'], 'rb').read()


def test_saver_under_the_refined_matte(tmp_path, executor):
    import guided_ref as G
    import png_photo_saver_case as S
    fine = S.run(str(tmp_path / 'a'), 'cpu', alpha_matte=True, matte_refine=(4, 1e-4))
    S.run(str(tmp_path / 'b'), 'cpu', alpha_matte=True, matte_refine=(4, 1e-4), redact=dict(mode='fill', edge='matte'))
    S.run(str(tmp_path / 'c'), 'cpu', soft_masks=True, matte_refine=(4, 1e-4), redact=dict(mode='fill', edge='matte'))    # no matte output: composed and refined here
    assert len(executor.redact_log) == 6
    for t in range(3):
        want = np.array(Image.open(fine[f'vid/alpha/{t:05d}.png']))
        assert np.array_equal(executor.redact_log[t][1], want) and np.array_equal(executor.redact_log[3 + t][1], want)


class _Recorder:
    """Wraps an executor and keeps (kind, flags) of every descriptor."""
    is_mock = True

    def __init__(self, inner):
        self.inner, self.ops = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def stream(self):
        return 0

    def run(self, arr):
        for rec in arr:
            self.ops.append((int(rec['kind']), int(rec['flags'])))
        return self.inner.run(arr)


def test_a_saver_without_the_switch_issues_what_it_issued_before(tmp_path, executor):
    """The op lists of the default paths as tests/test_guided_cpu.py records them: no descriptor more, none less; no 65536 and no buffer set
    of the stage without the switch.  With it: the distance stage, the stage and the JPEG stage join behind the frame's other lists."""
    import png_photo_saver_case as S
    rec = _Recorder(_lib.get_executor())
    _lib.set_executor_for_testing(rec)
    S.run(str(tmp_path / 'a'), 'cpu', egress='device', alpha_matte=True, soft_masks=True)
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 512), (36, 8), (36, 8), (36, 8)] * 3
    rec.ops.clear()
    S.run(str(tmp_path / 'c'), 'cpu', egress='device', cutout=True)
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 16384)] * 3
    rec.ops.clear()
    s = S.saver(str(tmp_path / 'e'), 'cpu', egress='device', dilate_mask=2.0)
    for t, fr in enumerate(S.frames()):
        s.process(S.planes(t), f'{t:05d}.jpg', resize_needed=True, shape=(S.H, S.W), image_u8=torch.from_numpy(fr))
    assert s._pools['redact'].alive == 0 and s.redact is None and not any(k.startswith('redact') for k in s._scratch._slots)
    s.end()
    assert rec.ops == [(36, 4 | 8), (36, 4096), (36, 8)] * 3 and all(f != 65536 for _, f in rec.ops)
    assert executor.redact_calls == []
    rec.ops.clear()
    S.run(str(tmp_path / 'd'), 'cpu', egress='device', alpha_matte=True, redact=dict(mode='blur', strength=2))
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 8), (36, 4096), (36, 65536), (36, 128)] * 3


def test_bad_saver_arguments(tmp_path, executor):
    import png_photo_saver_case as S
    from cutie_amd.inference.object_manager import ObjectManager
    for bad, match in (('blur', 'dict'), (dict(strength=3), 'mode is one of'), (dict(mode='sharpen'), 'mode is one of'),
                       (dict(mode='blur', radius=3), 'unknown keys'), (dict(mode='blur', strength=0), 'blur radius 0'),
                       (dict(mode='blur', strength=65), 'blur radius 65'), (dict(mode='blur', strength=2.5), 'strength is an integer'),
                       (dict(mode='pixelate', strength=1), 'pixelate cell 1'), (dict(mode='pixelate', strength=257), 'pixelate cell 257'),
                       (dict(mode='fill', color=(1, 2)), 'three bytes'), (dict(mode='fill', color=(0, 0, 300)), 'three bytes'),
                       (dict(mode='fill', color='red'), 'three bytes'), (dict(mode='blur', grow=-1), '0 .. 255'), (dict(mode='blur', grow=256), '0 .. 255'),
                       (dict(mode='blur', grow=float('nan')), '0 .. 255'), (dict(mode='blur', edge='soft'), 'edge is one of'),
                       (dict(mode='blur', edge='matte', grow=2), 'must be 0'), (dict(mode='blur', targets=3), 'targets')):
        with pytest.raises(ValueError, match='redact.*' + match):
            S.saver(str(tmp_path), 'cpu', redact=bad)
    om = ObjectManager()
    om.add_new_objects([1])
    with pytest.raises(ValueError, match='redact.*use_long_id'):
        RU.ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, redact=dict(mode='fill'), processor=object())
    with pytest.raises(ValueError, match='redact needs the processor'):
        RU.ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, redact=dict(mode='fill'))
    s = S.saver(str(tmp_path), 'cpu', redact=dict(mode='fill', edge='matte'))
    try:
        with pytest.raises(ValueError, match='process_merged.*redact'):
            s.process_merged([S.planes(0)], '00000.jpg', (S.H, S.W))
        with pytest.raises(ValueError, match='path_to_image or image_u8'):          # the stage reads the frame
            s.process(S.planes(0), '00000.jpg', resize_needed=True, shape=(S.H, S.W))
    finally:
        s.end()


def test_the_merged_plane_is_redacted_under_its_mask(tmp_path, executor):
    import png_photo_saver_case as S
    s = S.saver(str(tmp_path / 'm'), 'cpu', egress='device', redact=dict(mode='fill', color=(0, 255, 0)))
    fr = S.frames()[0]
    s.process_merged([S.planes(0), S.planes(0)], '00000.jpg', (S.H, S.W), image_u8=torch.from_numpy(fr))
    s.end()
    ids = np.array(Image.open(tmp_path / 'm' / 'vid' / '00000.png'))
    assert np.array_equal(executor.redact_log[0][1] != 0, ids != 0)
    assert open(tmp_path / 'm' / 'vid' / 'redacted' / '00000.jpg', 'rb').read() == _jpeg_file(R.model(fr, executor.redact_log[0][1], 'fill', color=(0, 255, 0)))


# ---- parser -----------------------------------------------------------------------------------------------------------------------------------
def test_process_video_parser(capsys):
    from cutie_amd.process_video import arg_parser, redact_args
    base = ['-v', 'v', '-m', 'm', '-o', 'o']
    ap = arg_parser()
    a = ap.parse_args(base)
    assert a.redact is None and redact_args(ap, a) is None
    assert redact_args(ap, ap.parse_args(base + ['--redact', 'blur'])) == \
        dict(mode='blur', strength=12, color=(0, 0, 0), grow=0.0, edge='mask', background=False, targets=None)
    assert redact_args(ap, ap.parse_args(base + ['--redact', 'pixelate']))['strength'] == 16
    got = redact_args(ap, ap.parse_args(base + ['--redact', 'pixelate', '--redact-strength', '256', '--redact-grow', '2.5', '--redact-background',
                                                '--target-objects', '2', '1']))
    assert got == dict(mode='pixelate', strength=256, color=(0, 0, 0), grow=2.5, edge='mask', background=True, targets=[2, 1])
    got = redact_args(ap, ap.parse_args(base + ['--redact', 'fill', '--redact-color', '255', '0', '7', '--redact-edge', 'matte']))
    assert got == dict(mode='fill', strength=0, color=(255, 0, 7), grow=0.0, edge='matte', background=False, targets=None)
    assert redact_args(ap, ap.parse_args(base + ['--redact', 'blur', '--redact-strength', '64']))['strength'] == 64
    RU.redact_config(got)                                                          # what the parser builds is what the saver takes
    for bad in (['--redact', 'sharpen'], ['--redact'], ['--redact-strength', '3'], ['--redact-grow', '1'], ['--redact-background'],
                ['--redact-color', '1', '2', '3'], ['--redact-edge', 'matte'],
                ['--redact', 'blur', '--redact-strength', '0'], ['--redact', 'blur', '--redact-strength', '65'],
                ['--redact', 'blur', '--redact-strength', '2.5'], ['--redact', 'pixelate', '--redact-strength', '1'],
                ['--redact', 'pixelate', '--redact-strength', '257'], ['--redact', 'fill', '--redact-strength', '3'],
                ['--redact', 'blur', '--redact-color', '1', '2', '3'], ['--redact', 'fill', '--redact-color', '1', '2'],
                ['--redact', 'fill', '--redact-color', '1', '2', '256'], ['--redact', 'blur', '--redact-grow', '-1'],
                ['--redact', 'blur', '--redact-grow', '256'], ['--redact', 'blur', '--redact-edge', 'soft'],
                ['--redact', 'blur', '--redact-edge', 'matte', '--redact-grow', '2']):
        with pytest.raises(SystemExit):
            redact_args(ap, ap.parse_args(base + bad))
    from cutie_amd.eval_vos import arg_parser as eval_parser
    with pytest.raises(SystemExit):                                                # eval_vos is out of scope
        eval_parser().parse_args(['--redact', 'blur'])
    capsys.readouterr()
