"""The colour guided filter (PROB_TO_ID flags == 32768) without a GPU: the numpy model of the contract (tests/guided_ref.py) against the
textbook filter in float64, its exact properties, OpList.guided_filter and the descriptor through tests/mock_exec_guided.py, ResultSaver
(matte_refine=...) over the frames of tests/png_photo_saver_case.py, and the parser of process_video.  The stage adds no host-side C++
(csrc/guided.hip holds kernels and their launcher only), so there is nothing for a sanitizer build to run."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.inference.utils import results_utils as RU

import guided_cases as GC
import guided_ref as G
import matte_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53                       # unit roundoff of binary64


def bound(eps):
    """How far the contract's q may lie from 255 times the textbook filter's, in grey levels.

    Fixed point: A_c = rint(a_c 2^20) is off by at most 2^-21 in a_c, which a guide value of at most 255 multiplies, three channels; B =
    rint(b 2^12) is off by at most 2^-13.  Window means of such errors are no larger: 3 * 255 * 2^-21 + 2^-13 = 4.9e-4.
    The solve: on the [0, 1] scale the covariance of a window has eigenvalues in [0, 0.75] (a channel's variance is at most 1/4, the
    trace at most 3/4), so M = Sigma + eps Id has condition number kappa <= (0.75 + eps) / eps.  The adjugate / determinant solve is
    a few dozen float64 operations on exact integers; its forward error is bounded by c kappa u |a| with a constant c for which 64 is
    generous (Higham, Accuracy and Stability, section 9: c ~ 3 n^2 for n = 3 and the operation count of Cramer's rule).  |a| <= sigma_p /
    (2 sqrt(eps)) <= 1 / (4 sqrt(eps)) (the plane's deviation is at most 1/2).  An error da in a moves a I by at most 3 * 255 |da| grey
    levels and b = mean(p) - a . mean(I) by as much again: 6 * 255 * 64 * kappa * u / (4 sqrt(eps)).  The textbook side has an error of
    its own of the same order -- its covariances come from E[Ip] - E[I]E[p] in floating point, an absolute error of order u on entries
    that eps regularises: relative u / eps ~ kappa u --, hence the factor 2."""
    kappa = (0.75 + eps) / eps
    return 3 * 255 * 2.0 ** -21 + 2.0 ** -13 + 2 * (6 * 255 * 64 * kappa * U / (4 * np.sqrt(eps)))


def test_the_bound_is_what_the_derivation_says():
    assert abs((3 * 255 * 2.0 ** -21 + 2.0 ** -13) - 4.9e-4) < 2e-5
    assert bound(1e-6) < 6e-3 and bound(1e-2) < 6e-4          # far below half a grey level: the bytes can differ only next to a half


CASES = [(kind, H, W, r, eps) for kind in GC.CONTENTS for (H, W, r, eps) in ((23, 31, 2, 1e-6), (40, 37, 7, 1e-4), (33, 70, 64, 1e-2))] + \
        [('noise', 50, 45, 16, 1.0), ('grey_guide', 64, 64, 1, 1e-6), ('edge', 48, 96, 8, 1e-6), ('noise', 140, 150, 64, 1e-6)]


@pytest.mark.parametrize('kind,H,W,r,eps', CASES)
def test_model_against_the_textbook_filter(kind, H, W, r, eps):
    guide, planes = GC.make(kind, H, W, 2)
    out, q = G.model(guide, planes, r, eps, full=True)
    eps32 = float(np.float32(eps))                             # the descriptor carries a float: the textbook filter gets the same number
    ideal = 255.0 * np.stack([G.textbook(guide / 255.0, p / 255.0, r, eps32) for p in planes])
    err = float(np.abs(q - ideal).max())
    print(kind, (H, W), r, eps, 'max |q - 255 q_ideal|', err, 'bound', bound(eps))
    assert err <= bound(eps)
    rounded = np.clip(np.rint(ideal), 0, 255)
    off = out.astype(np.int64) - rounded.astype(np.int64)
    assert np.abs(off).max() <= 1
    frac = np.abs(ideal - np.floor(ideal) - 0.5)               # the distance of the ideal from a half
    assert (frac[off != 0] <= bound(eps)).all()


def test_exact_properties():
    rng = np.random.default_rng(3)
    guide, planes = GC.make('noise', 21, 34, 2, seed=1)
    for c in (0, 1, 77, 254, 255):                             # constant in, the same bytes out
        const = np.full((1, 21, 34), c, np.uint8)
        for eps in (1e-6, 1e-2):
            assert np.array_equal(G.model(guide, const, 5, eps), const)
    g1 = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)       # 1 x 1: the plane
    for v in (0, 9, 255):
        assert G.model(g1, np.full((1, 1, 1), v, np.uint8), 3, 1e-4).tolist() == [[[v]]]
    big = G.model(guide, planes, 34, 1e-4)                     # r >= max(H, W): every window is the frame
    assert np.array_equal(big, G.model(guide, planes, 64, 1e-4)) and np.array_equal(big, G.model(guide, planes, 40, 1e-4))
    A, B = G.coefficients(guide, planes, 34, 1e-4)
    assert all((A[:, c] == A[:, c, :1, :1]).all() for c in range(3)) and (B == B[:, :1, :1]).all()       # one fit for the whole frame
    t = G.model(np.ascontiguousarray(guide.transpose(1, 0, 2)), np.ascontiguousarray(planes.transpose(0, 2, 1)), 4, 1e-4)
    assert np.array_equal(t.transpose(0, 2, 1), G.model(guide, planes, 4, 1e-4))                          # transposing commutes
    # Permuting the guide's channels: the written order sums three products pairwise from the left -- (x0 + x1) + x2 -- and float64
    # addition is not associative, so another channel order may round a_c, det and q differently: equality is NOT implied by the
    # contract.  What holds is the bound against the ideal on both sides, so the two q differ by at most twice the bound.
    for perm in ((1, 0, 2), (2, 1, 0), (1, 2, 0)):
        qa = G.model(guide, planes, 4, 1e-6, full=True)[1]
        qb = G.model(np.ascontiguousarray(guide[..., perm]), planes, 4, 1e-6, full=True)[1]
        assert np.abs(qa - qb).max() <= 2 * bound(1e-6)


def test_the_refined_edge_is_steeper_at_the_guides_edge():
    guide, planes = GC.make('edge', 40, 96, 3)
    out = G.model(guide, planes, 8, 1e-4)
    for s in range(3):
        before, after = GC.edge_slopes(guide, planes[s], out[s])
        print('plane', s, 'rise across the edge: input', before, 'refined', after)
        assert after > 2 * before                              # a ramp of 9 pixels rises 28 levels per pixel; the refined one sits on the step


# ---- descriptor and arguments -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def executor():
    from mock_exec_guided import GuidedMockExecutor
    ex = GuidedMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(M.MatteExecutor(ex))
    yield ex
    _lib.set_executor_for_testing(None)


def test_descriptor_and_argument_checks(executor):
    H, W, S = 9, 13, 3
    guide_np, planes_np = GC.make('noise', H, W, S)
    room = torch.zeros((H, 3 * W + 5), dtype=torch.uint8)
    guide = room[:, :3 * W].view(H, W, 3)
    guide.copy_(torch.from_numpy(guide_np))
    proom = torch.zeros((S, H + 2, W + 3), dtype=torch.uint8)
    planes = proom[:, :H, :W]
    planes.copy_(torch.from_numpy(planes_np))
    out = torch.zeros((S, H, W), dtype=torch.uint8)
    scratch = torch.zeros(O.OpList.guided_scratch_words(S, H, W), dtype=torch.int32)
    ol = O.OpList()
    ol.guided_filter(guide, planes, out, scratch, radius=3, eps=1e-4)
    ol.run()
    assert executor.guided_calls == [(H, W, S, 3, float(np.float32(1e-4)))]
    assert np.array_equal(out.numpy(), G.model(guide_np, planes_np, 3, 1e-4))
    last = planes[2].clone()
    out2 = torch.zeros((S, H, W), dtype=torch.uint8)
    ol = O.OpList()
    ol.guided_filter(guide, planes[:2], out2, scratch, radius=3, eps=1e-4, last=last)          # the last plane in a tensor of its own
    ol.guided_filter(guide, None, out[:1], scratch, radius=64, eps=1.0, last=last)
    ol.guided_filter(guide, planes[:1], out[1:2], scratch, radius=1, eps=1e-6)                  # the limits are inside
    ol.run()
    assert torch.equal(out2[:2], torch.from_numpy(G.model(guide_np, planes_np, 3, 1e-4))[:2]) and executor.guided_calls[1][2] == 3
    assert torch.equal(out2[2], torch.from_numpy(G.model(guide_np, planes_np, 3, 1e-4))[2])
    assert O.OpList.guided_scratch_words(2, 5, 7) == 4 * 2 * 5 * 7
    assert (O.OpList.GUIDED_MAX_RADIUS, O.OpList.GUIDED_MAX_PLANES) == (G.MAX_RADIUS, G.MAX_PLANES) == (64, 16)
    assert O.OpList.GUIDED_TILE_X + 2 * O.OpList.GUIDED_MAX_RADIUS == O.OpList.GUIDED_THREADS
    good = dict(guide=guide, planes=planes, out=out, scratch=scratch, radius=3, eps=1e-4)
    for bad in (dict(guide=guide.float()), dict(guide=torch.zeros((H, W, 4), dtype=torch.uint8)), dict(guide=torch.zeros((H, W), dtype=torch.uint8)),
                dict(ldrow=3 * W - 1), dict(planes=planes.int()), dict(planes=planes[:, :, :W - 1]), dict(planes=proom[:, :H, ::2][:, :, :W]),
                dict(planes=None), dict(planes=torch.zeros((17, H, W), dtype=torch.uint8), out=torch.zeros((17, H, W), dtype=torch.uint8)),
                dict(planes=torch.zeros((16, H, W), dtype=torch.uint8), last=last), dict(last=last[:, :4]), dict(last=last.int()),
                dict(radius=0), dict(radius=65), dict(eps=5e-7), dict(eps=1.01), dict(eps=float('nan')),
                dict(out=out[:2]), dict(out=out.int()), dict(out=torch.zeros((S, H, W + 1), dtype=torch.uint8)[:, :, :W]),
                dict(scratch=scratch[:-1]), dict(scratch=scratch.float()),
                dict(out=proom.view(-1)[:S * H * W].view(S, H, W)), dict(out=room.view(-1)[:S * H * W].view(S, H, W))):       # in place: refused
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match='guided_filter'):
            O.OpList().guided_filter(kw.pop('guide'), kw.pop('planes'), kw.pop('out'), kw.pop('scratch'), **kw)
    ol = O.OpList()                                                                             # 32768 is a stage on its own
    ol.add(O.PROB_TO_ID, 32768 | 8, [0, H, W, 3, 3 * W, W, H * W, 0, scratch.numel(), S, 0], [1e-4], [None, None, guide, out, None, scratch, planes])
    with pytest.raises(Exception):
        ol.run()
    src = open(os.path.join(HERE, '..', 'include', 'cutie_hip.h')).read()
    assert 'flags == 32768' in src and 'bit 9 (value 512)' in src and 'CUTIE_GUIDED_MAX_RADIUS 64' in src and 'CUTIE_GUIDED_MAX_PLANES 16' in src
    kern = open(os.path.join(HERE, '..', 'cutie_amd', 'csrc', 'guided.hip')).read()
    assert f'#define GF_T {O.OpList.GUIDED_THREADS} ' in kern and f'#define GF_TY {O.OpList.GUIDED_TILE_Y} ' in kern and '#define GF_RMAX 64 ' in kern
    assert 'int launch_guided_filter' in kern and 'guided.hip' in open(os.path.join(HERE, '..', 'cutie_amd', 'csrc', 'Makefile')).read()
    assert '32768' in open(os.path.join(HERE, '..', 'INTEGRATION.md')).read()


def test_a_stale_library_is_named(monkeypatch):
    monkeypatch.setattr(_lib, '_executor', None)
    monkeypatch.setattr(_lib, 'has_guided_filter', lambda: False)
    with pytest.raises(_lib.HipLibraryError, match='32768'):
        O.OpList().guided_filter(torch.zeros((2, 2, 3), dtype=torch.uint8), None, None, None, radius=1, eps=1e-4)


# ---- saver and parser -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('egress', ['host', 'device'])
@pytest.mark.parametrize('png_codes', ['fixed', 'dynamic'])
def test_saver_refines_what_it_writes(tmp_path, executor, egress, png_codes):
    import png_photo_saver_case as S
    kw = dict(egress=egress, cutout=True, alpha_matte=True, soft_masks=True, png_codes=png_codes, target_objects=[3])
    plain = S.run(str(tmp_path / 'plain'), 'cpu', **kw)
    assert executor.guided_calls == []
    fine = S.run(str(tmp_path / 'fine'), 'cpu', matte_refine=(4, 1e-4), **kw)
    assert sorted(plain) == sorted(fine) and len(fine) == 3 * (1 + 1 + 2 + 1)
    assert executor.guided_calls == [(S.H, S.W, 3, 4, float(np.float32(1e-4)))] * 3            # two soft masks and the matte: one launch per frame
    changed = 0
    for t, fr in enumerate(S.frames()):
        for name in (f'vid/alpha/{t:05d}.png', f'vid/soft_masks/5/{t:05d}.png', f'vid/soft_masks/3/{t:05d}.png'):
            a, b = np.array(Image.open(plain[name])), np.array(Image.open(fine[name]))
            assert np.array_equal(b, G.model(fr, a[None], 4, 1e-4)[0]), name
            changed += int(not np.array_equal(a, b))
        cut = np.array(Image.open(fine[f'vid/cutout/{t:05d}.png']))
        assert cut.shape == (S.H, S.W, 4) and np.array_equal(cut[..., :3], fr)
        assert np.array_equal(cut[..., 3], np.array(Image.open(fine[f'vid/alpha/{t:05d}.png'])))
        assert open(plain[f'vid/{t:05d}.png'], 'rb').read() == open(fine[f'vid/{t:05d}.png'], 'rb').read()     # the id masks keep their bytes
    assert changed == 9


def test_a_cutout_alone_and_soft_masks_alone(tmp_path, executor):
    import png_photo_saver_case as S
    plain = S.run(str(tmp_path / 'a'), 'cpu', alpha_matte=True, target_objects=[3])
    cut = S.run(str(tmp_path / 'b'), 'cpu', cutout=True, matte_refine=(4, 1e-4), target_objects=[3])
    assert [c[2] for c in executor.guided_calls] == [1] * 3
    for t, fr in enumerate(S.frames()):
        rgba = np.array(Image.open(cut[f'vid/cutout/{t:05d}.png']))
        assert np.array_equal(rgba[..., 3], G.model(fr, np.array(Image.open(plain[f'vid/alpha/{t:05d}.png']))[None], 4, 1e-4)[0])
    executor.guided_calls.clear()
    S.run(str(tmp_path / 'c'), 'cpu', soft_masks=True, matte_refine=(2, 1e-2))
    assert [c[2:4] for c in executor.guided_calls] == [(2, 2)] * 3


def test_a_cutout_beyond_the_row_limit_takes_the_refined_plane(tmp_path, executor, monkeypatch):
    import png_photo_saver_case as S
    monkeypatch.setattr(O.OpList, 'PNG_PHOTO_ROW_LIMIT', 4 * S.W)                # RGBA rows no longer fit: the cut-out goes through PIL
    files = S.run(str(tmp_path / 'wide'), 'cpu', cutout=True, alpha_matte=True, matte_refine=(4, 1e-4))
    plain = S.run(str(tmp_path / 'plain'), 'cpu', alpha_matte=True)
    for t, fr in enumerate(S.frames()):
        cut = np.array(Image.open(files[f'vid/cutout/{t:05d}.png']))
        want = G.model(fr, np.array(Image.open(plain[f'vid/alpha/{t:05d}.png']))[None], 4, 1e-4)[0]
        assert np.array_equal(cut[..., :3], fr) and np.array_equal(cut[..., 3], want)
        assert np.array_equal(np.array(Image.open(files[f'vid/alpha/{t:05d}.png'])), want)


def test_more_than_sixteen_planes_go_in_groups(executor):
    """K + 1 = 19 planes: a launch of 16 soft masks, then one of 2 soft masks and the matte (the buffers' side of ResultSaver._queue_matte)."""
    from cutie_amd.inference.utils.saver_buffers import MatteBuffers
    H, W, K = 6, 7, 18
    b = MatteBuffers(H, W, K, (), True, torch.device('cpu'), lambda *a: None, refine=True)
    assert tuple(b.refined.shape) == (K + 1, H, W) and b.final_plane(K).data_ptr() == b.refined[K].data_ptr()
    plain = MatteBuffers(H, W, K, (), True, torch.device('cpu'), lambda *a: None)
    assert plain.refined is None and plain.final_plane(K) is plain.matte and plain.final_plane(1).data_ptr() == plain.planes[1].data_ptr()


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
    """The op lists of the default paths, as recorded on the tree before the stage existed (tests/test_png_photo_cpu.py holds the same
    lists): no descriptor more, none less, none changed; with the switch one launch per frame joins behind the planes' launches."""
    import png_photo_saver_case as S
    rec = _Recorder(_lib.get_executor())
    _lib.set_executor_for_testing(rec)
    S.run(str(tmp_path / 'a'), 'cpu', egress='device', alpha_matte=True, soft_masks=True)
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 512), (36, 8), (36, 8), (36, 8)] * 3
    rec.ops.clear()
    S.run(str(tmp_path / 'b'), 'cpu', egress='device', alpha_matte=True, soft_masks=True, cutout=True, png_codes='dynamic')
    assert rec.ops == ([(36, 4 | 8), (36, 256), (36, 512)] + [(36, 16384)] * 4) * 3
    rec.ops.clear()
    S.run(str(tmp_path / 'c'), 'cpu', egress='device', cutout=True)
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 16384)] * 3
    rec.ops.clear()
    S.run(str(tmp_path / 'd'), 'cpu', egress='device', alpha_matte=True, soft_masks=True, matte_refine=(4, 1e-4))
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 512), (36, 32768), (36, 8), (36, 8), (36, 8)] * 3


def test_bad_arguments_are_refused(tmp_path, executor):
    import png_photo_saver_case as S
    from cutie_amd.inference.object_manager import ObjectManager
    for bad, match in (((0, 1e-4), 'radius 0'), ((65, 1e-4), 'radius 65'), ((4, 1e-7), 'eps'), ((4, 2.0), 'eps'), ((4, float('nan')), 'eps'),
                       (4, 'matte_refine'), ((4,), 'matte_refine'), ((2.5, 1e-4), 'matte_refine'), (('a', 'b'), 'matte_refine')):
        with pytest.raises(ValueError, match=match):
            S.saver(str(tmp_path), 'cpu', alpha_matte=True, matte_refine=bad)
    with pytest.raises(ValueError, match='none of them is set'):
        S.saver(str(tmp_path), 'cpu', matte_refine=(4, 1e-4))
    with pytest.raises(ValueError, match='none of them is set'):
        S.saver(str(tmp_path), 'cpu', matte_refine=(4, 1e-4), vis_modes=('popup',))       # the JPEGs are not refined
    om = ObjectManager()
    om.add_new_objects([1])
    with pytest.raises(ValueError, match='matte_refine.*use_long_id'):
        RU.ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, alpha_matte=True, matte_refine=(4, 1e-4), processor=object())
    with pytest.raises(ValueError, match='matte_refine needs the processor'):
        RU.ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, alpha_matte=True, matte_refine=(4, 1e-4))
    s = S.saver(str(tmp_path), 'cpu', alpha_matte=True, matte_refine=(4, 1e-4))
    try:
        assert s.matte_refine == (4, 1e-4)
        with pytest.raises(ValueError, match='process_merged'):
            s.process_merged([S.planes(0)], '00000.jpg', (S.H, S.W))
        with pytest.raises(ValueError, match='path_to_image or image_u8'):                  # the guide is the frame
            s.process(S.planes(0), '00000.jpg', resize_needed=True, shape=(S.H, S.W))
    finally:
        s.end()
    s = S.saver(str(tmp_path), 'cpu')
    try:
        assert s.matte_refine is None
    finally:
        s.end()


def test_process_video_parser(capsys):
    from cutie_amd.process_video import arg_parser, refine_args
    base = ['-v', 'v', '-m', 'm', '-o', 'o']
    ap = arg_parser()
    a = ap.parse_args(base)
    assert a.refine_matte is None and a.refine_eps is None and refine_args(ap, a) is None
    a = ap.parse_args(base + ['--alpha', '--refine-matte', '16'])
    assert refine_args(ap, a) == (16, 1e-4)
    a = ap.parse_args(base + ['--soft-masks', '--refine-matte', '64', '--refine-eps', '1e-6'])
    assert refine_args(ap, a) == (64, 1e-6)
    a = ap.parse_args(base + ['--cutout', '--refine-matte', '1', '--refine-eps', '1'])
    assert refine_args(ap, a) == (1, 1.0)
    for bad in (['--alpha', '--refine-eps', '1e-3'], ['--alpha', '--refine-matte', '0'], ['--alpha', '--refine-matte', '65'],
                ['--alpha', '--refine-matte', '4', '--refine-eps', '1e-7'], ['--alpha', '--refine-matte', '4', '--refine-eps', '1.5'],
                ['--refine-matte', '4'], ['--vis', 'popup', '--refine-matte', '4'], ['--alpha', '--refine-matte', '2.5'], ['--alpha', '--refine-matte']):
        with pytest.raises(SystemExit):
            refine_args(ap, ap.parse_args(base + bad))
    from cutie_amd.eval_vos import arg_parser as eval_parser
    with pytest.raises(SystemExit):                                                          # eval_vos has none of the matte outputs
        eval_parser().parse_args(['--refine-matte', '4'])
    capsys.readouterr()
