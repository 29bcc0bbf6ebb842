"""Multi-scale merge on the MI355X (PROB_TO_ID flags&16, ABI 8): the fused kernel against the library's own chain per member (RESIZE ->
(x * 255).to(uint8) -> int32 sum -> first maximum -> lut; equal ids) and against the numpy model (tests/merge_ref.py), the integer-sum
properties, the PNG stage behind it, every argument check of the launcher, and the driver end to end on the bike example: host against
device egress, against three independent single-size runs (exact) and against the file route (score dumps + merge_multi_scale)."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config

import merge_ref as M
import png_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _lut(P, dtype):
    hi = 250 if dtype == torch.uint8 else 70000
    return torch.tensor([0] + [hi - 3 * k for k in range(1, P)], dtype=torch.int32, device='cuda')


def _first_max(total):
    """Index of the first largest value along dim 0, plane by plane (no reliance on how a library breaks ties)."""
    best, arg = total[0].clone(), torch.zeros_like(total[0], dtype=torch.long)
    for q in range(1, total.shape[0]):
        m = total[q] > best
        arg[m] = q
        best = torch.where(m, total[q], best)
    return arg


def _chain(probs, lut, OH, OW, dtype):
    total = torch.zeros((probs[0].shape[0], OH, OW), dtype=torch.int32, device='cuda')
    for p in probs:
        P, h, w = p.shape
        full = torch.empty((P, OH, OW), dtype=torch.float32, device='cuda')
        ol = O.OpList()
        ol.resize(p, full, C=P, H=h, W=w, OH=OH, OW=OW, plane=p.stride(0), ldrow=p.stride(1))
        ol.run()
        total += (full * 255).to(torch.uint8).to(torch.int32)
    return lut.long()[_first_max(total)].to(dtype)


def _fused(probs, lut, OH, OW, dtype, off=0):
    buf = torch.full((OH * OW + 2 * GUARD + 4,), 77, dtype=dtype, device='cuda')
    out = buf[GUARD + off:GUARD + off + OH * OW].view(OH, OW)
    ol = O.OpList()
    ol.prob_to_id_merged(probs, lut, out, out_hw=(OH, OW))
    ol.run()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD + off] == 77).all()) and bool((buf[GUARD + off + OH * OW:] == 77).all())
    return out


def _probs(P, h, w, seed, smooth=True):
    return M.smooth_probs(P, h, w, seed, smooth).cuda()


def _check(probs, OH, OW, dtype, off=0):
    lut = _lut(probs[0].shape[0], dtype)
    got = _fused(probs, lut, OH, OW, dtype, off)
    assert torch.equal(got, _chain(probs, lut, OH, OW, dtype))
    want = M.merge([p.cpu().numpy() for p in probs], lut.cpu().numpy(), OH, OW)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    return got


# ---- fused equals the chain, bit for bit -------------------------------------------------------------------------------------------------
CASES = [([(37, 53)], (101, 149)),
         ([(37, 53), (30, 40)], (101, 149)),
         ([(37, 53), (30, 40), (97, 131)], (101, 149)),
         ([(101, 149), (37, 53), (150, 220)], (101, 149)),        # identity, up and down in one op
         ([(33, 47), (33, 90)], (33, 90)),
         ([(5, 7), (1, 1)], (9, 13)),
         ([(30, 40), (35, 47), (40, 53), (45, 60), (50, 67), (55, 73), (60, 80), (61, 83)], (61, 83)),
         ([(60, 107), (75, 133), (90, 160)], (120, 216))]        # OW % 4 == 0: packed stores


@pytest.mark.parametrize('srcs,dst', CASES, ids=[f'S{len(s)}to{d[0]}x{d[1]}' for s, d in CASES])
@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32], ids=['u8', 'i32'])
def test_fused_equals_the_chain_and_the_model(srcs, dst, dtype):
    probs = [_probs(4, h, w, seed=3 * k + dst[1]) for k, (h, w) in enumerate(srcs)]
    _check(probs, *dst, dtype)


@pytest.mark.parametrize('P', range(1, 9))
def test_plane_counts(P):
    probs = [_probs(P, 60, 90, seed=P, smooth=False), _probs(P, 41, 57, seed=P + 20)]
    for dtype in (torch.uint8, torch.int32):
        _check(probs, 77, 113, dtype)


def test_strided_views_of_a_padded_tensor_are_read_in_place():
    g = torch.Generator().manual_seed(5)
    big = [torch.softmax(torch.randn(3, 96, 144, generator=g), 0).cuda(), torch.softmax(torch.randn(3, 64, 80, generator=g), 0).cuda()]
    views = [big[0][:, 3:3 + 85, 7:7 + 131], big[1][:, 8:8 + 50, 2:2 + 71]]      # what `step` returns: rows and planes of the padded tensor
    assert not any(v.is_contiguous() for v in views)
    lut = _lut(3, torch.uint8)
    got = _check(views, 170, 262, torch.uint8)
    assert torch.equal(got, _fused([v.contiguous() for v in views], lut, 170, 262, torch.uint8))


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32], ids=['u8', 'i32'])
def test_misaligned_output_is_written_element_by_element(dtype):
    """OW % 4 == 0 but the output starts 1 / 2 / 3 elements behind an aligned address: the same ids, nothing outside."""
    probs = [_probs(4, 60, 90, seed=21), _probs(4, 96, 144, seed=22)]
    want = _check(probs, 96, 144, dtype)
    for off in (1, 2, 3):
        assert torch.equal(_fused(probs, _lut(4, dtype), 96, 144, dtype, off=off), want)


# ---- the sum is an integer sum of quantised scores ---------------------------------------------------------------------------------------
def _const(levels, h, w):
    """Planes that are constant at (level + 0.5) / 255: a bilinear sample stays within a few ulps, so it quantises to `level`."""
    return torch.tensor([(v + 0.5) / 255 for v in levels], dtype=torch.float32).view(-1, 1, 1).expand(-1, h, w).contiguous().cuda()


GEO = [(24, 36), (31, 47), (50, 70)]


def test_quantisation_comes_before_the_sum():
    """0.5001 and 0.5019 both quantise to 127 in every member: the sums tie and the FIRST plane wins -- a float sum picks the second."""
    probs = [torch.tensor([0.5001, 0.5019]).view(2, 1, 1).expand(-1, h, w).contiguous().cuda() for h, w in GEO]
    lut = torch.tensor([11, 22], dtype=torch.int32, device='cuda')
    got = _fused(probs, lut, 41, 59, torch.uint8)
    assert bool((got == 11).all())
    assert torch.equal(got, _chain(probs, lut, 41, 59, torch.uint8))


def test_members_weigh_in_quantised_steps():
    """Member A prefers plane 1 by 50 quantised steps, member B plane 2 by the same 50: the sums tie at 187 and plane 1 (the first) wins;
    one step more for B and plane 2 wins."""
    lut = torch.tensor([5, 6, 7], dtype=torch.int32, device='cuda')
    a = _const([10, 127, 77], 24, 36)
    for b2, want in ((110, 6), (111, 7)):
        b = _const([10, 60, b2], 31, 47)
        got = _fused([a, b], lut, 41, 59, torch.uint8)
        assert bool((got == want).all())
        assert torch.equal(got, _chain([a, b], lut, 41, 59, torch.uint8))


def test_one_quantises_to_255():
    """1.0 -> 255 (an identity member samples it exactly): plane 1 = 255 + 100 beats plane 0 = 254 + 100 + ... only then."""
    a = torch.stack([torch.full((41, 59), 254.5 / 255), torch.ones(41, 59)]).cuda()
    b = _const([100, 100], 24, 36)
    lut = torch.tensor([3, 9], dtype=torch.int32, device='cuda')
    got = _fused([a, b], lut, 41, 59, torch.uint8)
    assert bool((got == 9).all())
    assert torch.equal(got, _chain([a, b], lut, 41, 59, torch.uint8))


def test_all_equal_inputs_give_plane_zero():
    probs = [torch.full((4, h, w), 0.25, device='cuda') for h, w in GEO]
    lut = torch.tensor([17, 1, 2, 3], dtype=torch.int32, device='cuda')
    for dtype in (torch.uint8, torch.int32):
        assert bool((_fused(probs, lut, 41, 59, dtype) == 17).all())


def test_the_order_of_the_members_changes_nothing():
    probs = [_probs(5, h, w, seed=40 + k) for k, (h, w) in enumerate(GEO)]
    lut = _lut(5, torch.uint8)
    want = _fused(probs, lut, 67, 101, torch.uint8)
    for perm in ((1, 2, 0), (2, 1, 0), (0, 2, 1)):
        assert torch.equal(_fused([probs[k] for k in perm], lut, 67, 101, torch.uint8), want)


# ---- with the PNG stage ------------------------------------------------------------------------------------------------------------------
def _with_png(probs, lut, H, W, cap=None):
    cap = O.OpList.png_capacity(H, W) if cap is None else cap
    ids = torch.full((H, W), 77, dtype=torch.uint8, device='cuda')
    buf = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    stream = buf[GUARD:GUARD + cap]
    status = torch.full((4,), -1, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device='cuda')
    ol = O.OpList()
    ol.prob_to_id_merged(probs, lut, ids, out_hw=(H, W), png=(stream, status, scratch))
    ol.run()
    torch.cuda.synchronize()
    return ids, buf.cpu().numpy(), stream.cpu().numpy(), status.cpu().numpy()


def test_merge_and_deflate_in_one_op():
    probs = [_probs(4, 60, 107, seed=11), _probs(4, 75, 133, seed=12), _probs(4, 90, 160, seed=13)]
    lut = _lut(4, torch.uint8)
    for H, W in ((120, 214), (135, 240)):
        ids, buf, stream, status = _with_png(probs, lut, H, W)
        assert torch.equal(ids, _chain(probs, lut, H, W, torch.uint8))
        want, adler = R.encode(ids.cpu().numpy())
        assert int(status[2]) == 0 and int(status[0]) == len(want) and (int(status[1]) & 0xffffffff) == adler
        assert stream[:len(want)].tobytes() == want
        assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
    need = len(want)
    for cap in ((need - 1) // 4 * 4, 64):                       # the overflow bit as before: nothing written, [0] says what it needs
        ids2, buf, stream, status = _with_png(probs, lut, H, W, cap=cap)
        assert int(status[2]) & 1 and int(status[0]) == need and torch.equal(ids2, ids)
        assert (buf == 0xA5).all()


# ---- argument checks of the launcher (nothing is launched) -----------------------------------------------------------------------------
def test_error_cases_return_minus_two_and_leave_the_output_alone():
    probs = [_probs(3, 20, 30, seed=1), _probs(3, 25, 37, seed=2)]
    ptrs, geom = O.OpList.merge_tables(probs)
    lut = _lut(3, torch.uint8)
    OH, OW = 40, 60
    out = torch.full((OH * OW * 8,), 77, dtype=torch.uint8, device='cuda')          # (room for any output type)
    stream = torch.full((O.OpList.png_capacity(OH, OW),), 0xA5, dtype=torch.uint8, device='cuda')
    status = torch.full((4,), -1, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.png_scratch_words(OH, OW), dtype=torch.int32, device='cuda')
    good = dict(flags=4 | 16, P=3, S=2, OH=OH, OW=OW, p0=ptrs, p6=geom)
    cases = [(dict(flags=16), 'flags&4 must accompany'),
             (dict(flags=2 | 4 | 16), 'uint8 or int32'),
             (dict(S=0), '1 <= S <= 8'), (dict(S=9), '1 <= S <= 8'), (dict(S=-1), '1 <= S <= 8'),
             (dict(p0=None), 'source table'), (dict(p6=None), 'source table'),
             (dict(flags=4 | 8 | 16, p0=None), 'source table'),                  # (not the PNG stage on its own)
             (dict(flags=4 | 16 | 32), 'unknown flags'), (dict(flags=4 | 16 | 64), 'unknown flags'),
             (dict(flags=1 | 4 | 8 | 16), 'uint8 ids'),
             (dict(P=0), 'P >= 1'), (dict(OH=0), 'empty shape'), (dict(OW=0), 'empty shape')]
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [a['P'], 0, 0, 0, 0, a['OH'], a['OW'], stream.numel(), scratch.numel(), a['S']], [],
               [a['p0'], lut, out, stream, status, scratch, a['p6']])
        arr = ol.finalize()
        assert _lib.load().cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in _lib.load().cutie_hip_last_error().decode(), (change, _lib.load().cutie_hip_last_error().decode())
        with pytest.raises(RuntimeError, match='cutie_exec failed'):
            ol.run()
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((stream == 0xA5).all()) and bool((status == -1).all())
    ol = O.OpList()                                             # and the untouched descriptor runs
    ol.prob_to_id_merged(probs, lut, out[:OH * OW].view(OH, OW), out_hw=(OH, OW))
    ol.run()
    assert torch.equal(out[:OH * OW].view(OH, OW), _chain(probs, lut, OH, OW, torch.uint8)) and bool((out[OH * OW:] == 77).all())


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
SIZES = (240, 320, 400)


def _copy_clip(root, names):
    src = os.path.join(HERE, 'golden', 'bike')
    for name in names:
        img_dir, msk_dir = os.path.join(root, 'JPEGImages', name), os.path.join(root, 'Annotations', name)
        os.makedirs(img_dir)
        os.makedirs(msk_dir)
        for f in sorted(os.listdir(src)):
            shutil.copy(os.path.join(src, f), img_dir if f.endswith('.jpg') else msk_dir)


def _scales(root, sizes=SIZES):
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    return [list(VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False, size=s).get_datasets())
            for s in sizes]


def _images(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith('.png'):
                im = Image.open(os.path.join(dp, f))
                out[os.path.relpath(os.path.join(dp, f), root)] = (im.mode, im.getpalette(), np.array(im))
    return out


def _files(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(root) for f in fs}


def _single_run(net, cfg, rd):
    """One member on its own, driven plainly (no look-ahead, no saver): per frame a copy of what `step` returned, and the id table."""
    from cutie_amd.inference.inference_core import InferenceCore
    core = InferenceCore(net, cfg=cfg)
    n, out = len(rd), []
    for ti in range(n):
        d = rd[ti]
        mask, valid = d.get('mask'), d.get('valid_labels')
        prob = core.step(d['rgb'].cuda(), mask.cuda() if mask is not None else None, valid.tolist() if valid is not None else None, end=(ti == n - 1))
        out.append((d['info']['frame'], d['info']['shape'], prob.clone()))
    return out, {t: o.id for t, o in core.object_manager.tmp_id_to_obj.items()}


def _chain_of_runs(net, cfg, readers):
    runs = [_single_run(net, cfg, rd) for rd in readers]
    assert all(r[1] == runs[0][1] for r in runs)
    P = runs[0][0][0][2].shape[0]
    lut = torch.zeros(P, dtype=torch.int32, device='cuda')
    for t, o in runs[0][1].items():
        lut[t] = o
    want = {}
    for k, (frame, shape, _) in enumerate(runs[0][0]):
        want[frame[:-4] + '.png'] = _chain([r[0][k][2] for r in runs], lut, int(shape[0]), int(shape[1]), torch.uint8).cpu().numpy()
    return want


@pytest.fixture(scope='module')
def net():
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    _lib.set_executor_for_testing(None)
    n = CUTIE(default_config()).cuda().eval()
    n.load_weights(S.decisive_state_dict())
    return n


@pytest.fixture(scope='module')
def bike(net, tmp_path_factory):
    """The multi-scale runs of the bike example, made once: host and device egress, and the chain over three independent runs."""
    from cutie_amd.eval_vos import process_video_multiscale
    root = str(tmp_path_factory.mktemp('ms'))
    _copy_clip(root, ['bike'])
    cfg = default_config()
    with torch.inference_mode():
        stats = {}
        for eg in ('host', 'device'):
            readers = [sc[0] for sc in _scales(root)]
            stats[eg] = process_video_multiscale(net, cfg, readers, os.path.join(root, eg), dataset='d17-val', egress=eg)
        want = _chain_of_runs(net, cfg, [sc[0] for sc in _scales(root)])
    torch.cuda.synchronize()
    return dict(root=root, stats=stats, want=want, host=_images(os.path.join(root, 'host')), device=_images(os.path.join(root, 'device')))


def test_host_and_device_egress_write_equal_images(bike):
    host, dev = bike['host'], bike['device']
    assert sorted(host) == sorted(dev) == [f'bike/0000{k}.png' for k in range(4)]
    for k in host:
        assert host[k][0] == dev[k][0] == 'P' and host[k][1] == dev[k][1] and np.array_equal(host[k][2], dev[k][2]), k
        assert host[k][2].shape == (480, 854)
    for eg in ('host', 'device'):
        assert bike['stats'][eg]['frames'] == 4 and bike['stats'][eg]['seconds'] > 0
    for eg in ('host', 'device'):                               # masks only: no score dump anywhere below the runs
        assert not any('Scores' in d or f.endswith('.npz') for d, _, fs in os.walk(os.path.join(bike['root'], eg)) for f in fs + ['']), eg


def test_pixels_equal_the_chain_over_three_independent_runs(bike):
    """A clip's probabilities do not depend on how it is driven: the masks of the one-pass run equal, exactly, the chain applied to the
    probabilities of three single-size runs made one after another (ordering and buffer-lifetime mistakes of the driver show here)."""
    want = bike['want']
    assert len(want) == 4
    for f, ids in want.items():
        assert np.array_equal(bike['host']['bike/' + f][2], ids), f
        print(f'{f}: object pixels {int((ids != 0).sum())} of {ids.size}, ids {np.unique(ids).tolist()}')
    assert len(np.unique(want['00000.png'])) >= 2


def test_against_the_file_route(bike, net):
    """Three process_video(save_scores=True) runs + merge_multi_scale.merge.  That route resamples with torch's F.interpolate; every
    member can move a plane's quantised score by at most 1, so pixels may differ only where the file route's two largest sums lie within
    2 S, and on at most 0.5 % of the pixels of a frame (a condition, not a measurement).
    Measured on the MI355X (sizes 240 / 320 / 400): 0 differing pixels on every frame; 0.03-0.05 % of the file route's pixels lie within
    the gap (frame 00002 is all background at these sizes: 0 %); the counts are printed."""
    from cutie_amd.eval_vos import process_video
    from cutie_amd.merge_multi_scale import merge
    root = bike['root']
    runs = []
    with torch.inference_mode():
        for s, sc in zip(SIZES, _scales(root)):
            run = os.path.join(root, f'run{s}')
            process_video(net, default_config(save_scores=True), sc[0], os.path.join(run, 'Annotations'), dataset='d17-val', save_scores=True,
                          score_output_root=os.path.join(run, 'Scores'))
            runs.append(run)
    out = os.path.join(root, 'merged')
    assert merge(runs, out, 'D', num_proc=1) == 4
    S = len(SIZES)
    for k in range(4):
        f = f'0000{k}'
        got = bike['host'][f'bike/{f}.png'][2]
        ref = np.array(Image.open(os.path.join(out, 'bike', f + '.png')))
        total = sum(np.load(os.path.join(r, 'Scores', 'bike', f + '.npz'))['prob'].astype(np.int32) for r in runs)
        srt = np.sort(total, axis=0)
        gap = srt[-1] - srt[-2]
        diff = got != ref
        print(f'frame {f}: {int(diff.sum())} of {diff.size} pixels differ from the file route; {float((gap <= 2 * S).mean()):.4%} of its pixels '
              f'lie within the 2 S gap')
        assert float((gap <= 2 * S).mean()) <= 0.005             # (else the cap below says nothing: other sizes would be needed)
        assert bool((gap[diff] <= 2 * S).all())
        assert diff.sum() <= 0.005 * diff.size


def test_flip_aug_members(net, bike):
    """--flip-aug applies to every member (the cores' own flip lanes): again the chain over independent runs, exactly."""
    from cutie_amd.eval_vos import process_video_multiscale
    root = bike['root']
    cfg = default_config(flip_aug=True)
    with torch.inference_mode():
        process_video_multiscale(net, cfg, [sc[0] for sc in _scales(root, (240, 320))], os.path.join(root, 'flip'), egress='device')
        want = _chain_of_runs(net, cfg, [sc[0] for sc in _scales(root, (240, 320))])
    got = _images(os.path.join(root, 'flip'))
    for f, ids in want.items():
        assert np.array_equal(got['bike/' + f][2], ids), f


def test_two_clips_in_flight_write_the_same_files(net, bike, tmp_path):
    from cutie_amd.eval_vos import process_video_multiscale
    from cutie_amd.parallel import run_concurrent
    root = str(tmp_path)
    _copy_clip(root, ['bikeA', 'bikeB'])
    cfg = default_config()
    with torch.inference_mode():
        for c in range(2):
            process_video_multiscale(net, cfg, [sc[c] for sc in _scales(root)], os.path.join(root, 'seq'), dataset='d17-val', egress='device')
        scales = _scales(root)
        res = run_concurrent(net, range(2), lambda view, c: process_video_multiscale(view, cfg, [sc[c] for sc in scales], os.path.join(root, 'cc'),
                                                                                    dataset='d17-val', egress='device'), streams=2)
    torch.cuda.synchronize()
    assert sorted(res) == [0, 1] and all(r['frames'] == 4 for r in res.values())
    seq, cc = _files(os.path.join(root, 'seq')), _files(os.path.join(root, 'cc'))
    assert len(seq) == 8 and seq == cc
    imgs = _images(os.path.join(root, 'cc'))
    for name in ('bikeA', 'bikeB'):                               # and both copies are the clip itself
        for k in range(4):
            assert np.array_equal(imgs[f'{name}/0000{k}.png'][2], bike['host'][f'bike/0000{k}.png'][2])


def test_sizes_on_the_command_line_write_masks_and_no_scores(tmp_path, monkeypatch, capsys):
    from cutie_amd import eval_vos
    root = str(tmp_path)
    _copy_clip(root, ['bikeA', 'bikeB'])
    out = os.path.join(root, 'out')
    monkeypatch.setattr(sys, 'argv', ['eval_vos', '--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations'),
                                      '--output', out, '--sizes', '240', '320', '--egress', 'device', '--clips-in-flight', '2'])
    eval_vos.main()
    assert '8 frames' in capsys.readouterr().out
    imgs = _images(os.path.join(out, 'Annotations'))
    assert sorted(imgs) == [f'{n}/0000{k}.png' for n in ('bikeA', 'bikeB') for k in range(4)]
    assert all(v[2].shape == (480, 854) for v in imgs.values())
    assert not os.path.exists(os.path.join(out, 'Scores'))
