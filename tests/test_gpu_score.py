"""DAVIS J&F counts on the MI355X (PROB_TO_ID flags == 64, ABI 10, csrc/score.hip) against the numpy / scipy model (tests/jf_ref.py):
exact integer equality everywhere -- the kernel over shapes, planes and object lists, with the table pre-filled with garbage and guards
around it; every refusal of the launcher; and end to end: eval_vos --score with host egress, device egress, in lock step and multi-scale,
and score_masks over the folders those runs wrote."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.utils import davis_metrics as M

import jf_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 1024
LISTS = ([1], [3, 1, 2], [1, 2, 5, 9, 17, 100, 200, 254])
EVERY = sorted({i for ids in LISTS for i in ids})              # the model runs once per plane pair, over every id any list names


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device_counts(pred, gt, objects, r, scratch=None):
    """the stage on one pair -> int [n, 8]; the table is pre-filled with 0x7f bytes and sits between guards"""
    H, W = pred.shape
    n = len(objects)
    buf = torch.full((GUARD + n * 8 + GUARD,), 0x7f7f7f7f, dtype=torch.int32, device='cuda')
    counts = buf[GUARD:GUARD + n * 8].view(n, 8)
    ol = O.OpList()
    ol.jf_counts(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda(), objects, counts, scratch,
                 H=H, W=W, radius=r)
    ol.run()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0x7f7f7f7f).all()) and bool((buf[GUARD + n * 8:] == 0x7f7f7f7f).all())
    return counts.cpu().numpy().astype(np.int64)


def _shift(a, dy, dx):
    """a moved by (dy, dx), zeros coming in"""
    out = np.zeros_like(a)
    H, W = a.shape
    if dy < H and dx < W:
        out[dy:, dx:] = a[:H - dy, :W - dx]
    return out


def _planes(H, W, r):
    """[(name, pred, gt)]: every kind of plane, at every shape"""
    rng = np.random.default_rng(H * 100003 + W * 101 + r)
    cell = max(2, min(H, W) // 5)
    ids = np.array([0, 0, 0, 1, 2, 3, 5, 9, 17, 100, 200, 254, 7, 33], dtype=np.uint8)       # 7 and 33 are in no list
    blobs = rng.choice(ids, size=(-(-H // cell), -(-W // cell))).repeat(cell, 0).repeat(cell, 1)[:H, :W]
    z = np.zeros((H, W), dtype=np.uint8)
    out = [('shift<r', _shift(blobs, 0, r - 1), blobs), ('shift=r', _shift(blobs, 0, r), blobs), ('shift>r', _shift(blobs, r + 1, 0), blobs),
           ('shift=r down', _shift(blobs, r, 0), blobs)]
    # single pixels: the four corners, columns 63 | 64 (two words of a row), and the seams of the launches -- the pack kernel gives a
    # wave 4 and a block 16 consecutive words of the row-major word plane, a block of the match kernel takes 256
    WW = -(-W // 64)
    dots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(y, x) for x in (63, 64, 127, 128, 255, 256) for y in (0, H // 2) if x < W]
    for g in (4, 16, 256, 512):
        for gg in (g - 1, g):
            y, wx = divmod(gg, WW)
            if y < H:
                dots += [(y, wx * 64), (y, min(wx * 64 + 63, W - 1))]
    a, b = z.copy(), z.copy()
    for q, (y, x) in enumerate(dots):
        a[y, x] = EVERY[q % 3]
        yy, xx = min(y + (q % 3) * (r // 2 + 1), H - 1), min(x + (q % 2) * r, W - 1)        # its partner: on it, or up to beyond r away
        b[yy, xx] = EVERY[q % 3]
    out.append(('dots', a, b))
    rect = z.copy()
    rect[H // 4:H // 2 + 1, W // 4:W // 2 + 1] = 1                                          # an object that the other plane does not have at all
    out += [('pred alone', rect, z), ('gt alone', z, rect)]
    out += [('background', z, z), ('one object everywhere', z + 1, z + 1), ('everywhere against nothing', z + 2, z),
            ('checkerboard', ((np.add.outer(np.arange(H), np.arange(W)) % 2) + 1).astype(np.uint8),
             ((np.add.outer(np.arange(H), np.arange(W) + 1) % 2) + 1).astype(np.uint8))]
    void = blobs.copy()
    void[H // 4:H // 2 + 1, W // 3:] = 255                                                 # a void region in the ground truth only
    out.append(('void', blobs, void))
    noise = rng.choice(ids, size=(H, W))
    out.append(('noise', noise, _shift(noise, 1, 1)))
    return out


SHAPES = [(1, 1, 1), (5, 3, 4), (37, 70, 1), (37, 70, 2), (37, 70, 3), (64, 64, 8), (65, 129, 8), (130, 200, 8), (67, 257, 40), (480, 854, 8)]


@pytest.mark.parametrize('H,W,r', SHAPES)
def test_kernel_equals_the_model(H, W, r):
    planes = _planes(H, W, r)
    want = R.counts_batch([(p, g) for _, p, g in planes], EVERY, r)                        # [pair, id of EVERY, 8]
    scratch = torch.empty(O.OpList.jf_scratch_words(H, W, len(LISTS[-1])), dtype=torch.int32, device='cuda')
    seen = np.zeros(8, dtype=np.int64)
    for (name, pred, gt), rows in zip(planes, want):
        for objects in LISTS:
            got = _device_counts(pred, gt, objects, r, scratch if len(objects) > 1 else None)
            exp = rows[[EVERY.index(i) for i in objects]]
            assert np.array_equal(got, exp), (name, objects, got.tolist(), exp.tolist())
            seen += exp.sum(0)
    if H * W > 64:                                                                         # the cases exercise every column, and both
        assert (seen > 0).all()                                                            # matched and unmatched boundary pixels
        assert want[:, :, 4].sum() < want[:, :, 2].sum() and want[:, :, 5].sum() < want[:, :, 3].sum()


def test_the_same_launch_twice_and_a_list_in_another_order():
    H, W, r = 65, 129, 8
    _, pred, gt = _planes(H, W, r)[0]
    a = _device_counts(pred, gt, [1, 2, 5, 9], r)
    b = _device_counts(pred, gt, [1, 2, 5, 9], r)
    c = _device_counts(pred, gt, [9, 5, 2, 1], r)
    assert np.array_equal(a, b) and np.array_equal(a, c[::-1]) and a[:, 2].min() > 0


def test_refusals_come_from_the_launcher():
    H, W, n = 37, 70, 3
    ids = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    objs = torch.arange(1, 257, dtype=torch.int32, device='cuda')
    table = torch.full((256, 8), -7, dtype=torch.int32, device='cuda')
    words = O.OpList.jf_scratch_words(H, W, n)
    scratch = torch.empty(O.OpList.jf_scratch_words(H, W, 256) + 4, dtype=torch.int32, device='cuda')
    lut = torch.zeros(4, dtype=torch.int32, device='cuda')
    prob = torch.zeros((2, H, W), dtype=torch.float32, device='cuda')
    odd = torch.zeros(64, dtype=torch.int32, device='cuda')
    good = dict(flags=64, H=H, W=W, n=n, r=1, words=scratch.numel(), p0=None, p1=None, pred=ids, gt=ids, scratch=scratch, objs=objs, table=table)
    cases = [(dict(flags=64 | f, p0=prob, p1=lut), 'unknown flags') for f in (1, 2, 4, 8, 16, 32)]
    cases += [(dict(H=0), 'empty shape'), (dict(W=0), 'empty shape'), (dict(H=-1), 'empty shape'), (dict(H=1 << 16, W=1 << 15), 'exceeds 2^31'),
              (dict(n=0), '0 objects'), (dict(n=256), '256 objects'), (dict(r=0), 'radius 0'), (dict(r=41), 'radius 41'),
              (dict(pred=None), 'the predicted ids (p2)'), (dict(gt=None), 'the ground-truth ids (p3)'), (dict(scratch=None), 'the scratch (p5)'),
              (dict(objs=None), 'the object ids (p6)'), (dict(table=None), 'the counts (p7)'),
              (dict(table=odd[1:]), 'aligned'), (dict(scratch=scratch[1:]), 'aligned'), (dict(objs=odd.view(torch.uint8)[1:]), 'aligned'),
              (dict(words=words - 1), f'needs {words}')]
    lib = _lib.load()
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [2, a['H'], a['W'], H * W, W, a['r'], W, 0, a['words'], a['n']], [],
               [a['p0'], a['p1'], a['pred'], a['gt'], None, a['scratch'], a['objs'], a['table']])
        arr = ol.finalize()
        assert lib.cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in lib.cutie_hip_last_error().decode(), (change, lib.cutie_hip_last_error().decode())
    torch.cuda.synchronize()
    assert bool((table == -7).all())
    for change, msg in ((dict(objects=[0]), '1 .. 254'), (dict(objects=[255]), '1 .. 254'), (dict(objects=[4, 4]), 'duplicate'), (dict(radius=41), 'radius 41')):
        with pytest.raises(ValueError, match=msg):
            O.OpList().jf_counts(**dict(dict(pred=ids, gt=ids, objects=[1], counts=table[:len(change.get('objects', [1]))], H=H, W=W, radius=1), **change))


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    _lib.set_executor_for_testing(None)
    n = CUTIE(default_config()).cuda().eval()
    n.load_weights(S.decisive_state_dict())
    return n


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    """A copy of the tests/golden/bike frames as two videos; ground truth: frame 0 is the golden mask, the others are shifted copies of it"""
    root = str(tmp_path_factory.mktemp('score'))
    src = os.path.join(HERE, 'golden', 'bike')
    first = Image.open(os.path.join(src, '00000.png'))
    ids = np.array(first)
    for name in ('bikeA', 'bikeB'):
        img_dir, msk_dir, gt_dir = (os.path.join(root, d, name) for d in ('JPEGImages', 'Annotations', 'GT'))
        for d in (img_dir, msk_dir, gt_dir):
            os.makedirs(d)
        shutil.copy(os.path.join(src, '00000.png'), msk_dir)
        for t in range(4):
            shutil.copy(os.path.join(src, f'0000{t}.jpg'), img_dir)
            im = Image.fromarray(_shift(ids, 2 * t, 5 * t))
            im.putpalette(first.getpalette())
            im.save(os.path.join(gt_dir, f'0000{t}.png'))
    for d in ('JPEGImages', 'Annotations', 'GT'):                 # and a dataset of one video for the plain runs
        shutil.copytree(os.path.join(root, d, 'bikeA'), os.path.join(root, 'one', d, 'bikeA'))
    return root


def _args(argv):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(argv)
    E.check_args(ap, args)
    return args


def _model_scores(results, gt, name, frames):
    gts = [np.array(Image.open(os.path.join(gt, name, f))) for f in frames]
    first = np.array(Image.open(os.path.join(gt, name, sorted(os.listdir(os.path.join(gt, name)))[0])))
    objects = list(range(1, int(first[first != 255].max()) + 1))
    preds = [np.array(Image.open(os.path.join(results, name, f))) for f in frames]
    c = R.counts_batch(list(zip(preds, gts)), objects, M.bound_pix(*gts[0].shape))
    return {'objects': objects, 'frames': list(frames), 'counts': c.tolist(), 'J': M.j_from_counts(c).tolist(), 'F': M.f_from_counts(c).tolist()}


def _read(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith('.csv') or f == 'scores.json'}


def _check_run(root, out, names, frames=('00001.png', '00002.png')):
    """scores.json of a run = the model over the PNGs that run wrote; its CSVs = write_results of those counts; score_masks agrees"""
    from cutie_amd.score_masks import score_folders
    gt, ann = os.path.join(root, 'GT'), os.path.join(out, 'Annotations')
    want = {n: _model_scores(ann, gt, n, frames) for n in names}
    back = json.load(open(os.path.join(out, 'scores.json')))
    assert sorted(back['sequences']) == sorted(names)
    for n in names:
        assert back['sequences'][n]['counts'] == want[n]['counts'], n
        assert back['sequences'][n] == want[n], n
    M.write_results(os.path.join(out, 'model'), 'd17-val', want)
    score_folders(ann, gt, dataset='d17-val', output=os.path.join(out, 'again'))
    files = _read(out)
    assert len(files) == 3 and files == _read(os.path.join(out, 'model')) == _read(os.path.join(out, 'again'))
    return want


def test_eval_vos_score_host_device_lockstep(net, dataset, capsys):
    from cutie_amd import eval_vos as E
    root = dataset
    one = os.path.join(root, 'one')
    got = {}
    for name, base, names, extra in (('host', one, ['bikeA'], []), ('device', one, ['bikeA'], ['--egress', 'device']),
                                     ('lockstep', root, ['bikeA', 'bikeB'], ['--egress', 'device', '--lockstep', '2'])):
        out = os.path.join(root, 'out_' + name)
        args = _args(['--images', os.path.join(base, 'JPEGImages'), '--masks', os.path.join(base, 'Annotations'), '--gt', os.path.join(base, 'GT'),
                      '--output', out, '--dataset', 'd17-val', '--score'] + extra)
        res = E.run_dataset(net, default_config(), args)
        assert all(r['frames'] == 4 and r['scores'] is not None for r in res.values())
        assert 'd17-val: J&F-Mean' in capsys.readouterr().out
        got[name] = _check_run(base, out, names)
    first = got['host']['bikeA']
    assert len(first['objects']) >= 1 and np.asarray(first['counts'])[:, 0, 7].min() > 0   # the ground truth has its object on the scored frames
    assert got['device'] == got['host']                            # the same masks, the same counts
    assert got['lockstep']['bikeA'] == got['lockstep']['bikeB']    # two copies of one video side by side


def test_eval_vos_score_multiscale_and_all_frames(net, dataset):
    from cutie_amd import eval_vos as E
    root = os.path.join(dataset, 'one')
    assert os.path.isdir(root)
    out = os.path.join(dataset, 'out_sizes')
    args = _args(['--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations'), '--gt', os.path.join(root, 'GT'),
                  '--output', out, '--dataset', 'd17-val', '--score', '--score-all-frames', '--sizes', '480', '600', '--egress', 'device'])
    res = E.run_dataset(net, default_config(), args)
    assert res[0]['frames'] == 4 and len(res[0]['scores']['frames']) == 4
    want = _check_run_all(root, out)
    assert np.asarray(want['bikeA']['counts'])[0, 0, 0] > 0         # frame 0 comes back as its input mask: it overlaps the ground truth


def _check_run_all(root, out):
    """as _check_run, every frame scored"""
    from cutie_amd.score_masks import score_folders
    gt, ann = os.path.join(root, 'GT'), os.path.join(out, 'Annotations')
    want = {'bikeA': _model_scores(ann, gt, 'bikeA', [f'0000{t}.png' for t in range(4)])}
    back = json.load(open(os.path.join(out, 'scores.json')))
    assert back['sequences'] == want
    M.write_results(os.path.join(out, 'model'), 'd17-val', want)
    score_folders(ann, gt, dataset='d17-val', output=os.path.join(out, 'again'), score_all_frames=True)
    assert _read(out) == _read(os.path.join(out, 'model')) == _read(os.path.join(out, 'again'))
    return want
