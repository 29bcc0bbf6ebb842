"""BURST egress on the MI355X (PROB_TO_ID flags == 32, ABI 9, csrc/rle.hip): the device RLE encoder against the numpy codec
(cutie_amd/inference/utils/coco_rle.py) byte for byte, with guard bytes around the stream, the table and the status; run-to-run identity;
every argument check of the launcher; the capacity bit; and end to end: ResultSaver and eval_vos with egress='device' against 'host'."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.inference.utils import coco_rle as R

import burst_fixture as BF

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0xA5


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _encode(plane, objects, cap=None, scratch_words=None):
    """-> (strings or None on overflow, table [n, 4], status [4]); asserts the guards around the three outputs."""
    H, W = plane.shape
    n = len(objects)
    want = [R.encode(plane == o) for o in objects]
    if cap is None:
        cap = sum(len(s) for s in want) + 5
    ids = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.uint8)).cuda()
    objs = torch.tensor(list(objects) or [0], dtype=torch.int32).cuda()
    buf = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    tab = torch.full((GUARD + 4 * max(n, 1) + GUARD,), -7, dtype=torch.int32, device='cuda')
    sta = torch.full((GUARD + 4 + GUARD,), -7, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.rle_scratch_words(H, W, n) if scratch_words is None else scratch_words, dtype=torch.int32, device='cuda')
    stream, table, status = buf[GUARD:GUARD + cap], tab[GUARD:GUARD + 4 * max(n, 1)].view(-1, 4), sta[GUARD:GUARD + 4]
    ol = O.OpList()
    ol.rle_encode(ids, objs, stream, table, status, scratch, H=H, W=W, n_objects=n)
    ol.run()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + cap:] == FILL).all())
    assert bool((tab[:GUARD] == -7).all()) and bool((tab[GUARD + 4 * n:] == -7).all())
    assert bool((sta[:GUARD] == -7).all()) and bool((sta[GUARD + 4:] == -7).all())
    st, tb, raw = status.cpu().numpy(), table.cpu().numpy()[:n], stream.cpu().numpy().tobytes()
    if st[1] != 0:
        assert bool((stream == FILL).all())
        return None, tb, st
    return [raw[o:o + ln].decode('ascii') for o, ln, _, _ in tb], tb, st


def _check(plane, objects):
    got, tb, st = _encode(plane, objects)
    want = [R.encode(plane == o) for o in objects]
    assert got == want
    counts = [R.counts_of(plane == o) for o in objects]
    assert tb[:, 2].tolist() == [len(c) for c in counts]
    assert tb[:, 3].tolist() == [int((plane == o).sum()) for o in objects]
    assert tb[:, 0].tolist() == np.concatenate(([0], np.cumsum([len(s) for s in want])))[:-1].astype(int).tolist()
    assert st.tolist() == [sum(len(s) for s in want), 0, sum(len(c) for c in counts), 0]
    return got


SHAPES = [(1, 1), (1, 13), (13, 1), (5, 7), (37, 53), (101, 149)]


@pytest.mark.parametrize('H,W', SHAPES)
def test_kernel_matches_the_numpy_codec(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    z = np.zeros((H, W), dtype=np.uint8)
    _check(z, [1, 2])                                            # all background: one count each
    _check(np.full((H, W), 9, dtype=np.uint8), [9])              # one object covering everything: counts [0, H W]
    _check(np.full((H, W), 9, dtype=np.uint8), [3, 9, 200])      # ... and two listed but absent
    m = z.copy()
    m[0, 0] = m[-1, -1] = 4                                      # first and last pixel
    _check(m, [4])
    if H > 2 and W > 1:                                          # the bottom rows of one column and the top rows of the next: ONE run
        m = z.copy()
        m[H - 2:, W // 2 - 1] = 6
        m[:2, W // 2] = 6
        got = _check(m, [6])
        assert len(R.from_string(got[0])) == 3
    blobs = rng.integers(0, 6, size=(-(-H // 4), -(-W // 3))).astype(np.uint8).repeat(4, 0).repeat(3, 1)[:H, :W]
    _check(blobs, [1, 2, 3, 4, 5])
    _check(blobs, [5, 2])                                        # ids present but not listed count as background, any list order
    _check(blobs, [7, 1, 250])                                   # listed but absent between present ones
    noise = rng.integers(0, 4, size=(H, W)).astype(np.uint8)
    _check(noise, [1, 2, 3])
    _check(noise, [])                                            # no object: an empty stream


def test_255_objects_of_per_pixel_random_ids():
    rng = np.random.default_rng(7)
    plane = rng.integers(1, 256, size=(37, 53)).astype(np.uint8)
    _check(plane, list(range(1, 256)))
    _check(plane, list(range(255, 0, -1)))


def test_720p_single_far_pixel_and_blobs():
    m = np.zeros((720, 1280), dtype=np.uint8)
    m[-1, -1] = 3
    got = _check(m, [3, 1])
    assert R.from_string(got[0]) == [720 * 1280 - 1, 1] and len(got[0]) == 6
    yy, xx = np.mgrid[:720, :1280]
    for k, (cy, cx, r) in enumerate([(200, 300, 150), (500, 900, 180), (360, 640, 90), (700, 20, 60)]):
        m[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    _check(m, [1, 2, 3, 4])


def test_the_same_launch_twice_gives_the_same_bytes():
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 9, size=(101, 149)).astype(np.uint8)
    a, ta, sa = _encode(plane, list(range(1, 9)))
    b, tb, sb = _encode(plane, list(range(1, 9)))
    assert a == b and np.array_equal(ta, tb) and np.array_equal(sa, sb)


def test_refusals_come_from_the_launcher():
    H, W, n = 37, 53, 3
    ids = torch.zeros((H, W), dtype=torch.uint8, device='cuda')
    objs = torch.arange(1, 257, dtype=torch.int32, device='cuda')
    stream = torch.full((4096,), FILL, dtype=torch.uint8, device='cuda')
    table = torch.full((256, 4), -7, dtype=torch.int32, device='cuda')
    status = torch.full((4,), -7, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.rle_scratch_words(H, W, 256), dtype=torch.int32, device='cuda')
    lut = torch.zeros(4, dtype=torch.int32, device='cuda')
    prob = torch.zeros((2, H, W), dtype=torch.float32, device='cuda')
    good = dict(flags=32, H=H, W=W, n=n, words=scratch.numel(), p0=None, p1=None, stream=stream, status=status, table=table)
    cases = [(dict(flags=32 | f, p0=prob, p1=lut), 'unknown flags') for f in (1, 2, 4, 8, 16)]
    cases += [(dict(stream=None), 'the stream (p3)'), (dict(status=None), 'the status (p4)'), (dict(table=None), 'the table (p7)'),
              (dict(status=stream[1:]), 'aligned'),
              (dict(H=0), 'empty shape'), (dict(W=0), 'empty shape'), (dict(n=256), '256 objects'),
              (dict(words=O.OpList.rle_scratch_words(H, W, n) - 1), 'scratch of')]
    lib = _lib.load()
    for change, msg in cases:
        a = dict(good, **change)
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, a['flags'], [2, a['H'], a['W'], H * W, W, H, W, stream.numel(), a['words'], a['n']], [],
               [a['p0'], a['p1'], ids, a['stream'], a['status'], scratch, objs, a['table']])
        arr = ol.finalize()
        assert lib.cutie_exec(arr.ctypes.data, 1, torch.cuda.current_stream().cuda_stream) == -2, change
        assert msg in lib.cutie_hip_last_error().decode(), (change, lib.cutie_hip_last_error().decode())
    torch.cuda.synchronize()
    assert bool((stream == FILL).all()) and bool((table == -7).all()) and bool((status == -7).all())
    with pytest.raises(ValueError, match='256 objects'):
        O.OpList().rle_encode(ids, objs, stream, table, status, scratch, H=H, W=W, n_objects=256)


def test_a_short_stream_sets_the_error_bit_and_writes_nothing():
    rng = np.random.default_rng(11)
    plane = rng.integers(0, 5, size=(37, 53)).astype(np.uint8)
    objects = [1, 2, 3, 4]
    need = sum(len(R.encode(plane == o)) for o in objects)
    for cap in (need - 1, need // 2, 0):
        got, tb, st = _encode(plane, objects, cap=cap)               # (_encode asserts the guards and the untouched stream)
        assert got is None and st.tolist()[:2] == [need, 1]
        assert tb[:, 1].tolist() == [len(R.encode(plane == o)) for o in objects]
    got, _, _ = _encode(plane, objects, cap=need)                    # exactly enough
    assert got == [R.encode(plane == o) for o in objects]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.config import default_config
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


def _smooth_probs(P, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.interpolate(torch.randn(1, P, max(h // 16, 2), max(w // 16, 2), generator=g), size=(h, w), mode='bicubic',
                                        align_corners=False)[0] * 4 + torch.randn(P, h, w, generator=g) * 0.3
    return torch.softmax(x, 0).cuda()


def _pngs(root):
    return {os.path.relpath(os.path.join(dp, f), root): np.array(Image.open(os.path.join(dp, f)))
            for dp, _, fs in os.walk(root) for f in fs if f.endswith('.png')}


def test_saver_device_egress_writes_the_host_json(gpu_net, tmp_path, monkeypatch):
    """One annotated and one other frame through ResultSaver, egress 'host' | 'device' | 'device' with a stream too short for the
    strings (the writer encodes such a frame on the host): equal video_json, equal PNG pixels."""
    from cutie_amd.config import default_config
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.inference.utils import results_utils as RU
    core = InferenceCore(gpu_net, cfg=default_config())
    core.object_manager.add_new_objects([1, 2, 5, 9])
    H, W = 101, 149
    frames = [('00000.jpg', _smooth_probs(4, H, W, 1)), ('00001.jpg', _smooth_probs(4, H, W, 2))]       # plane 4 (object 9) does not exist: absent
    frames = [(f, torch.cat([p, torch.zeros_like(p[:1])])) for f, p in frames]
    init = json.loads(json.dumps(BF.sequence('bike')))
    got = {}
    for name, eg in (('host', 'host'), ('device', 'device'), ('short', 'device')):
        if name == 'short':
            monkeypatch.setattr(RU, 'RLE_SLAB', RU.RLE_TABLE + 8)
        saver = RU.ResultSaver(os.path.join(str(tmp_path), name), 'bike', dataset='burst-val', object_manager=core.object_manager,
                               use_long_id=False, palette=RU.davis_palette, init_json=init, processor=core, egress=eg)
        assert saver.egress == eg
        with torch.inference_mode():
            for f, p in frames:
                saver.process(p, f)
        saver.end()
        got[name] = (json.dumps(saver.video_json), _pngs(os.path.join(str(tmp_path), name)))
        if name == 'short':
            assert saver._rle_warned
        elif eg == 'device':
            assert not saver._rle_warned
    seg = json.loads(got['host'][0])['segmentations']
    lut = np.array([0, 1, 2, 5, 9])
    ids = lut[frames[0][1].argmax(0).cpu().numpy()]
    assert seg[1] == {} and sorted(seg[0]) == [str(v) for v in np.unique(ids) if v != 0] and len(seg[0]) >= 2 and '9' not in seg[0]
    for oid, s in seg[0].items():
        assert np.array_equal(R.decode(s['rle'], H, W), ids == int(oid))
    for name in ('device', 'short'):
        assert got[name][0] == got['host'][0]
        assert sorted(got[name][1]) == sorted(got['host'][1]) == ['bike/00000.png', 'bike/00001.png']
        for k, v in got['host'][1].items():
            assert np.array_equal(got[name][1][k], v), (name, k)


def test_eval_vos_device_egress_writes_the_host_predictions(tmp_path, monkeypatch, capsys):
    """The command line on a two-sequence BURST dataset: --egress host | device | device in lock step -> equal predictions.json, whose
    strings are the PNGs of their frames."""
    import sys
    from cutie_amd import eval_vos
    from test_burst_cpu import check_predictions
    images, json_path, _ = BF.make(tmp_path, names=('bikeA', 'bikeB'))
    preds = {}
    for name, extra in (('host', []), ('device', ['--egress', 'device']), ('lockstep', ['--egress', 'device', '--lockstep', '2'])):
        out = os.path.join(str(tmp_path), name)
        monkeypatch.setattr(sys, 'argv', ['eval_vos', '--dataset', 'burst-val', '--images', images, '--json', json_path, '--output', out] + extra)
        eval_vos.main()
        assert '8 frames' in capsys.readouterr().out
        preds[name] = check_predictions(out, ('bikeA', 'bikeB'))
    assert preds['device'] == preds['host'] and preds['lockstep'] == preds['host']
    a, b = _pngs(os.path.join(str(tmp_path), 'host')), _pngs(os.path.join(str(tmp_path), 'device'))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
