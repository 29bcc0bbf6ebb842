"""The batch JPEG decode on CPU (RESIZE flags 8 / 16 / 32 with 256): the layout and the descriptor builders, ``jpegs_to_device`` /
``to_device_many`` under the interpreter of tests/jpeg_batch_ref.py against the one-frame forms and PIL, the batched look-ahead
``Window``, and the drivers with ``decode_batch`` 3 against 1 and against the host path: the same PNG bytes."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.data import jpeg as J
from cutie_amd.inference.data import device_ingest as DI
from cutie_amd.inference.data.prefetch import Window, fill_together, pop_together
from oracle.weights import make_state_dict

import jpeg_corpus
from jpeg_batch_ref import JpegBatchMock, check_row
from test_ingest_cpu import _dataset, _make_video, _pngs

CORPUS = jpeg_corpus.corpus(large=False)
SMALL = [(n, d) for n, d in CORPUS if len(d) < 20000 and '480x854' not in n and 'bike' not in n and 'judo' not in n]


def _packets(cases, **kw):
    out = []
    for name, data in cases:
        pkt, why = J.parse(data, **kw)
        assert pkt is not None, (name, why)
        pkt.source = name
        out.append(pkt)
    return out


@pytest.fixture
def batch_exec():
    before = _lib._executor
    _lib.set_executor_for_testing(JpegBatchMock())
    JpegBatchMock.reset()
    yield
    _lib.set_executor_for_testing(before)


# ---- layout and builders -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('guard', [0, 64])
def test_layout_over_the_corpus(guard):
    assert len(CORPUS) == 61
    pkts = _packets(CORPUS)
    rounds = 3
    table, sz = O.OpList.jpeg_layout(pkts, rounds=rounds, guard=guard)
    assert table.dtype == np.int32 and table.shape == (61, 8) and sz['rounds'] == rounds
    unit = {'packets': 1, 'work': 4, 'coef': 2, 'planes': 1, 'rgb': 1}                 # bytes per element
    align = {'packets': 16, 'work': 8, 'coef': 16, 'planes': 8, 'rgb': 16}             # bytes
    for col, name in enumerate(('packets', 'work', 'coef', 'planes', 'rgb')):
        end = 0                                                                        # bytes used so far
        for k, pkt in enumerate(pkts):
            own = pkt.buf.nbytes if name == 'packets' else J.stage_sizes(pkt, rounds)[name]
            off = int(table[k, col]) * unit[name]
            g = guard if name in ('coef', 'planes', 'rgb') else 0
            assert off % align[name] == 0, (name, k)
            assert off >= end + g, (name, k, 'overlaps its predecessor or its guard')
            end = off + own * unit[name] + g
        assert end <= sz[name] * unit[name] < 1 << 31, name
    h = np.stack([p.hdr for p in pkts])
    assert table[:, 5].tolist() == [p.buf.nbytes for p in pkts] and table[:, 6].tolist() == (3 * h[:, J.HDR_W]).tolist()
    assert not table[:, 7].any()
    assert (sz['max_chunk'], sz['max_seg'], sz['max_block']) == tuple(int(h[:, c].max()) for c in (J.HDR_NCHUNK, J.HDR_NSEG, J.HDR_NBLOCK))
    assert sz['max_pix'] == int((h[:, J.HDR_H].astype(np.int64) * h[:, J.HDR_W]).max())
    # the check the kernels make passes on every row of a layout, and fails where the header asks for more chunks than the row holds
    blob = np.zeros(sz['packets'], dtype=np.uint8)
    for k, p in enumerate(pkts):
        blob[table[k, 0]:table[k, 0] + p.buf.nbytes] = p.buf
    ints = [61] + [sz[k] for k in ('packets', 'work', 'coef', 'planes', 'rgb', 'rounds', 'max_chunk', 'max_seg', 'max_block', 'max_pix')]
    assert all(check_row(table, k, blob, ints) is not None for k in range(61))
    blob[table[5, 0]:table[5, 0] + 256].view(np.int32)[J.HDR_NCHUNK] += 1
    assert check_row(table, 5, blob, ints) is None and check_row(table, 6, blob, ints) is not None


def test_layout_refuses_a_bad_guard_and_2_gib():
    pkts = _packets(CORPUS[:2])
    with pytest.raises(ValueError, match='guard'):
        O.OpList.jpeg_layout(pkts, guard=8)

    class Big:                                                                          # a packet whose header claims 2^24 blocks
        def __init__(self, p):
            self.buf, self.hdr = p.buf, p.hdr.copy()
            self.hdr[J.HDR_NBLOCK] = 1 << 24
    with pytest.raises(ValueError, match='2\\^31'):
        O.OpList.jpeg_layout([Big(pkts[0])] * 2)


def test_builders_fill_the_documented_fields():
    pkts = _packets(SMALL[:3])
    table, sz = O.OpList.jpeg_layout(pkts, rounds=2)
    blob = torch.zeros(sz['packets'], dtype=torch.uint8)
    tab = torch.from_numpy(table)
    work, coef = torch.zeros(sz['work'], dtype=torch.int32), torch.zeros(sz['coef'], dtype=torch.int16)
    planes, rgb = torch.zeros(sz['planes'], dtype=torch.uint8), torch.zeros(sz['rgb'], dtype=torch.uint8)
    status = torch.zeros((3, 4), dtype=torch.int32)
    ol = O.OpList(prio=False)
    ol.jpeg_huff_batch(blob, tab, sz, status, n=3, work=work, coef=coef)
    ol.jpeg_idct_batch(blob, tab, sz, status, n=3, coef=coef, planes=planes)
    ol.jpeg_color_batch(blob, tab, sz, status, n=3, planes=planes, rgb=rgb)
    arr = ol.finalize()
    assert arr['kind'].tolist() == [O.RESIZE] * 3 and arr['flags'].tolist() == [256 | 8, 256 | 16, 256 | 32]
    want = [3, sz['packets'], sz['work'], sz['coef'], sz['planes'], sz['rgb'], 2, sz['max_chunk'], sz['max_seg'], sz['max_block'], sz['max_pix']]
    for k in range(3):
        assert arr['i'][k, :11].tolist() == want
        assert arr['p'][k, [0, 1, 6]].tolist() == [blob.data_ptr(), tab.data_ptr(), status.data_ptr()]
    assert arr['p'][0, 2:6].tolist() == [work.data_ptr(), coef.data_ptr(), 0, 0]
    assert arr['p'][1, 2:6].tolist() == [0, coef.data_ptr(), planes.data_ptr(), 0]
    assert arr['p'][2, 2:6].tolist() == [0, 0, planes.data_ptr(), rgb.data_ptr()]
    for bad in (dict(n=0), dict(n=65536)):
        with pytest.raises(ValueError, match='images'):
            O.OpList(prio=False).jpeg_huff_batch(blob, tab, sz, status, work=work, coef=coef, **bad)
    with pytest.raises(ValueError, match='coef'):
        O.OpList(prio=False).jpeg_huff_batch(blob, tab, sz, status, n=3, work=work, coef=coef.int())
    with pytest.raises(ValueError, match='rgb'):
        O.OpList(prio=False).jpeg_color_batch(blob, tab, sz, status, n=3, planes=planes, rgb=rgb[:-1])
    with pytest.raises(ValueError, match='status'):
        O.OpList(prio=False).jpeg_idct_batch(blob, tab, sz, status[:2], n=3, coef=coef, planes=planes)
    with pytest.raises(ValueError, match='table'):
        O.OpList(prio=False).jpeg_idct_batch(blob, tab.long(), sz, status, n=3, coef=coef, planes=planes)


def test_a_stale_library_is_refused(monkeypatch):
    """Outside the interpreter the builders ask the library for the forms first (no new ABI number came with them)."""
    pkts = _packets(SMALL[:1])
    table, sz = O.OpList.jpeg_layout(pkts)
    _lib.set_executor_for_testing(None)
    monkeypatch.setattr(_lib, 'has_jpeg_batch', lambda: False)
    with pytest.raises(_lib.HipLibraryError, match='stale'):
        O.OpList(prio=False).jpeg_idct_batch(torch.zeros(sz['packets'], dtype=torch.uint8), torch.from_numpy(table), sz,
                                             torch.zeros((1, 4), dtype=torch.int32), n=1, coef=torch.zeros(sz['coef'], dtype=torch.int16),
                                             planes=torch.zeros(sz['planes'], dtype=torch.uint8))


# ---- jpegs_to_device / to_device_many under the interpreter -----------------------------------------------------------------------------
def test_batch_frames_equal_the_one_frame_decode_and_pil(batch_exec):
    pkts = _packets(SMALL)
    assert len(pkts) >= 20
    sizes = [None if k % 3 else (max(1, p.shape[0] // 2), max(1, p.shape[1] // 2 + 1)) for k, p in enumerate(pkts)]
    frames, u8s = DI.jpegs_to_device(pkts, 'cpu', sizes, keep_u8=True, guard=32)
    assert JpegBatchMock.batch_ops == {8: 1, 16: 1, 32: 1} and JpegBatchMock.one_frame == 0
    for k, (pkt, (name, data)) in enumerate(zip(pkts, SMALL)):
        one = DI.jpeg_to_device(pkt, 'cpu', sizes[k])
        assert frames[k].dtype == torch.float32 and frames[k].is_contiguous() and torch.equal(frames[k], one), name
        assert np.array_equal(u8s[k].numpy(), jpeg_corpus.pil_rgb(data)), name
    assert JpegBatchMock.one_frame == 3 * len(pkts)


def test_a_truncated_file_raises_with_its_name(batch_exec):
    cases = [c for c in SMALL if '17x9' in c[0] or '120x160' in c[0]][:5]
    pkts = _packets(cases)
    data = cases[3][1]
    bad, why = J.parse(data[:len(data) * 2 // 3])
    assert bad is not None, why
    bad.source = 'cut.jpg'
    pkts[3] = bad
    with pytest.raises(ValueError, match='cut.jpg'):
        DI.jpegs_to_device(pkts, 'cpu')
    before = dict(DI.decode_stats)
    frames, chk = DI.jpegs_to_device(pkts, 'cpu', check=False)                          # no error yet
    for k in (0, 1, 2, 4):
        chk(k)
        assert np.array_equal((frames[k] * 255).round().byte().permute(1, 2, 0).numpy(), jpeg_corpus.pil_rgb(cases[k][1]))
    assert DI.decode_stats['frames'] == before['frames'] + 4
    with pytest.raises(ValueError, match='cut.jpg'):
        chk(3)
    chk()                                                                               # everything has been looked at
    assert DI.decode_stats['frames'] == before['frames'] + 4
    names = list('abcde')
    with pytest.raises(ValueError, match='^d: '):
        DI.jpegs_to_device(pkts, 'cpu', names=names)


def test_to_device_many_with_a_progressive_file_in_the_middle(tmp_path, batch_exec):
    root = str(tmp_path)
    _make_video(root, 'v', n=4, h=64, w=96)
    frame = os.path.join(root, 'JPEGImages', 'v', '00002.jpg')
    Image.open(frame).save(frame, format='JPEG', quality=95, progressive=True)
    dec = next(iter(_dataset(root, ingest='device-decode').get_datasets()))
    again = next(iter(_dataset(root, ingest='device-decode').get_datasets()))
    recs = [dec[t] for t in range(4)]
    assert ['jpeg' in r for r in recs] == [True, True, False, True] and dict(dec.decode_fallbacks) == {'progressive': 1}
    many = DI.to_device_many(recs, 'cpu', keep_u8=True)
    assert JpegBatchMock.batch_ops[8] == 1 and JpegBatchMock.one_frame == 0
    assert ['decode_check' in r for r in many] == [True, True, False, True]
    loop = [DI.to_device(again[t], 'cpu', keep_u8=True) for t in range(4)]
    for t, (a, b) in enumerate(zip(many, loop)):
        a = DI.finish(a)
        assert set(a) == set(b) and set(a['info']) == set(b['info']), t
        assert torch.equal(a['rgb'], b['rgb']) and torch.equal(a['info']['image_u8'], b['info']['image_u8']), t
        assert {k: v for k, v in a['info'].items() if k != 'image_u8'} == {k: v for k, v in b['info'].items() if k != 'image_u8'}
    eager = DI.to_device_many([next(iter(_dataset(root, ingest='device-decode').get_datasets()))[t] for t in range(4)], 'cpu', defer_check=False)
    assert not any('decode_check' in r for r in eager)


# ---- the batched window ------------------------------------------------------------------------------------------------------------------
class _Uploads:
    """Records are ints; an uploaded record is a dict whose check raises for the frames in ``bad``."""

    def __init__(self, bad=()):
        self.bad, self.calls, self.checked = set(bad), [], []

    def one(self, r):
        self.calls.append([r])
        return {'id': r}

    def many(self, records, owners):
        self.calls.append(list(records))
        assert len(owners) == len(records)
        return [{'id': r} for r in records]

    def check(self, rec):
        self.checked.append(rec['id'])
        if rec['id'] in self.bad:
            raise ValueError(f'frame {rec["id"]}')
        return rec


@pytest.mark.parametrize('n', [0, 1, 7, 12, 13])
@pytest.mark.parametrize('depth', [1, 5, 16])
def test_batched_window_pops_the_same_sequence_and_never_sees_less(n, depth):
    a, b = _Uploads(), _Uploads()
    w1 = Window(iter(range(n)), a.one, a.check, depth)
    w4 = Window(iter(range(n)), None, b.check, depth, upload_many=b.many, batch=4)
    seq = []
    while w1.queued:
        assert w4.queued
        r1, r4 = w1.pop(), w4.pop()
        assert r1 == r4
        seq.append(r4['id'])
        assert len(w4.queued) >= len(w1.queued)
        assert [r['id'] for r in w4.queued] == list(range(r4['id'] + 1, r4['id'] + 1 + len(w4.queued)))
    assert not w4.queued and seq == list(range(n))
    assert [r for c in b.calls for r in c] == list(range(n))                            # every record uploaded once, in order
    assert all(len(c) == 4 for c in b.calls[:-1]) and (not b.calls or 1 <= len(b.calls[-1]) <= 4)
    assert len(b.calls) == -(-n // 4)                                                   # the last partial group included


def test_batch_1_is_the_old_path():
    a = _Uploads()
    w = Window(iter(range(3)), a.one, a.check, 2, upload_many=a.many, batch=1)
    assert a.calls == [[0], [1]] and w.depth == 2
    with pytest.raises(ValueError, match='upload_many'):
        Window(iter(range(3)), a.one, a.check, 2, batch=2)


def test_the_deferred_check_fires_at_the_pop_of_the_bad_frame():
    u = _Uploads(bad={5})
    w = Window(iter(range(9)), None, u.check, 2, upload_many=u.many, batch=4)
    assert [r for c in u.calls for r in c] == [0, 1, 2, 3]                             # frame 5 is not up yet
    for t in range(5):
        assert w.pop()['id'] == t                                                       # 5 is uploaded on the way, and not checked
    assert 5 in [r for c in u.calls for r in c] and u.checked == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match='frame 5'):
        w.pop()


def test_windows_fill_together_and_a_dry_feed_drops_out():
    u = _Uploads()
    ws = [Window(iter(range(100 * c, 100 * c + n)), None, u.check, 3, upload_many=u.many, batch=3, tag=c, fill=False)
          for c, n in enumerate((8, 4))]
    fill_together(ws)
    assert u.calls == [[0, 1, 2, 100, 101, 102]] and [len(w.queued) for w in ws] == [3, 3]
    got = [[], []]
    for t in range(4):
        for c, r in enumerate(pop_together(ws)):
            got[c].append(r['id'])
    # one joint call for both; the short feed has ended and dropped out, the long one goes on alone
    assert u.calls[1:] == [[3, 4, 5, 103], [6, 7]] and ws[1].dry and not ws[1].queued
    while ws[0].queued:
        got[0].append(pop_together(ws[:1])[0]['id'])
    assert got == [list(range(8)), list(range(100, 104))] and len(u.calls) == 3


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def batch_net():
    from cutie_amd.model.cutie import CUTIE
    mx = JpegBatchMock()
    mx.per_sample_conv = True
    before = _lib._executor
    _lib.set_executor_for_testing(mx)
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net, mx
    _lib.set_executor_for_testing(before)


@pytest.fixture
def net(batch_net):
    before = _lib._executor
    _lib.set_executor_for_testing(batch_net[1])
    yield batch_net[0]
    _lib.set_executor_for_testing(before)


def _three_ways(root, run):
    """run(tag, ingest, decode_batch) for 'host', B = 1 and B = 3 -> the batch ops of the B = 3 run; the PNG bytes must agree."""
    out, ops = {}, None
    with torch.inference_mode():
        for tag, ingest, B in (('host', 'host', 1), ('b1', 'device-decode', 1), ('b3', 'device-decode', 3)):
            JpegBatchMock.reset()
            run(os.path.join(root, tag), ingest, B)
            out[tag] = _pngs(os.path.join(root, tag))
            if tag == 'b1':
                assert not JpegBatchMock.batch_ops and JpegBatchMock.one_frame > 0         # the default does not reach the new forms
            if tag == 'b3':
                assert JpegBatchMock.one_frame == 0
                ops = dict(JpegBatchMock.batch_ops)
                assert ops[8] == ops[16] == ops[32]
    assert out['host'] and out['b1'] == out['host'] and out['b3'] == out['host']
    return ops[8], len(out['host'])


def test_eval_vos_one_clip(tmp_path, net):
    from cutie_amd.eval_vos import process_video
    root = str(tmp_path)
    _make_video(root, 'vA', n=7, ids=(1, 2), seed=21)
    cfg = default_config(mem_every=2)

    def run(out, ingest, B):
        rd = next(iter(_dataset(root, ingest=ingest).get_datasets()))
        assert process_video(net, cfg, rd, out, decode_batch=B)['frames'] == 7
    assert _three_ways(root, run) == (3, 7)                                              # ceil(7 / 3) launch chains


def test_eval_vos_lockstep_of_unequal_lengths(tmp_path, net):
    from cutie_amd.eval_vos import process_videos_lockstep
    root = str(tmp_path)
    _make_video(root, 'vA', n=5, ids=(1, 2), seed=21)
    _make_video(root, 'vB', n=3, ids=(4, 9), seed=22)
    cfg = default_config(mem_every=2)

    def run(out, ingest, B):
        process_videos_lockstep(net, cfg, list(_dataset(root, ingest=ingest).get_datasets()), out, decode_batch=B)
    assert _three_ways(root, run) == (2, 8)                                              # ceil(5 / 3): the two feeds fill together


def test_eval_vos_two_scales(tmp_path, net):
    from cutie_amd.eval_vos import process_video_multiscale
    root = str(tmp_path)
    _make_video(root, 'vA', n=4, ids=(1, 2), seed=23)
    cfg = default_config(mem_every=2)

    def run(out, ingest, B):
        rds = [next(iter(_dataset(root, size=s, ingest=ingest).get_datasets())) for s in (-1, 48)]
        process_video_multiscale(net, cfg, rds, out, decode_batch=B)
    assert _three_ways(root, run) == (2, 4)


def test_process_video(tmp_path, net):
    from cutie_amd.process_video import process_video, video_config
    from cutie_amd.inference.utils.results_utils import davis_palette
    from cutie_amd.utils.synth import SyntheticClip
    root = str(tmp_path)
    clip = SyntheticClip(64, 96, 2, 5, seed=5)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(5):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(clip.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    cfg = video_config(mem_every=2)

    def run(out, ingest, B):
        assert process_video(net, cfg, os.path.join(root, 'frames'), os.path.join(root, 'masks'), out, ingest=ingest, decode_batch=B)['frames'] == 5
    assert _three_ways(root, run) == (1 + 2, 5)                                          # the annotated frame, then ceil(5 / 3)


def test_command_line_rules():
    from cutie_amd import eval_vos as E, process_video as PV
    ap = E.arg_parser()
    base = ['--images', 'i', '--masks', 'm', '--output', 'o']
    assert ap.parse_args(base).decode_batch == 1 and ap.parse_args(base).ingest == 'host'          # the defaults stay
    args = ap.parse_args(base + ['--ingest', 'device-decode', '--decode-batch', '8'])
    E.check_args(ap, args)
    assert args.decode_batch == 8
    with pytest.raises(SystemExit):
        E.check_args(ap, ap.parse_args(base + ['--decode-batch', '0']))
    pv = PV.arg_parser().parse_args(['-v', 'v', '-m', 'm', '-o', 'o'])
    assert pv.decode_batch == 1 and pv.ingest == 'host'


def test_decode_batch_is_ignored_outside_device_decode(tmp_path, net):
    from cutie_amd.eval_vos import process_video
    root = str(tmp_path)
    _make_video(root, 'vA', n=3, ids=(1, 2), seed=21)
    JpegBatchMock.reset()
    with torch.inference_mode():
        for ingest in ('host', 'device'):
            rd = next(iter(_dataset(root, ingest=ingest).get_datasets()))
            assert process_video(net, default_config(mem_every=2), rd, os.path.join(root, ingest), decode_batch=4)['frames'] == 3
    assert not JpegBatchMock.batch_ops and _pngs(os.path.join(root, 'device')) == _pngs(os.path.join(root, 'host'))
    with pytest.raises(ValueError, match='decode_batch'):
        process_video(net, default_config(), next(iter(_dataset(root).get_datasets())), os.path.join(root, 'x'), decode_batch=0)
