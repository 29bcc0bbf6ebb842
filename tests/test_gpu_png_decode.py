"""The PNG decode stages on the GPU (RESIZE flags 64 / 128, csrc/png_dec.hip): every corpus file (tests/png_corpus.py) equals PIL's bytes, one
at a time and as ONE batch of all files in a single launch per stage, between guard bytes; the status blocks equal the model's
(tests/png_dec_ref.py); the corrupt set raises the model's error bits -- error handling in bounded time, as for JPEG: every corrupt packet has
been through the kernel's serial core under the sanitizers on the CPU first (test_png_decode_cpu.py); and the three consumers --
SequenceScorer(gt_decode='device'), score_masks --decode device, eval_vos --score --gt-decode device -- give the host mode's results."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_corpus as C            # noqa: E402
import png_dec_ref as R           # noqa: E402

from cutie_amd import _lib                                                   # noqa: E402
from cutie_amd.config import default_config                                 # noqa: E402
from cutie_amd.inference.data import device_ingest as DI, png_packet as P   # noqa: E402
from cutie_amd.inference.utils import davis_metrics as M                    # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64


@pytest.fixture(scope='module')
def corpus():
    """[(name, packet, PIL's array, the model's status)] -- built once, shared, left alone."""
    _lib.set_executor_for_testing(None)
    before = sum(P.fallbacks.values())
    out = []
    for name, data in C.accepted(os.path.join(HERE, 'golden')):
        pkt, why = P.parse(data, name)
        assert pkt is not None, (name, why)
        out.append((name, pkt, np.array(Image.open(io.BytesIO(data))), R.decode(pkt)[1]))
    assert sum(P.fallbacks.values()) == before and len(out) > 80
    return out


@pytest.fixture(scope='module')
def corrupt():
    return [(name, P.parse(data, name)[0], bit) for name, data, bit in C.corrupt()]


def _whole(t):
    """The whole output buffer behind a decoded view."""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def _check_guards(views, packets):
    buf = _whole(views[0]).cpu().numpy()
    keep = np.ones(buf.size, dtype=bool)
    base = views[0].data_ptr() - views[0].storage_offset()
    for v, pk in zip(views, packets):
        o = v.data_ptr() - base
        keep[o:o + pk.nbytes_out] = False
    assert keep.sum() >= GUARD * (len(views) + 1) and bool((buf[keep] == 0xA5).all())


def test_every_file_alone(corpus):
    for name, pkt, ref, status in corpus:
        (got,), chk = DI.png_to_device([pkt], 'cuda', check=False, guard=GUARD)
        chk()
        assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape, name
        assert np.array_equal(got.cpu().numpy(), ref), name
        assert chk.status.numpy()[0].tolist() == status, (name, chk.status.numpy()[0].tolist(), status)
        _check_guards([got], [pkt])


def test_all_files_in_one_launch(corpus):
    packets = [c[1] for c in corpus]
    assert len({c[2].shape for c in corpus}) > 20 and {int(p.hdr[P.HDR_DEPTH]) for p in packets} == {1, 2, 4, 8}      # sizes and depths mixed
    views, chk = DI.png_to_device(packets, 'cuda', check=False, guard=GUARD)
    chk()
    st = chk.status.numpy()
    for k, (name, pkt, ref, status) in enumerate(corpus):
        assert np.array_equal(views[k].cpu().numpy(), ref), name
        assert st[k].tolist() == status, (name, st[k].tolist(), status)
    _check_guards(views, packets)


def test_corrupt_set_raises_the_models_bits(corpus, corrupt):
    good = next(c for c in corpus if c[0] == 'golden/bike/00000.png')
    for name, pkt, bit in corrupt:
        want = R.decode(pkt)[1]
        assert want[0] == bit
        views, chk = DI.png_to_device([good[1], pkt, good[1]], 'cuda', names=['a', name, 'b'], check=False, guard=GUARD)
        with pytest.raises(ValueError, match=name):
            chk()
        st = chk.status.numpy()
        assert st[1].tolist() == want, (name, st[1].tolist(), want)
        assert st[0].tolist() == st[2].tolist() == good[3]
        for k in (0, 2):                                          # a good image next to a bad one is still right
            assert np.array_equal(views[k].cpu().numpy(), good[2]), name
        _check_guards(views, [good[1], pkt, good[1]])
    with pytest.raises(ValueError, match='cut_half'):             # check=True waits and raises by itself
        DI.png_to_device([good[1], corrupt[1][1]], 'cuda', names=['x', 'somewhere/cut_half.png'])


def test_bad_header_and_table(corpus):
    from cutie_amd import ops as O
    good = corpus[0]
    bad = np.array(good[1].buf)
    bad[4 * P.HDR_STREAM:4 * P.HDR_STREAM + 4] = np.frombuffer(np.int32(1 << 20).tobytes(), dtype=np.uint8)     # a stream longer than the buffer
    views, chk = DI.png_to_device([good[1], P.Packet(bad, good[1].shape, 'bad')], 'cuda', check=False)
    with pytest.raises(ValueError, match='bad'):
        chk()
    assert chk.status.numpy()[1].tolist() == [R.E_HEADER, 0, 0, 0] and chk.status.numpy()[0].tolist() == good[3]
    assert np.array_equal(views[0].cpu().numpy(), good[2])
    # table entries that point outside the buffers
    pkt = good[1]
    table, pb, ib, ob = O.OpList.png_layout([pkt] * 3)
    table[1, 1] = ib                                              # inflated rows behind the inflate buffer
    table[2, 2] = ob - 1                                          # pixels run past the output
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    blob = np.zeros(pb, dtype=np.uint8)
    for k in range(3):
        blob[table[k, 0]:table[k, 0] + pkt.buf.nbytes] = pkt.buf
    packets, tab = dev(blob), dev(table)
    infl, out = torch.zeros(ib, dtype=torch.uint8, device='cuda'), torch.full((ob,), 0xA5, dtype=torch.uint8, device='cuda')
    status = torch.full((3, 4), -1, dtype=torch.int32, device='cuda')
    ol = O.OpList()
    ol.png_inflate(packets, tab, infl, status, n=3)
    ol.png_unfilter(packets, tab, infl, out, status, n=3)
    ol.run()
    st = status.cpu().numpy()
    assert st[0].tolist() == good[3] and st[1, 0] == R.E_HEADER and st[2, 0] == R.E_HEADER
    assert np.array_equal(out[:pkt.nbytes_out].cpu().numpy().reshape(pkt.shape), good[2]) and bool((out[table[1, 2]:] == 0xA5).all())
    lib = _lib.load()
    for flags, msg in ((64 | 4, 'cannot be combined'), (64 | 8, 'cannot be combined')):
        arr = ol.arr[:1].copy()
        arr['flags'][0] = flags
        assert lib.cutie_exec(arr.ctypes.data, 1, None) != 0 and msg in lib.cutie_hip_last_error().decode()


# ---- consumers -----------------------------------------------------------------------------------------------------------------------------
def _blob(H, W, t, k):
    yy, xx = np.mgrid[:H, :W]
    return ((yy - (30 + 6 * t + 20 * k)) ** 2 + (xx - (40 + 9 * t + 30 * k)) ** 2) < (14 + 3 * k) ** 2


@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    """3 videos x 6 frames of 96 x 136, written with PIL: JPEGImages, GT (moving discs), Annotations (frame 0 = GT) and Pred (GT shifted)."""
    root = str(tmp_path_factory.mktemp('pngdec'))
    H, W = 96, 136
    rng = np.random.default_rng(3)
    pal = bytes(rng.integers(0, 256, 768, dtype=np.uint8))
    for v in range(3):
        name = f'vid{v}'
        for d in ('JPEGImages', 'GT', 'Annotations', 'Pred'):
            os.makedirs(os.path.join(root, d, name))
        for t in range(6):
            ids = np.zeros((H, W), dtype=np.uint8)
            for k in range(v + 1):
                ids[_blob(H, W, t, k)] = k + 1
            img = np.clip(rng.integers(90, 130, (H, W, 3)) + ids[..., None] * 40, 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, 'JPEGImages', name, f'{t:05d}.jpg'), quality=92)
            for d, arr in (('GT', ids), ('Pred', np.roll(ids, (1 + t % 2, 2), (0, 1)))) + ((('Annotations', ids),) if t == 0 else ()):
                im = Image.fromarray(arr)
                im.putpalette(pal)
                im.save(os.path.join(root, d, name, f'{t:05d}.png'))
    return root


def _read(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith('.csv') or f == 'scores.json'}


def test_sequence_scorer_gt_decode_device(folders):
    gt, pred = os.path.join(folders, 'GT'), os.path.join(folders, 'Pred')
    for v in range(3):
        tables = {}
        for mode in ('host', 'device'):
            sc = M.SequenceScorer(gt, f'vid{v}', 'cuda', gt_decode=mode)
            for t in range(6):
                ids = torch.from_numpy(np.array(Image.open(os.path.join(pred, f'vid{v}', f'{t:05d}.png')))).cuda()
                sc.add(f'{t:05d}.png', ids)
            res = sc.finish()
            tables[mode] = (sc.table.cpu().numpy().copy(), res)
            assert sc.gt_fallbacks == {} and sc.gt_device_frames == (6 if mode == 'device' else 0)
        assert tables['host'][0].shape == (6, v + 1, 8) and tables['host'][0][:, :, 7].min() > 0
        assert np.array_equal(tables['host'][0], tables['device'][0]) and tables['host'][1] == tables['device'][1]
    with pytest.raises(ValueError):
        M.SequenceScorer(gt, 'vid0', 'cuda', gt_decode='gpu')


def test_sequence_scorer_declined_and_corrupt_ground_truth(folders, tmp_path):
    import shutil
    # a frame the parser declines (a real Adam7 file, which PIL reads) takes the host route, is counted, and scores as in host mode
    lace = str(tmp_path / 'lace')
    os.makedirs(os.path.join(lace, 'v'))
    rng = np.random.default_rng(9)
    for t in range(3):
        ids = C.mask(96, 136, 20 + t)
        with open(os.path.join(lace, 'v', f'{t:05d}.png'), 'wb') as f:
            f.write(C.interlaced_file(ids))
        assert np.array_equal(np.array(Image.open(os.path.join(lace, 'v', f'{t:05d}.png'))), ids)
    pred = torch.from_numpy(C.mask(96, 136, 30)).cuda()
    tables = {}
    for mode in ('host', 'device'):
        sc = M.SequenceScorer(lace, 'v', 'cuda', gt_decode=mode, skip_first_last=False)
        for t in range(3):
            sc.add(f'{t:05d}.png', pred)
        tables[mode] = sc.finish()
        assert sc.gt_fallbacks == ({'interlaced': 3} if mode == 'device' else {}) and sc.gt_device_frames == 0
    assert tables['host'] == tables['device'] and tables['host'] is not None
    # mode L at 8 bits is accepted; a corrupt stream in a fine container is a ValueError with the file's name, in finish at the latest
    gt = str(tmp_path / 'GT')
    shutil.copytree(os.path.join(folders, 'GT', 'vid1'), os.path.join(gt, 'vid1'))
    f2 = os.path.join(gt, 'vid1', '00002.png')
    Image.fromarray(np.array(Image.open(f2))).save(f2)
    assert Image.open(f2).mode == 'L'
    load = lambda t: torch.from_numpy(np.array(Image.open(os.path.join(folders, 'Pred', 'vid1', f'{t:05d}.png')))).cuda()       # noqa: E731
    sc = M.SequenceScorer(gt, 'vid1', 'cuda', gt_decode='device')
    sc.add('00001.png', load(1))
    sc.add('00002.png', load(2))
    assert sc.gt_fallbacks == {} and sc.gt_device_frames == 2
    f4 = os.path.join(gt, 'vid1', '00004.png')
    pkt = P.parse_file(f4)[0]
    stream = pkt.buf[P.HDR_BYTES:].tobytes()
    with open(f4, 'wb') as f:
        f.write(C.png_file(136, 96, int(pkt.hdr[P.HDR_DEPTH]), 3, stream[:len(stream) // 2]))
    sc.add('00004.png', load(4))
    with pytest.raises(ValueError, match='00004.png'):
        sc.finish()


def test_score_folders_decode_device(folders, tmp_path):
    from cutie_amd import score_masks as S
    gt, pred = os.path.join(folders, 'GT'), os.path.join(folders, 'Pred')
    outs = {}
    for mode in ('host', 'device'):
        out = str(tmp_path / mode)
        glob, per = S.score_folders(pred, gt, dataset='syn', output=out, decode=mode)
        outs[mode] = (_read(out), glob, per)
    assert len(outs['host'][0]) == 3 and outs['host'][0] == outs['device'][0] and outs['host'][1:] == outs['device'][1:]
    assert sorted(outs['host'][2]) == ['vid0', 'vid1', 'vid2'] and all(len(v['frames']) == 4 for v in outs['host'][2].values())
    assert S.decode_fallbacks == {}
    S.DECODE_BATCH, keep = 4, S.DECODE_BATCH                      # batches that do not divide the video
    try:
        out = str(tmp_path / 'all')
        S.score_folders(pred, gt, dataset='syn', output=out, decode='device', score_all_frames=True)
        S.score_folders(pred, gt, dataset='syn', output=out + '_host', score_all_frames=True)
        assert _read(out) == _read(out + '_host')
    finally:
        S.DECODE_BATCH = keep
    assert S.arg_parser().parse_args(['--results', 'a', '--gt', 'b', '--decode', 'device']).decode == 'device'


def test_eval_vos_score_gt_decode_device(folders):
    from cutie_amd import eval_vos as E
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(S.decisive_state_dict())
    res = {}
    for mode in ('host', 'device'):
        out = os.path.join(folders, 'out_' + mode)
        ap = E.arg_parser()
        args = ap.parse_args(['--images', os.path.join(folders, 'JPEGImages'), '--masks', os.path.join(folders, 'Annotations'), '--gt',
                              os.path.join(folders, 'GT'), '--output', out, '--dataset', 'd17-val', '--score', '--egress', 'device',
                              '--gt-decode', mode])
        E.check_args(ap, args)
        run = E.run_dataset(net, default_config(), args)
        assert all(r['frames'] == 6 and r['scores'] is not None for r in run.values())
        res[mode] = _read(out)
    assert len(res['host']) == 3 and res['host'] == res['device']
    assert len(json.loads(res['device']['scores.json'])['sequences']) == 3
