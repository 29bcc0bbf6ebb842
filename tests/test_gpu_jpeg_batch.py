"""The batch forms of the GPU JPEG decode on the MI355X (RESIZE flags 8 / 16 / 32 with 256, jpeg.hip): the small corpus in ONE batch
against PIL and against the one-frame launches of the same packets, with guard bytes around every image's regions; batch order and
size, forced serial completion, errors that stay with their image, the table / header check, and the eval drivers with
``decode_batch`` 4 against 1."""
import os
import shutil

import numpy as np
import pytest
import torch

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.data import jpeg as J
from oracle.weights import make_state_dict

import jpeg_corpus
import jpeg_ref

pytestmark = pytest.mark.gpu
GUARD = 4096
ERR_TABLE = 4
SMALL = jpeg_corpus.corpus(large=False)


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _parse(data, **kw):
    pkt, why = J.parse(data, **kw)
    assert pkt is not None, why
    return pkt


def _one_frame(pkt, rounds=O.JPEG_SYNC_ROUNDS):
    """The one-frame launches of a packet -> coef, planes, rgb (numpy), status."""
    from cutie_amd.inference.data.device_ingest import jpeg_buffers
    b = jpeg_buffers(pkt, 'cuda', rounds)
    ref = (pkt, b['pkt'])
    ol = O.OpList(prio=False)
    ol.jpeg_huff(ref, work=b['work'], coef=b['coef'], status=b['status'], rounds=rounds)
    ol.jpeg_idct(ref, coef=b['coef'], planes=b['planes'])
    ol.jpeg_color(ref, planes=b['planes'], rgb=b['rgb'])
    ol.finalize()
    ol.run()
    torch.cuda.synchronize()
    return {k: b[k].cpu().numpy().copy() for k in ('coef', 'planes', 'rgb', 'status')}


def _batch(pkts, rounds=O.JPEG_SYNC_ROUNDS, patch=None):
    """The three batch stages over ``pkts`` in buffers filled with 0xA5, GUARD bytes around every image's coef, planes and rgb ->
    per image {coef, planes, rgb, status} (numpy).  Asserts that no byte outside the images' own regions changed.
    patch(blob, table): changes the packet bytes after the layout was made (a header that disagrees with its row)."""
    n = len(pkts)
    table, sz = O.OpList.jpeg_layout(pkts, rounds=rounds, guard=GUARD)
    blob = np.zeros(sz['packets'], dtype=np.uint8)
    for k, p in enumerate(pkts):
        blob[table[k, 0]:table[k, 0] + p.buf.nbytes] = p.buf
    if patch is not None:
        patch(blob, table)
    dev = {'packets': torch.from_numpy(blob).cuda(), 'table': torch.from_numpy(table).cuda(),
           'work': torch.empty(sz['work'], dtype=torch.int32, device='cuda'),
           'coef': torch.full((sz['coef'],), -0x5A5B, dtype=torch.int16, device='cuda'),           # the bytes 0xA5 0xA5
           'planes': torch.full((sz['planes'],), 0xA5, dtype=torch.uint8, device='cuda'),
           'rgb': torch.full((sz['rgb'],), 0xA5, dtype=torch.uint8, device='cuda'),
           'status': torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device='cuda')}
    ol = O.OpList(prio=False)
    ol.jpeg_huff_batch(dev['packets'], dev['table'], sz, dev['status'], n=n, work=dev['work'], coef=dev['coef'])
    ol.jpeg_idct_batch(dev['packets'], dev['table'], sz, dev['status'], n=n, coef=dev['coef'], planes=dev['planes'])
    ol.jpeg_color_batch(dev['packets'], dev['table'], sz, dev['status'], n=n, planes=dev['planes'], rgb=dev['rgb'])
    ol.finalize()
    ol.run()
    torch.cuda.synchronize()
    host = {k: dev[k].cpu().numpy() for k in ('coef', 'planes', 'rgb', 'status')}
    out = []
    outside = {k: np.ones(host[k].shape, dtype=bool) for k in ('coef', 'planes', 'rgb')}
    for k, p in enumerate(pkts):
        own = J.stage_sizes(p, rounds)
        res = {'status': host['status'][k].copy()}
        for col, name in ((2, 'coef'), (3, 'planes'), (4, 'rgb')):
            o = int(table[k, col])
            res[name] = host[name][o:o + own[name]].copy()
            outside[name][o:o + own[name]] = False
        res['rgb'] = res['rgb'].reshape(p.shape + (3,))
        out.append(res)
    assert (host['coef'][outside['coef']] == -0x5A5B).all(), 'write outside the images in coef'
    assert (host['planes'][outside['planes']] == 0xA5).all(), 'write outside the images in planes'
    assert (host['rgb'][outside['rgb']] == 0xA5).all(), 'write outside the images in rgb'
    assert outside['coef'].sum() >= n * GUARD and outside['rgb'].sum() >= 2 * n * GUARD
    return out


@pytest.fixture(scope='module')
def corpus():
    """The small corpus parsed once, with PIL's bytes and the one-frame launches of every packet."""
    _lib.set_executor_for_testing(None)
    pkts = [_parse(d) for _, d in SMALL]
    return {'names': [n for n, _ in SMALL], 'pkts': pkts, 'pil': [jpeg_corpus.pil_rgb(d) for _, d in SMALL],
            'one': [_one_frame(p) for p in pkts]}


@pytest.fixture(scope='module')
def whole(corpus):
    return _batch(corpus['pkts'])


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ('coef', 'planes', 'rgb')) and a['status'][0] == b['status'][0]


def test_the_corpus_in_one_batch(corpus, whole):
    assert len(whole) == 61
    for name, pkt, pil, one, got in zip(corpus['names'], corpus['pkts'], corpus['pil'], corpus['one'], whole):
        st = got['status']
        assert st[0] == 0, (name, st)
        # (the rounds used and the serial count are not compared: a thread racing with a continuation may store a stale exit)
        assert 1 <= st[1] <= O.JPEG_SYNC_ROUNDS + 1 and 0 <= st[2] <= pkt.hdr[J.HDR_NSEG] and st[3] == 0, (name, st)
        assert np.array_equal(got['rgb'], pil), (name, int((got['rgb'] != pil).sum()))
        assert np.array_equal(got['coef'], one['coef']), name
        assert np.array_equal(got['planes'], one['planes']), name


def test_order_and_batch_size_do_not_matter(corpus, whole):
    rev = _batch(corpus['pkts'][::-1])[::-1]
    for name, a, b in zip(corpus['names'], whole, rev):
        assert _same(a, b), name
    for k in (0, 17, 60):
        assert _same(_batch([corpus['pkts'][k]])[0], whole[k]), corpus['names'][k]


def test_every_segment_through_the_serial_finish(corpus):
    """chunk_bits = 64 and no sync rounds: every segment of every image is decoded by one thread; the same bytes."""
    pick = [k for k, n in enumerate(corpus['names']) if any(s in n for s in ('_1x1_', '_7x13_', '_17x9_')) or n == 'restart_rows_33x47_L']
    assert len(pick) >= 20
    pkts = [_parse(SMALL[k][1], chunk_bits=64) for k in pick]
    got = _batch(pkts, rounds=0)
    chunks = 0
    for k, pkt, g in zip(pick, pkts, got):
        # (with no round every segment counts as not synchronised: rounds used = 0 + 1, serial segments = all)
        assert g['status'].tolist() == [0, 1, int(pkt.hdr[J.HDR_NSEG]), 0], (corpus['names'][k], g['status'])
        assert np.array_equal(g['rgb'], corpus['pil'][k]) and np.array_equal(g['coef'], corpus['one'][k]['coef']), corpus['names'][k]
        chunks += int(pkt.hdr[J.HDR_NCHUNK]) - int(pkt.hdr[J.HDR_NSEG])
    assert chunks > len(pick)                                                            # segments of several chunks are among them


def test_an_error_stays_with_its_image(corpus):
    small = [k for k, n in enumerate(corpus['names']) if '_17x9_' in n][:2]
    mid = [k for k, n in enumerate(corpus['names']) if n.startswith('gradient_120x160_420')][:3]
    order = [small[0], mid[0], small[1], mid[1], mid[2]]
    datas = [SMALL[k][1] for k in order]
    sos = datas[1].index(b'\xff\xda')
    datas[1] = datas[1][:sos + (len(datas[1]) - sos) // 2]                               # #1: half the entropy data, no EOI
    bad = bytearray(datas[3])
    sos = datas[3].index(b'\xff\xda')
    start = sos + 2 + int.from_bytes(datas[3][sos + 2:sos + 4], 'big')
    bad[start + 10:start + 40] = b'\xff\x00' * 15                                        # #3: 240 one bits: no code is all ones
    datas[3] = bytes(bad)
    pkts = [_parse(d) for d in datas]
    got = _batch(pkts)
    for j, (k, g) in enumerate(zip(order, got)):
        if j in (1, 3):
            want = _one_frame(pkts[j])['status'][0]
            assert want != 0 and g['status'][0] == want, (j, g['status'], want)
        else:
            assert g['status'][0] == 0 and np.array_equal(g['rgb'], corpus['pil'][k]), j
    assert got[1]['status'][0] & jpeg_ref.ERR_TRUNC


def test_a_header_that_asks_for_more_chunks_than_its_row_is_skipped(corpus):
    ks = [k for k, n in enumerate(corpus['names']) if n.startswith('gradient_120x160_420')][:2]
    pkts = [corpus['pkts'][ks[0]], corpus['pkts'][ks[1]], corpus['pkts'][ks[0]]]

    def patch(blob, table):
        hdr = blob[table[1, 0]:table[1, 0] + 4 * J.HDR_WORDS].view(np.int32)
        hdr[J.HDR_NCHUNK] += 3
    got = _batch(pkts, patch=patch)                                                      # (asserts the guards)
    assert got[1]['status'][0] == ERR_TABLE, got[1]['status']
    assert (got[1]['rgb'] == 0xA5).all() and (got[1]['planes'] == 0xA5).all() and (got[1]['coef'] == -0x5A5B).all()
    for j in (0, 2):
        assert got[j]['status'][0] == 0 and np.array_equal(got[j]['rgb'], corpus['pil'][ks[0]])


def test_jpegs_to_device_equals_jpeg_to_device(corpus):
    from cutie_amd.inference.data.device_ingest import jpeg_to_device, jpegs_to_device
    ks = [k for k, n in enumerate(corpus['names']) if '480x854' not in n][:12]
    pkts = [corpus['pkts'][k] for k in ks]
    sizes = [None if j % 2 else (max(1, p.shape[0] // 2), max(1, p.shape[1] // 2)) for j, p in enumerate(pkts)]
    frames, u8s = jpegs_to_device(pkts, 'cuda', sizes, keep_u8=True)
    for j, k in enumerate(ks):
        one = jpeg_to_device(pkts[j], 'cuda', sizes[j])
        assert frames[j].is_contiguous() and torch.equal(frames[j], one), corpus['names'][k]
        assert np.array_equal(u8s[j].cpu().numpy(), corpus['pil'][k])
    data = next(d for n, d in SMALL if n.startswith('gradient_120x160_420'))
    cut = _parse(data[:len(data) * 2 // 3])
    with pytest.raises(ValueError, match='^third: '):
        jpegs_to_device([pkts[0], pkts[1], cut], 'cuda', names=['first', 'second', 'third'])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.model.cutie import CUTIE
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


def _bytes(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), 'rb').read()
    return out


def test_bike_decode_batch_4_writes_the_pngs_of_1(gpu_net, tmp_path):
    from cutie_amd.eval_vos import process_video, process_videos_lockstep
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    src = os.path.join(os.path.dirname(__file__), 'golden', 'bike')
    root = str(tmp_path)
    for vid in ('bikeA', 'bikeB'):
        img_dir, msk_dir = os.path.join(root, 'JPEGImages', vid), os.path.join(root, 'Annotations', vid)
        os.makedirs(img_dir); os.makedirs(msk_dir)
        for f in sorted(os.listdir(src)):
            shutil.copy(os.path.join(src, f), img_dir if f.endswith('.jpg') else msk_dir)
    cfg = default_config()

    def readers():
        return list(VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False,
                                   ingest='device-decode').get_datasets())
    with torch.inference_mode():
        for B in (1, 4):
            rds = readers()
            r = process_video(gpu_net, cfg, rds[0], os.path.join(root, f'alone{B}'), dataset='d17-val', decode_batch=B)
            assert r['frames'] == len(rds[0]) and sum(rds[0].decode_fallbacks.values()) == 0
            process_videos_lockstep(gpu_net, cfg, readers(), os.path.join(root, f'ls{B}'), dataset='d17-val', decode_batch=B)
    torch.cuda.synchronize()
    alone = _bytes(os.path.join(root, 'alone1'))
    assert len(alone) == 4 and _bytes(os.path.join(root, 'alone4')) == alone
    ls = _bytes(os.path.join(root, 'ls1'))
    assert len(ls) == 8 and _bytes(os.path.join(root, 'ls4')) == ls
