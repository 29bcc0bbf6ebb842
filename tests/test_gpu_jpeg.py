"""GPU JPEG decode on the MI355X (RESIZE flags 8 / 16 / 32, jpeg.hip, ABI 6): every stage against the integer reference
(tests/jpeg_ref.py) with guard bytes around every buffer, the whole decode byte-identical to PIL on the corpus (1080p included), the
error word on truncated and corrupt data, and the eval drivers end to end in the three ingest modes."""
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.inference.data import jpeg as J
from oracle.weights import make_state_dict

import jpeg_corpus
import jpeg_ref

pytestmark = pytest.mark.gpu
GUARD = 4096
SENT = {torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A}


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _guarded(n, dtype):
    """Device buffer of n elements with GUARD sentinel elements on each side (8-byte aligned view) -> (buffer, view)."""
    buf = torch.full((2 * GUARD + n,), SENT[dtype], dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, dtype):
    return bool((buf[:GUARD] == SENT[dtype]).all()) and bool((buf[-GUARD:] == SENT[dtype]).all())


def _decode(data, *, rounds=O.JPEG_SYNC_ROUNDS, chunk_bits=J.CHUNK_BITS):
    """The three stages on guarded buffers, each checked against the reference; -> (rgb uint8 [H, W, 3], status, coef error bits)."""
    pkt, why = J.parse(data, chunk_bits)
    assert pkt is not None, why
    sz = J.stage_sizes(pkt, rounds)
    H, W = pkt.shape
    bufs = {k: _guarded(sz[k], dt) for k, dt in (('coef', torch.int16), ('planes', torch.uint8), ('work', torch.int32), ('rgb', torch.uint8))}
    sbuf, status = _guarded(4, torch.int32)
    pbuf, dpkt = _guarded(pkt.buf.nbytes, torch.uint8)
    dpkt.copy_(torch.from_numpy(pkt.buf))
    ref = (pkt, dpkt)
    coef, planes, rgb = bufs['coef'][1], bufs['planes'][1], bufs['rgb'][1]
    for stage in range(3):
        ol = O.OpList(prio=False)
        if stage == 0:
            ol.jpeg_huff(ref, work=bufs['work'][1], coef=coef, status=status, rounds=rounds)
        elif stage == 1:
            ol.jpeg_idct(ref, coef=coef, planes=planes)
        else:
            ol.jpeg_color(ref, planes=planes, rgb=rgb)
        ol.finalize()
        ol.run()
        torch.cuda.synchronize()
        if stage == 0:
            st = status.cpu().numpy().copy()
            if st[0]:
                break
            want, err = jpeg_ref.huff(pkt.buf)
            assert err == 0
            assert np.array_equal(coef.cpu().numpy().reshape(-1, 64), want), 'Huffman stage differs from the reference'
        elif stage == 1:
            assert np.array_equal(planes.cpu().numpy(), jpeg_ref.idct(pkt.buf, want)), 'IDCT stage differs from the reference'
    for k, (buf, _) in bufs.items():
        assert _intact(buf, buf.dtype), f'write outside {k}'
    assert _intact(sbuf, torch.int32) and _intact(pbuf, torch.uint8)
    return rgb.view(H, W, 3).cpu().numpy(), st


def _whole(data):
    """Decode without the per-stage reference (large frames): -> (rgb, status)."""
    pkt, why = J.parse(data)
    assert pkt is not None, why
    from cutie_amd.inference.data.device_ingest import jpeg_buffers
    b = jpeg_buffers(pkt, 'cuda')
    dpkt = b['pkt'][:pkt.buf.nbytes]
    dpkt.copy_(torch.from_numpy(pkt.buf))
    ol = O.OpList(prio=False)
    ol.jpeg_huff((pkt, dpkt), work=b['work'], coef=b['coef'], status=b['status'])
    ol.jpeg_idct((pkt, dpkt), coef=b['coef'], planes=b['planes'])
    ol.jpeg_color((pkt, dpkt), planes=b['planes'], rgb=b['rgb'])
    ol.finalize()
    ol.run()
    torch.cuda.synchronize()
    return b['rgb'].cpu().numpy().copy(), b['status'].cpu().numpy().copy()


SMALL = jpeg_corpus.corpus(large=False)


@pytest.mark.parametrize('case', SMALL, ids=[n for n, _ in SMALL])
def test_stages_match_reference_and_pil(case):
    name, data = case
    rgb, st = _decode(data)
    assert st[0] == 0, (name, st)
    pil = jpeg_corpus.pil_rgb(data)
    assert np.array_equal(rgb, pil), (name, int((rgb != pil).sum()))


def test_whole_corpus_is_pil_bytes():
    """Every corpus file, 720p and 1080p included, byte-identical to PIL; sync statistics printed."""
    worst_rounds, serial = 0, 0
    for name, data in jpeg_corpus.corpus(large=True):
        rgb, st = _whole(data)
        assert st[0] == 0, (name, st)
        pil = jpeg_corpus.pil_rgb(data)
        assert rgb.shape == pil.shape and np.array_equal(rgb, pil), (name, int((rgb != pil).sum()))
        worst_rounds, serial = max(worst_rounds, int(st[1])), serial + int(st[2])
    print(f'corpus: max sync rounds {worst_rounds}, serial segments {serial}')


@pytest.mark.parametrize('chunk_bits,rounds', [(64, 0), (64, 1), (256, 2), (4096, 3)])
def test_speculation_never_changes_the_result(chunk_bits, rounds):
    """Tiny chunks and no sync rounds force the serial completion; every setting gives the same bytes."""
    data = jpeg_corpus.encode(jpeg_corpus.image('synthetic', 96, 136, 2), quality=90, subsampling=2)
    rgb, st = _decode(data, rounds=rounds, chunk_bits=chunk_bits)
    assert st[0] == 0 and np.array_equal(rgb, jpeg_corpus.pil_rgb(data))
    if rounds == 0:
        assert st[2] >= 1                                          # every segment with more than one chunk is finished serially


def test_truncated_and_corrupt_data_set_the_error_word():
    data = jpeg_corpus.encode(jpeg_corpus.image('noise', 64, 96, 3), quality=90, subsampling=2)
    pkt, _ = J.parse(data)
    sos = data.index(b'\xff\xda')
    cut = data[:sos + (len(data) - sos) // 2]                      # half the entropy data, no EOI
    _, st = _decode(cut)
    assert st[0] & jpeg_ref.ERR_TRUNC, st
    bad = bytearray(data)
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], 'big')
    bad[start + 10:start + 40] = b'\xff\x00' * 15                   # 240 one bits: no Huffman code is all ones
    _, st = _decode(bytes(bad))
    assert st[0] != 0, st


def test_to_device_raises_on_a_bad_frame(tmp_path):
    from cutie_amd.inference.data.device_ingest import jpeg_to_device
    data = jpeg_corpus.encode(jpeg_corpus.image('noise', 64, 96, 3), quality=90)
    pkt, _ = J.parse(data[:len(data) // 2])
    with pytest.raises(ValueError, match='x.jpg'):
        jpeg_to_device(pkt, 'cuda', name='x.jpg')
    pkt, _ = J.parse(data)
    out = jpeg_to_device(pkt, 'cuda', (32, 48))
    torch.cuda.synchronize()
    assert out.shape == (3, 32, 48) and out.is_contiguous()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
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


def test_bike_three_modes_write_the_same_pngs(gpu_net, tmp_path):
    from cutie_amd.eval_vos import process_video
    from cutie_amd.inference.data.video_reader import VideoReader
    src = os.path.join(os.path.dirname(__file__), 'golden', 'bike')
    img_dir, msk_dir = os.path.join(tmp_path, 'JPEGImages', 'bike'), os.path.join(tmp_path, 'Annotations', 'bike')
    os.makedirs(img_dir); os.makedirs(msk_dir)
    for f in sorted(os.listdir(src)):
        shutil.copy(os.path.join(src, f), img_dir if f.endswith('.jpg') else msk_dir)
    cfg = default_config()
    with torch.inference_mode():
        for mode in ('host', 'device', 'device-decode'):
            rd = VideoReader('bike', img_dir, msk_dir, ingest=mode)
            r = process_video(gpu_net, cfg, rd, os.path.join(tmp_path, mode), dataset='d17-val')
            assert r['frames'] == len(rd)
            if mode == 'device-decode':
                assert sum(rd.decode_fallbacks.values()) == 0
    host = _bytes(os.path.join(tmp_path, 'host'))
    assert len(host) == len(os.listdir(img_dir))
    assert _bytes(os.path.join(tmp_path, 'device')) == host
    assert _bytes(os.path.join(tmp_path, 'device-decode')) == host


def test_720p_size_480_device_decode_equals_device(tmp_path):
    """--size 480 on 1280 x 720 frames: 'device-decode' PNGs are byte-identical to 'device' PNGs, with process_video and in lock step."""
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    from cutie_amd.eval_vos import lockstep_key, process_video, process_videos_lockstep
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from test_gpu_ingest import _make_720p_video
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(S.decisive_state_dict())
    root = str(tmp_path)
    _make_720p_video(root, 'vA', 6, (1, 2), 41)
    _make_720p_video(root, 'vB', 6, (3, 7), 42)
    rds = {m: list(VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False, size=480,
                                  ingest=m).get_datasets()) for m in ('device', 'device-decode')}
    assert [lockstep_key(r) for r in rds['device']] == [lockstep_key(r) for r in rds['device-decode']] == [((480, 853), 2, False)] * 2
    cfg = default_config(mem_every=3)
    with torch.inference_mode():
        for m in rds:
            for rd in rds[m]:
                process_video(net, cfg, rd, os.path.join(root, 'alone_' + m))
            process_videos_lockstep(net, cfg, rds[m], os.path.join(root, 'ls_' + m))
    torch.cuda.synchronize()
    dev = _bytes(os.path.join(root, 'alone_device'))
    assert len(dev) == 12
    assert _bytes(os.path.join(root, 'alone_device-decode')) == dev
    assert _bytes(os.path.join(root, 'ls_device-decode')) == _bytes(os.path.join(root, 'ls_device'))


def test_clips_in_flight_decode_in_their_own_buffers(gpu_net, tmp_path):
    """--clips-in-flight: parallel.run_concurrent runs process_video on 2 host threads and streams; clips of the same frame size decode at
    the same time and write the same PNGs as 'host' run one clip after another."""
    from cutie_amd.eval_vos import process_video
    from cutie_amd.parallel import run_concurrent
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from test_ingest_cpu import _make_video
    root = str(tmp_path)
    for k in range(4):
        _make_video(root, f'v{k}', n=6, h=120, w=200, ids=(1, 2), seed=50 + k)
    cfg = default_config(mem_every=2)
    out = {}
    with torch.inference_mode():
        for mode in ('host', 'device-decode'):
            rds = list(VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False,
                                      ingest=mode).get_datasets())
            if mode == 'host':
                for rd in rds:
                    process_video(gpu_net, cfg, rd, os.path.join(root, mode))
            else:
                run_concurrent(gpu_net, range(len(rds)), lambda view, c: process_video(view, cfg, rds[c], os.path.join(root, mode)),
                               streams=2)
            out[mode] = _bytes(os.path.join(root, mode))
    torch.cuda.synchronize()
    assert len(out['host']) == 24 and out['device-decode'] == out['host']
