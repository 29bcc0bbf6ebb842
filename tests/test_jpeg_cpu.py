"""GPU JPEG decode on CPU: the host parser (cutie_amd/inference/data/jpeg.py) and the integer reference (tests/jpeg_ref.py) against
PIL's Image.open(...).convert('RGB') byte for byte, the fallback of the files the GPU decoder does not take, and the 'device-decode'
ingest mode through the drivers under the torch interpreter with the RESIZE flags 8 / 16 / 32 run by the reference: its records and
PNGs equal those of 'host' and 'device'."""
import ctypes
import io
import os
import time

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
from test_ingest_cpu import IngestMock, _dataset, _make_video, _pngs


def _host(ptr, dtype, n):
    """numpy array of n elements aliasing host memory at ptr."""
    dt = np.dtype(dtype)
    return np.frombuffer((ctypes.c_char * (n * dt.itemsize)).from_address(int(ptr)), dtype=dt)


class JpegMock(IngestMock):
    """The interpreter with the JPEG stages of RESIZE (flags 8 / 16 / 32) run by the integer reference."""
    calls = 0

    def _op_37(self, flags, i, f, p):
        if not flags & 56:
            return super()._op_37(flags, i, f, p)
        assert not flags & 7
        JpegMock.calls += 1
        buf = _host(p[0], np.uint8, i[5]).copy()
        h = buf[:J.HDR_WORDS * 4].view(np.int32)
        nblock, H, W = int(h[J.HDR_NBLOCK]), int(h[J.HDR_H]), int(h[J.HDR_W])
        assert (i[2], i[7], i[8]) == (nblock, H, W)
        if flags & 8:
            coef, err = jpeg_ref.huff(buf)
            _host(p[2], np.int16, nblock * 64)[:] = coef.reshape(-1)
            _host(p[3], np.int32, 4)[:] = (err, 1, 0, 0)
        if flags & 16:
            coef = _host(p[2], np.int16, nblock * 64).reshape(nblock, 64)
            _host(p[4], np.uint8, i[6])[:] = jpeg_ref.idct(buf, coef)
        if flags & 32:
            rgb = jpeg_ref.color(buf, _host(p[4], np.uint8, i[6]))
            out = _host(p[5], np.uint8, (H - 1) * i[11] + 3 * W)
            for y in range(H):
                out[y * i[11]:y * i[11] + 3 * W] = rgb[y].reshape(-1)


@pytest.fixture
def jpeg_exec():
    _lib.set_executor_for_testing(JpegMock())
    yield
    _lib.set_executor_for_testing(None)


# ---- parser + reference against PIL ----------------------------------------------------------------------------------------------------
CORPUS = jpeg_corpus.corpus(large=False)


@pytest.mark.parametrize('case', CORPUS, ids=[n for n, _ in CORPUS])
def test_reference_is_pil(case):
    name, data = case
    pkt, why = J.parse(data)
    assert pkt is not None, why
    got = jpeg_ref.decode(pkt.buf)
    want = jpeg_corpus.pil_rgb(data)
    assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_reference_is_pil_at_1080p():
    data = jpeg_corpus.encode(jpeg_corpus.image('synthetic', 1080, 1920, 11), quality=95, subsampling=2)
    pkt, why = J.parse(data)
    assert np.array_equal(jpeg_ref.decode(pkt.buf), jpeg_corpus.pil_rgb(data))


def test_every_stage_is_libjpeg_not_a_lookalike():
    """The reference is not interchangeable with a near miss: replicated chroma with float colour conversion changes PIL's bytes on a
    4:2:0 frame, and the IDCT range limit wraps as libjpeg's table does."""
    data = jpeg_corpus.encode(jpeg_corpus.image('noise', 48, 64, 1), quality=90, subsampling=2)
    pkt, _ = J.parse(data)
    want = jpeg_corpus.pil_rgb(data)
    planes = jpeg_ref.idct(pkt.buf, jpeg_ref.huff(pkt.buf)[0])
    assert np.array_equal(jpeg_ref.color(pkt.buf, planes), want)
    Y = jpeg_ref._plane(pkt.buf, planes, 0)[:48, :64].astype(np.float64)
    cb = np.repeat(np.repeat(jpeg_ref._plane(pkt.buf, planes, 1), 2, 0), 2, 1)[:48, :64] - 128.0
    cr = np.repeat(np.repeat(jpeg_ref._plane(pkt.buf, planes, 2), 2, 0), 2, 1)[:48, :64] - 128.0
    plain = np.clip(np.round(np.stack([Y + 1.402 * cr, Y - 0.344136 * cb - 0.714136 * cr, Y + 1.772 * cb], 2)), 0, 255)
    assert not np.array_equal(plain.astype(np.uint8), want)
    assert jpeg_ref.range_limit(np.array([-100, 300, 600])).tolist() == [28, 255, 0]       # (600: libjpeg's 10-bit wrap, not a clamp)


@pytest.mark.parametrize('kind', ['progressive', 'cmyk', 'not_jpeg', 'png', 'adobe_rgb', 'truncated_header'])
def test_unsupported_files_are_rejected_with_a_reason(kind):
    arr = jpeg_corpus.image('noise', 24, 40, 2)
    if kind == 'progressive':
        data, reason = jpeg_corpus.encode(arr, quality=90, progressive=True), 'progressive'
    elif kind == 'cmyk':
        b = io.BytesIO()
        Image.fromarray(arr).convert('CMYK').save(b, format='JPEG', quality=90)
        data, reason = b.getvalue(), 'CMYK'
    elif kind == 'not_jpeg':
        data, reason = b'hello world', 'not a JPEG'
    elif kind == 'png':
        b = io.BytesIO()
        Image.fromarray(arr).save(b, format='PNG')
        data, reason = b.getvalue(), 'not a JPEG'
    elif kind == 'adobe_rgb':
        b = io.BytesIO()
        Image.fromarray(arr).save(b, format='JPEG', quality=90, keep_rgb=True)
        data, reason = b.getvalue(), 'RGB'
    else:
        data, reason = jpeg_corpus.encode(arr, quality=90)[:100], 'truncated'
    pkt, why = J.parse(data)
    assert pkt is None and reason in why, why


def test_packet_geometry():
    data = jpeg_corpus.encode(jpeg_corpus.image('noise', 37, 53, 2), quality=90, subsampling=2, restart_marker_blocks=3)
    pkt, _ = J.parse(data, chunk_bits=256)
    h = pkt.hdr
    assert pkt.shape == (37, 53) and h[J.HDR_NCOMP] == 3 and h[J.HDR_BPM] == 6 and (h[J.HDR_HMAX], h[J.HDR_VMAX]) == (2, 2)
    assert h[J.HDR_MCUS_X] == 4 and h[J.HDR_NMCU] == 12 and h[J.HDR_NBLOCK] == 12 * 6 and h[J.HDR_NSEG] == 4
    assert pkt.buf.nbytes == h[J.HDR_BYTES] and h[J.HDR_OFF_DATA] % 4 == 0
    sz = J.stage_sizes(pkt, 3)
    assert sz['coef'] == 72 * 64 and sz['planes'] == 72 * 64 and sz['rgb'] == 37 * 53 * 3
    assert sz['work'] == 10 * int(h[J.HDR_NCHUNK]) + 4 * 4


def test_builders_fill_the_abi_fields():
    data = jpeg_corpus.encode(jpeg_corpus.image('noise', 16, 24, 2), quality=90)
    pkt, _ = J.parse(data)
    dev = torch.from_numpy(pkt.buf.copy())
    ol = O.OpList(prio=False)
    w, c, s, pl, rgb = (torch.zeros(k, dtype=torch.int32) for k in (64, 5, 4, 6, 7))
    ol.jpeg_huff((pkt, dev), work=w, coef=c, status=s, rounds=2)
    ol.jpeg_idct((pkt, dev), coef=c, planes=pl)
    ol.jpeg_color((pkt, dev), planes=pl, rgb=rgb)
    arr = ol.finalize()
    assert arr['kind'].tolist() == [O.RESIZE] * 3 and arr['flags'].tolist() == [8, 16, 32]
    h = pkt.hdr
    assert arr['i'][0, :12].tolist() == [h[J.HDR_NCHUNK], h[J.HDR_NSEG], h[J.HDR_NBLOCK], J.CHUNK_BITS, 2, pkt.buf.nbytes,
                                         h[J.HDR_PLANE_BYTES], 16, 24, 64, 3, 72]
    assert arr['p'][0, :4].tolist() == [dev.data_ptr(), w.data_ptr(), c.data_ptr(), s.data_ptr()]
    assert arr['p'][2, 4:6].tolist() == [pl.data_ptr(), rgb.data_ptr()]


def test_parse_cost():
    """Host cost of one parse (printed; the target is well under 0.5 ms for a 1080p frame)."""
    data = jpeg_corpus.encode(jpeg_corpus.image('synthetic', 1080, 1920, 1), quality=90)
    J.parse(data)
    t = time.perf_counter()
    for _ in range(20):
        pkt, _ = J.parse(data)
    ms = (time.perf_counter() - t) / 20 * 1e3
    print(f'parse 1080p ({len(data)} bytes): {ms:.3f} ms')
    assert pkt is not None and ms < 50


# ---- reader + drivers under the interpreter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [-1, 48])
def test_device_decode_records_equal_host_records(tmp_path, jpeg_exec, size):
    from cutie_amd.inference.data.device_ingest import to_device
    _make_video(str(tmp_path), 'v', n=3, h=64, w=96)
    host = next(iter(_dataset(str(tmp_path), size=size).get_datasets()))
    dec = next(iter(_dataset(str(tmp_path), size=size, ingest='device-decode').get_datasets()))
    assert dec.ingest == 'device-decode'
    JpegMock.calls = 0
    for t in range(len(host)):
        h, d = host[t], dec[t]
        assert 'rgb' not in d and 'rgb_u8' not in d and isinstance(d['jpeg'], J.Packet)
        assert d['info']['rgb_shape'] == tuple(h['rgb'].shape[-2:])
        d = to_device(d, 'cpu')
        assert set(d) == set(h) and d['info'] == h['info']
        assert d['rgb'].dtype == torch.float32 and d['rgb'].is_contiguous() and torch.equal(d['rgb'], h['rgb']), t
    assert JpegMock.calls == 3 * len(host) and sum(dec.decode_fallbacks.values()) == 0


def test_fallbacks_are_counted(tmp_path, jpeg_exec):
    from cutie_amd.inference.data.device_ingest import to_device
    _make_video(str(tmp_path), 'v', n=3, h=64, w=96)
    frame = os.path.join(str(tmp_path), 'JPEGImages', 'v', '00001.jpg')
    Image.open(frame).save(frame, format='JPEG', quality=95, progressive=True)
    host = next(iter(_dataset(str(tmp_path)).get_datasets()))
    dec = next(iter(_dataset(str(tmp_path), ingest='device-decode').get_datasets()))
    recs = [dec[t] for t in range(3)]
    assert ['jpeg' in r for r in recs] == [True, False, True] and 'rgb_u8' in recs[1]
    assert dict(dec.decode_fallbacks) == {'progressive': 1}
    for t, r in enumerate(recs):
        assert torch.equal(to_device(r, 'cpu')['rgb'], host[t]['rgb'])


def test_bad_frame_raises_with_its_name(tmp_path, jpeg_exec):
    from cutie_amd.inference.data.device_ingest import to_device
    _make_video(str(tmp_path), 'v', n=2, h=64, w=96)
    frame = os.path.join(str(tmp_path), 'JPEGImages', 'v', '00001.jpg')
    data = open(frame, 'rb').read()
    open(frame, 'wb').write(data[:len(data) * 2 // 3])
    dec = next(iter(_dataset(str(tmp_path), ingest='device-decode').get_datasets()))
    r = dec[1]
    assert 'jpeg' in r
    with pytest.raises(ValueError, match='00001.jpg'):
        to_device(r, 'cpu')


def test_lockstep_key_is_the_same_in_every_mode(tmp_path):
    from cutie_amd.eval_vos import lockstep_key
    _make_video(str(tmp_path), 'a', n=2, h=64, w=96, ids=(1, 3))
    _make_video(str(tmp_path), 'b', n=2, h=80, w=60, ids=(2,))
    for size in (-1, 48):
        keys = {m: [lockstep_key(rd) for rd in _dataset(str(tmp_path), size=size, ingest=m).get_datasets()]
                for m in ('host', 'device', 'device-decode')}
        assert keys['host'] == keys['device'] == keys['device-decode']


@pytest.fixture(scope='module')
def jpeg_net():
    from cutie_amd.model.cutie import CUTIE
    mx = JpegMock()
    mx.per_sample_conv = True
    _lib.set_executor_for_testing(mx)
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net
    _lib.set_executor_for_testing(None)


@pytest.mark.parametrize('size', [-1, 48])
def test_eval_driver_device_decode_writes_the_host_pngs(tmp_path, jpeg_net, size):
    from cutie_amd.eval_vos import process_video, process_videos_lockstep
    root = str(tmp_path)
    _make_video(root, 'vA', n=4, ids=(1, 2), seed=21)
    _make_video(root, 'vB', n=3, ids=(4, 9), seed=22)
    cfg = default_config(mem_every=2)
    with torch.inference_mode():
        for mode in ('host', 'device', 'device-decode'):
            rds = list(_dataset(root, size=size, ingest=mode).get_datasets())
            for rd in rds:
                assert process_video(jpeg_net, cfg, rd, os.path.join(root, 'alone_' + mode))['frames'] == len(rd)
            process_videos_lockstep(jpeg_net, cfg, rds, os.path.join(root, 'ls_' + mode))
    host = _pngs(os.path.join(root, 'alone_host'))
    assert len(host) == 7
    for mode in ('device', 'device-decode'):
        assert _pngs(os.path.join(root, 'alone_' + mode)) == host
        assert _pngs(os.path.join(root, 'ls_' + mode)) == _pngs(os.path.join(root, 'ls_host'))


def test_process_video_device_decode_writes_the_host_pngs(tmp_path, jpeg_net):
    from cutie_amd.process_video import process_video, video_config
    from cutie_amd.inference.utils.results_utils import davis_palette
    from cutie_amd.utils.synth import SyntheticClip
    root = str(tmp_path)
    clip = SyntheticClip(64, 96, 2, 4, seed=5)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(4):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(clip.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    cfg = video_config(mem_every=2)
    out = {}
    for mode in ('host', 'device-decode'):
        r = process_video(jpeg_net, cfg, os.path.join(root, 'frames'), os.path.join(root, 'masks'), os.path.join(root, mode), ingest=mode)
        assert r['frames'] == 4
        out[mode] = _pngs(os.path.join(root, mode))
    assert len(out['host']) == 4 and out['device-decode'] == out['host']


# ---- libjpeg's table checks, the table cache ----------------------------------------------------------------------------------------
def test_tables_libjpeg_refuses_are_refused():
    """jpeg_make_d_derived_tbl: no code may be all ones (code >= 1 << length after a length), no DC symbol above 15."""
    assert J.huff_table(bytes([2] + [0] * 15), bytes([0, 1])) is None                     # codes 0 and 1 of length 1: '1' is all ones
    assert J.huff_table(bytes([1, 1] + [0] * 14), bytes([0, 1])) is not None              # 0, 10
    assert J.huff_table(bytes([0, 3] + [0] * 14), bytes([0, 1, 2])) is not None
    assert J.huff_table(bytes([0, 4] + [0] * 14), bytes([0, 1, 2, 3])) is None
    assert J.huff_table(bytes([0, 2] + [0] * 14), bytes([3, 16]), dc=True) is None
    assert J.huff_table(bytes([0, 2] + [0] * 14), bytes([3, 16]), dc=False) is not None
    data = bytearray(jpeg_corpus.extremes())
    i = data.index(b'\xff\xc4') + 5 + 16                                                  # the DC table's first symbol
    data[i] = 16
    pkt, why = J.parse(bytes(data))
    assert pkt is None and 'DHT' in why
    with pytest.raises(Exception):
        jpeg_corpus.pil_rgb(bytes(data))                                                  # (PIL refuses it too)


def test_extremes_decode_as_libjpeg():
    """DC categories 12 and 13, AC runs past index 63: decoded as PIL decodes them, not refused."""
    data = jpeg_corpus.extremes()
    pkt, why = J.parse(data)
    coef, err = jpeg_ref.huff(pkt.buf)
    assert err == 0 and coef[:, 0].tolist() == [2500, 50, -4050, 100] and coef[1, 63] == 27
    assert np.array_equal(jpeg_ref.decode(pkt.buf), jpeg_corpus.pil_rgb(data))
    coef[1, 63] = 0                                                                      # the store at 63 shows in the pixels
    assert not np.array_equal(jpeg_ref.color(pkt.buf, jpeg_ref.idct(pkt.buf, coef)), jpeg_corpus.pil_rgb(data))


def test_huffman_table_cache_is_bounded():
    J._huff_cache.clear()
    for k in range(J.HUFF_CACHE_SIZE + 40):
        counts = bytes([0] * (8 + k // 256) + [1] + [0] * (7 - k // 256))                 # one code of length 9 or 10
        assert J.huff_table(counts, bytes([k % 256])) is not None
    assert len(J._huff_cache) == J.HUFF_CACHE_SIZE
    J._huff_cache.clear()


# ---- deferred checks, names, several clips at once --------------------------------------------------------------------------------
@pytest.fixture
def mock_net(jpeg_net):
    """jpeg_net with its interpreter installed for this test (a function-scoped jpeg_exec before it may have removed it)."""
    before = _lib._executor
    mx = JpegMock()
    mx.per_sample_conv = True
    _lib.set_executor_for_testing(mx)
    yield jpeg_net
    _lib.set_executor_for_testing(before)


def _truncate(path):
    data = open(path, 'rb').read()
    open(path, 'wb').write(data[:len(data) * 2 // 3])


def test_deferred_check_raises_in_finish(tmp_path, jpeg_exec):
    from cutie_amd.inference.data.device_ingest import finish, to_device
    _make_video(str(tmp_path), 'v', n=2, h=64, w=96)
    _truncate(os.path.join(str(tmp_path), 'JPEGImages', 'v', '00001.jpg'))
    host = next(iter(_dataset(str(tmp_path)).get_datasets()))
    dec = next(iter(_dataset(str(tmp_path), ingest='device-decode').get_datasets()))
    good = to_device(dec[0], 'cpu', defer_check=True)
    assert 'decode_check' in good
    good = finish(good)
    assert 'decode_check' not in good and torch.equal(good['rgb'], host[0]['rgb'])
    bad = to_device(dec[1], 'cpu', defer_check=True)                                     # no error yet
    with pytest.raises(ValueError, match='00001.jpg'):
        finish(bad)


def test_eval_driver_raises_on_a_bad_frame(tmp_path, mock_net):
    jpeg_net = mock_net
    from cutie_amd.eval_vos import process_video
    root = str(tmp_path)
    _make_video(root, 'v', n=4, ids=(1, 2), seed=21)
    _truncate(os.path.join(root, 'JPEGImages', 'v', '00002.jpg'))
    rd = next(iter(_dataset(root, ingest='device-decode').get_datasets()))
    with torch.inference_mode(), pytest.raises(ValueError, match='00002.jpg'):
        process_video(jpeg_net, default_config(mem_every=2), rd, os.path.join(root, 'out'))


def test_process_video_error_names_the_file(tmp_path, mock_net):
    jpeg_net = mock_net
    from cutie_amd.process_video import process_video, video_config
    from cutie_amd.inference.utils.results_utils import davis_palette
    from cutie_amd.utils.synth import SyntheticClip
    root = str(tmp_path)
    clip = SyntheticClip(64, 96, 2, 3, seed=5)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(3):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(clip.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))
    _truncate(os.path.join(root, 'frames', '0000002.jpg'))
    with pytest.raises(ValueError, match='0000002.jpg'):
        process_video(jpeg_net, video_config(mem_every=2), os.path.join(root, 'frames'), os.path.join(root, 'masks'),
                      os.path.join(root, 'out'), ingest='device-decode')


def test_clips_in_flight_device_decode_writes_the_host_pngs(tmp_path, mock_net):
    """parallel.run_concurrent (one host thread per clip in flight) in 'device-decode': clips of the same frame size decode at the same
    time, each into its own buffers, and write the PNGs of 'host'."""
    from cutie_amd.eval_vos import process_video
    from cutie_amd.parallel import run_concurrent
    root = str(tmp_path)
    for k in range(4):
        _make_video(root, f'v{k}', n=3, ids=(1, 2), seed=30 + k)
    cfg = default_config(mem_every=2)
    out = {}
    for mode, streams in (('host', 1), ('device-decode', 2)):
        rds = list(_dataset(root, size=48, ingest=mode).get_datasets())
        run_concurrent(mock_net, range(len(rds)), lambda view, c: process_video(view, cfg, rds[c], os.path.join(root, mode)),
                       streams=streams)
        out[mode] = _pngs(os.path.join(root, mode))
    assert len(out['host']) == 12 and out['device-decode'] == out['host']
