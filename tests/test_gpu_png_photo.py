"""The filtered, dynamic-Huffman PNG stage on the MI355X (PROB_TO_ID flags == 16384, csrc/png_photo.hip) against the model
(tests/png_photo_ref.py): the stream BYTE for byte and the status words over the whole corpus (tests/png_photo_corpus.py), between guard
bytes, the sources unchanged; the capacity error; the device's own decoder on the L and RGB items; the same bytes twice; the launcher's
refusals; and a saver run over three frames of the bike example with the cut-outs, the alpha matte and the dynamic codes switched on."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.inference.utils import png as PNG

import png_photo_corpus as C
import png_photo_ref as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
FILL = 0x5a


@pytest.fixture(autouse=True)
def hip_executor():
    _lib.set_executor_for_testing(None)
    yield


def _device(s0, s1, cap=None, pad=0):
    """the stage on one image -> (stream bytes as written, status, the whole stream buffer); every buffer sits between guards that must
    survive, the sources must come back unchanged.  ``pad``: bytes between the rows of the first source (a strided frame)."""
    H, W = s0.shape[:2]
    B = (3 if s0.ndim == 3 else 1) + (1 if s1 is not None else 0)
    rowbytes = W * (3 if s0.ndim == 3 else 1)
    room = torch.full((H, rowbytes + pad), 0xa5, dtype=torch.uint8, device='cuda')
    src = room[:, :rowbytes].view(H, W, 3) if s0.ndim == 3 else room[:, :rowbytes]
    src.copy_(torch.from_numpy(np.ascontiguousarray(s0)))
    last = torch.from_numpy(np.ascontiguousarray(s1)).cuda() if s1 is not None else None
    before = room.clone(), (last.clone() if last is not None else None)
    cap = O.OpList.png_photo_capacity(H, W, B) if cap is None else cap
    words = O.OpList.png_photo_scratch_words(H, W, B)
    obuf = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    sbuf = torch.full((4 * GUARD + 4 * words + 4 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    ubuf = torch.full((GUARD + 16 + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    assert obuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0 and ubuf.data_ptr() % 16 == 0
    ol = O.OpList()
    ol.png_photo(src, obuf[GUARD:GUARD + cap], ubuf[GUARD:GUARD + 16].view(torch.int32), sbuf[4 * GUARD:4 * GUARD + 4 * words].view(torch.int32),
                 last=last)
    ol.run()
    torch.cuda.synchronize()
    assert torch.equal(room, before[0]) and (last is None or torch.equal(last, before[1]))                  # read only
    for buf, lo, size in ((obuf, GUARD, cap), (sbuf, 4 * GUARD, 4 * words), (ubuf, GUARD, 16)):
        assert bool((buf[:lo] == FILL).all()) and bool((buf[lo + size:] == FILL).all())
    status = ubuf[GUARD:GUARD + 16].view(torch.int32).cpu().numpy()
    whole = obuf[GUARD:GUARD + cap].cpu().numpy()
    n = int(status[0]) if status[2] == 0 else 0
    return whole[:n].tobytes(), status, whole


def test_form_is_announced():
    lib = _lib.load()
    assert lib.cutie_hip_abi_version() == 11 == _lib.ABI_VERSION
    assert lib.cutie_hip_build_flags() & P.BUILD_BIT and _lib.has_png_photo()


@pytest.mark.parametrize('name', list(C.corpus()))
def test_bytes_equal_the_model(name):
    s0, s1 = C.corpus()[name]
    e = C.encoded(name)
    want_stream, want_status = P.stage(s0, s1, O.OpList.png_photo_capacity(e['H'], (e['L'] - 1) // e['B'], e['B']))
    got, status, whole = _device(s0, s1)
    print(name, 'bytes', len(got), 'model', len(want_stream), 'status', status.tolist())
    assert status.tolist() == want_status.tolist()
    if got != want_stream:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want_stream, np.uint8)
        m = min(len(a), len(b))
        assert False, (name, 'first difference at byte', int(np.flatnonzero(a[:m] != b[:m])[0]) if (a[:m] != b[:m]).any() else m, 'of', len(b))
    assert bool((whole[(len(got) + 3) // 4 * 4:] == FILL).all())                 # nothing behind the stream's last word


@pytest.mark.parametrize('name', ['bike_rgba', 'noise', 'blocks', '1x1'])
def test_capacity_one_byte_short(name):
    s0, s1 = C.corpus()[name]
    e = C.encoded(name)
    need = len(e['stream'])
    for cap in ((need + 3) // 4 * 4 - 4, 0):                                      # the capacity is rounded down to a multiple of 4: < need
        got, status, whole = _device(s0, s1, cap=cap)
        assert status.tolist()[:1] == [need] and status[2] == 1 and status[3] == 0
        assert bool((whole == FILL).all())                                        # nothing written
    got, status, _ = _device(s0, s1, cap=(need + 3) // 4 * 4)                     # exactly enough
    assert status[2] == 0 and got == e['stream']


@pytest.mark.parametrize('name', ['bike_rgba', 'blocks_la', 'fib'])
def test_same_bytes_twice_and_strided(name):
    s0, s1 = C.corpus()[name]
    a = _device(s0, s1)[0]
    b = _device(s0, s1, pad=13)[0]                                                # a frame with a row stride of its own
    assert a == b == C.encoded(name)['stream']


def test_device_decoder_returns_the_sources():
    """RESIZE flags 64 | 128 (csrc/png_dec.hip) inflates and unfilters the L and RGB files the encoder wrote."""
    from cutie_amd.inference.data import png_packet
    from cutie_amd.inference.data.device_ingest import png_to_device
    packets, wants = [], []
    for name, (s0, s1) in C.corpus().items():
        if s1 is not None:
            continue
        stream = _device(s0, None)[0]
        H, W = s0.shape[:2]
        pk, why = png_packet.parse(PNG.assemble_image(stream, H, W, 3 if s0.ndim == 3 else 1), name)
        assert pk is not None, (name, why)
        packets.append(pk)
        wants.append(s0)
    outs = png_to_device(packets, 'cuda')
    for pk, t, want in zip(packets, outs, wants):
        assert np.array_equal(t.cpu().numpy(), want), pk.source


def test_launcher_refuses():
    ex = _lib.get_executor()
    src = torch.zeros((4, 8), dtype=torch.uint8, device='cuda')
    cap, words = O.OpList.png_photo_capacity(4, 8, 1), O.OpList.png_photo_scratch_words(4, 8, 1)
    stream = torch.zeros(cap, dtype=torch.uint8, device='cuda')
    status = torch.zeros(4, dtype=torch.int32, device='cuda')
    scratch = torch.zeros(words, dtype=torch.int32, device='cuda')

    def run(ints, ptrs, flags=16384):
        ol = O.OpList()
        ol.add(O.PROB_TO_ID, flags, ints, [], ptrs)
        ol.run()

    good_i = [0, 4, 8, 1, 8, 0, 0, cap, words]
    good_p = [None, None, src, stream, status, scratch, None]
    run(good_i, good_p)
    torch.cuda.synchronize()
    assert status.cpu().tolist()[2] == 0

    def bad(match, i=None, p=None, flags=16384):
        with pytest.raises(Exception, match=match):
            run(good_i if i is None else i, good_p if p is None else p, flags)

    bad('unknown flags', flags=16384 | 8)
    bad('unknown flags', flags=16384 | 1)
    bad('H >= 1', i=[0, 0, 8, 1, 8, 0, 0, cap, words])
    bad('1 or 3 channels', i=[0, 4, 8, 2, 16, 0, 0, cap, words])
    bad('W \\* B \\+ 1', i=[0, 4, 16384, 1, 16384, 0, 0, cap, words])
    bad('row strides', i=[0, 4, 8, 1, 7, 0, 0, cap, words])
    bad('negative capacity', i=[0, 4, 8, 1, 8, 0, 0, -4, words])
    bad('scratch of', i=[0, 4, 8, 1, 8, 0, 0, cap, words - 1])
    bad('needs the source', p=[None, None, None, stream, status, scratch, None])
    bad('needs the source', p=[None, None, src, stream, None, scratch, None])
    bad('aligned', p=[None, None, src, stream[1:], status, scratch, None])
    bad('aligned', p=[None, None, src, stream, status, scratch[1:], None])
    torch.cuda.synchronize()


def test_saver_run_writes_cutouts(tmp_path):
    """Three frames of the bike example through a ResultSaver with cutout, alpha matte and dynamic codes: the cut-out's RGB is the frame,
    its A the alpha file of the same run; the soft-mask and alpha files hold the pixels of a run with the fixed codes."""
    import png_photo_saver_case as S
    S.run_and_check(str(tmp_path), device='cuda')
