"""Device egress without a GPU: the PNG container (cutie_amd/inference/utils/png.py), the numpy model of the device encoder
(tests/png_ref.py) against zlib's inflater and PIL's reader, and the ``egress`` argument of ResultSaver / eval_vos."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as R                                        # noqa: E402

from cutie_amd.inference.utils import png as C            # noqa: E402
from cutie_amd.inference.utils import results_utils as RU  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
CORPUS = R.corpus(GOLDEN)


def _chunks(data: bytes):
    assert data[:8] == C.SIGNATURE
    o, out = 8, []
    while o < len(data):
        n, kind = struct.unpack('>I', data[o:o + 4])[0], data[o + 4:o + 8]
        body, crc = data[o + 8:o + 8 + n], struct.unpack('>I', data[o + 8 + n:o + 12 + n])[0]
        assert crc == (zlib.crc32(kind + body) & 0xffffffff), kind
        out.append((kind, body))
        o += 12 + n
    assert o == len(data)
    return out


def _plane(seed=0, H=37, W=53):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 6, (5, 7), dtype=np.uint8), np.ones((8, 8), np.uint8))[:H, :W]


@pytest.mark.parametrize('palette', ['davis', 'short_list', 'bytes_5', None])
def test_assemble_around_a_zlib_stream(palette):
    ids = _plane()
    H, W = ids.shape
    pal = {'davis': RU.davis_palette, 'short_list': [0, 0, 0, 255, 0, 0, 0, 255, 0, 9, 9, 9, 1, 2, 3, 4, 5, 6, 7, 8, 9],
           'bytes_5': bytes(range(5)), None: None}[palette]
    data = C.assemble(zlib.compress(R.filtered(ids).tobytes()), H, W, pal)
    kinds = [k for k, _ in _chunks(data)]                  # (every CRC verified in there)
    assert kinds == ([b'IHDR', b'PLTE', b'IDAT', b'IEND'] if pal is not None else [b'IHDR', b'IDAT', b'IEND'])
    ihdr = dict(_chunks(data))[b'IHDR']
    assert struct.unpack('>IIBBBBB', ihdr) == (W, H, 8, 3 if pal is not None else 0, 0, 0, 0)
    im = Image.open(io.BytesIO(data))
    assert im.mode == ('P' if pal is not None else 'L')
    assert np.array_equal(np.array(im), ids)
    # what the host path stores: putpalette + PIL's own save
    ref = Image.fromarray(ids)
    if pal is not None:
        ref.putpalette(pal)
    buf = io.BytesIO()
    ref.save(buf, format='PNG')
    back = Image.open(io.BytesIO(buf.getvalue()))
    assert back.mode == im.mode and back.getpalette() == im.getpalette()
    if pal is not None:
        assert dict(_chunks(data))[b'PLTE'] == dict(_chunks(buf.getvalue()))[b'PLTE']
        n = max(min(len(bytes(pal)) // 3, 256), 1)
        assert dict(_chunks(data))[b'PLTE'][:len(bytes(pal)[:3 * n])] == bytes(pal)[:3 * n]


def test_assemble_rejects_an_empty_image():
    with pytest.raises(ValueError):
        C.assemble(b'', 0, 4, None)


def test_corpus_holds_the_golden_masks_and_the_edge_cases():
    assert sum(k.startswith('golden/') for k in CORPUS) >= 7
    for k in ('zeros', 'checker', 'w1', 'h1', 'one_pixel', 'row257_id0', 'row258_id5', 'row259_id0', 'row260_id0', 'row261_id5', 'row516_id0',
              'row517_id0', 'run259', 'run260', 'id143', 'id144', 'id255', 'noise4', 'noise256'):
        assert k in CORPUS, k


@pytest.mark.parametrize('name', sorted(CORPUS))
def test_model_stream_inflates_to_the_filtered_plane(name):
    ids = CORPUS[name]
    H, W = ids.shape
    stream, adler = R.encode(ids)
    R.check_stream(stream, ids)
    assert adler == (zlib.adler32(R.filtered(ids).tobytes()) & 0xffffffff)
    assert len(stream) <= R.capacity(H, W)
    for row in R.tokens(ids):
        assert R.token_bytes(row) == W + 1
        assert all(t[0] == 'lit' or 3 <= t[1] <= 258 for t in row)
    for pal in (RU.davis_palette, None):
        im = Image.open(io.BytesIO(C.assemble(stream, H, W, pal)))
        assert im.mode == ('P' if pal is not None else 'L') and np.array_equal(np.array(im), ids)
        if pal is not None:
            assert bytes(im.getpalette()) == RU.davis_palette


def test_capacity_is_the_products_and_is_reached_by_nine_bit_literals_only():
    from cutie_amd.ops import OpList
    for H, W in ((1, 1), (480, 854), (1080, 1920), (7, 33), (40, 66)):
        assert OpList.png_capacity(H, W) == R.capacity(H, W)
    ids = CORPUS['checker_hi']
    H, W = ids.shape
    stream, _ = R.encode(ids)
    assert len(stream) > (H * W * 9) // 8                  # ~9 bits per pixel: the worst case is real
    assert len(stream) <= R.capacity(H, W)


def test_long_runs_leave_no_short_rest():
    for n in (259, 260):
        toks = R.row_tokens(np.concatenate([[0, 4], np.full(n + 1, 9)]).astype(np.uint8), None)
        m = [t for t in toks if t[0] == 'match']
        assert [t[1] for t in m] == [n - 3, 3] and all(t[2] == 1 for t in m), toks      # the first 9 is a literal, the run behind it is n
    assert [R.take(n) for n in (3, 258, 259, 260, 261, 516, 517, 600)] == [3, 258, 256, 257, 258, 258, 258, 258]


def test_adler_partials_compose():
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 256, (23, 301), dtype=np.uint8)
    f = R.filtered(ids)
    assert R.adler_combine([R.adler_row_partials(r) for r in f], f.shape[1]) == (zlib.adler32(f.tobytes()) & 0xffffffff)


def test_golden_480p_masks_are_small():
    seen = 0
    for name, ids in CORPUS.items():
        if name.startswith('golden/') and ids.shape[0] == 480:
            seen += 1
            assert len(R.encode(ids)[0]) <= ids.size // 32, name
    assert seen >= 5


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
class _OM:
    tmp_id_to_obj, obj_to_tmp_id = {}, {}


def _saver(tmp_path, **kw):
    kw.setdefault('palette', RU.davis_palette)
    return RU.ResultSaver(str(tmp_path), 'v', dataset='d17-val', object_manager=_OM(), use_long_id=False, **kw)


def test_unknown_egress_raises(tmp_path):
    with pytest.raises(ValueError):
        _saver(tmp_path, egress='gpu')


def test_device_egress_needs_a_processor(tmp_path):
    with pytest.raises(ValueError):
        _saver(tmp_path, egress='device')


def test_host_egress_is_the_default_and_falls_back(tmp_path):
    s = _saver(tmp_path)
    assert s.egress == 'host'
    s.end()
    s = _saver(tmp_path, egress='host')
    assert s.egress == 'host' and s.queue.maxsize == 10
    s.end()
    proc = object()
    for kw in (dict(visualize=True, visualize_output_root=str(tmp_path), palette=list(RU.davis_palette)), dict(save_mask=False)):
        s = _saver(tmp_path, egress='device', processor=proc, **kw)
        assert s.egress == 'host'
        s.end()
    s = RU.ResultSaver(str(tmp_path), 'v', dataset='d17-val', object_manager=_OM(), use_long_id=True, processor=proc, egress='device')
    assert s.egress == 'host'
    s.end()
    s = _saver(tmp_path, egress='device', processor=proc)
    assert s.egress == 'device'
    s.end()


def test_eval_vos_parses_egress():
    from cutie_amd import eval_vos
    base = ['--images', 'a', '--masks', 'b', '--output', 'c']
    assert eval_vos.arg_parser().parse_args(base).egress == 'host'
    assert eval_vos.arg_parser().parse_args(base + ['--egress', 'device']).egress == 'device'
    with pytest.raises(SystemExit):
        eval_vos.arg_parser().parse_args(base + ['--egress', 'gpu'])
    import inspect
    for fn in (eval_vos.process_video, eval_vos.process_videos_lockstep):
        assert inspect.signature(fn).parameters['egress'].default == 'host'


def test_process_video_parses_egress():
    import inspect
    from cutie_amd import process_video as PV
    base = ['-v', 'a', '-m', 'b', '-o', 'c']
    assert PV.arg_parser().parse_args(base).egress == 'host'
    assert PV.arg_parser().parse_args(base + ['--egress', 'device']).egress == 'device'
    with pytest.raises(SystemExit):
        PV.arg_parser().parse_args(base + ['--egress', 'gpu'])
    assert inspect.signature(PV.process_video).parameters['egress'].default == 'host'
    assert PV.EGRESS_MODES is RU.EGRESS_MODES == ('host', 'device')


def test_host_egress_writes_what_it_wrote_before(tmp_path):
    """egress='host' through a saver without a processor: PIL's file, byte for byte."""
    import torch

    class Obj:
        def __init__(self, i):
            self.id = i
    om = _OM()
    om.tmp_id_to_obj = {1: Obj(3), 2: Obj(7)}
    om.obj_to_tmp_id = {Obj(3): 1, Obj(7): 2}
    prob = torch.rand(3, 20, 30, generator=torch.Generator().manual_seed(1))
    s = RU.ResultSaver(str(tmp_path), 'v', dataset='d17-val', object_manager=om, use_long_id=False, palette=RU.davis_palette, egress='host')
    s.process(prob, '00000.jpg')
    s.end()
    lut = np.array([0, 3, 7], np.uint8)
    ref = Image.fromarray(lut[prob.argmax(0).numpy()])
    ref.putpalette(RU.davis_palette)
    buf = io.BytesIO()
    ref.save(buf, format='PNG')
    assert open(os.path.join(str(tmp_path), 'v', '00000.png'), 'rb').read() == buf.getvalue()
