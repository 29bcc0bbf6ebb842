"""The device overlay of --visualize without a GPU (PROB_TO_ID flags == 128, ABI 11): the numpy model of the stage (tests/jpeg_enc_ref.py)
writes PIL's bytes, the container and the blend are the host path's, and saver and driver -- run through the model -- write the host
overlay's files."""
import io
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_enc_ref as R                                   # noqa: E402
import png_ref                                             # noqa: E402
from mock_exec import F32, I32, U8, view                   # noqa: E402
from test_ingest_cpu import IngestMock, _dataset, _make_video      # noqa: E402

from cutie_amd import _lib, ops as O                       # noqa: E402
from cutie_amd.config import default_config               # noqa: E402
from cutie_amd.inference.utils import jpeg_writer as JW    # noqa: E402
from cutie_amd.inference.utils import results_utils as RU  # noqa: E402
from oracle.weights import make_state_dict                 # noqa: E402

SIZES = [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (21, 37), (24, 40), (33, 47)]     # odd block counts in one or both directions


def pil_bytes(a, quality=None):
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', **({} if quality is None else {'quality': quality}))
    return b.getvalue()


def content(kind, H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    if kind == 'noise':
        return np.random.RandomState(seed + H * 1000 + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == 'smooth':
        return np.stack([(y * 3 + x) % 256, (x * 5) % 256, (y + x * 2) % 256], -1).astype(np.uint8)
    if kind == 'flat':
        return np.full((H, W, 3), (200, 30, 90), np.uint8)
    if kind == 'stripes':        # horizontal stripes at the highest vertical frequency of a block: one coefficient at zigzag 35, a run of 34
        row = np.round(128 + 100 * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)).astype(np.uint8)
        return np.repeat(row[..., None], 3, -1)
    raise KeyError(kind)


# ---- the model against PIL ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['noise', 'smooth', 'flat'])
@pytest.mark.parametrize('H,W', SIZES, ids=lambda v: str(v))
def test_model_writes_pils_file(H, W, kind):
    a = content(kind, H, W)
    qt = JW.quant_tables(75)
    assert JW.wrap(R.encode(a, qt=qt), H, W, qt) == pil_bytes(a)             # (PIL's default: quality 75, 4:2:0)
    assert JW.wrap(R.encode(a, qt=qt), H, W, qt) == pil_bytes(a, 75)


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
@pytest.mark.parametrize('quality', [30, 100])
def test_model_at_other_qualities(quality, kind):
    a = content(kind, 21, 37)
    qt = JW.quant_tables(quality)
    assert JW.wrap(R.encode(a, qt=qt), 21, 37, qt) == pil_bytes(a, quality)


def test_model_codes_long_zero_runs():
    a = content('stripes', 33, 47)
    qt = JW.quant_tables(30)
    assert R.has_zrl(a, qt)
    assert JW.wrap(R.encode(a, qt=qt), 33, 47, qt) == pil_bytes(a, 30)


def test_model_blend_is_the_host_paths_float_expression():
    rs = np.random.RandomState(3)
    image_np = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    out_mask = rs.choice(np.array([0, 1, 3, 7, 200], dtype=np.uint8), size=(37, 53))     # 7 and 200 are not objects
    all_obj_ids, colors = [1, 3], RU.davis_palette_np
    rgb_mask = np.zeros((*out_mask.shape, 3), dtype=np.uint8)                # results_utils.py _writer, the host overlay
    for oid in all_obj_ids:
        rgb_mask[out_mask == oid] = colors[oid % len(colors)]
    alpha = ((out_mask == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
    want = (image_np * alpha + rgb_mask * (1 - alpha)).astype(np.uint8)
    tab = JW.color_table(colors, all_obj_ids)
    assert tab.shape == (256, 4) and not tab[7].any() and not tab[200].any() and tab[3, :3].tolist() == colors[3].tolist()
    got = R.blend(image_np, out_mask, tab)
    assert np.array_equal(got, want)
    assert (got[out_mask == 7] == image_np[out_mask == 7] >> 1).all()         # an id that is not an object: black, still halved
    assert np.array_equal(R.blend(image_np, None, None), image_np)


@pytest.mark.parametrize('quality', [75, 40])
@pytest.mark.parametrize('H,W', [(21, 37), (480, 854)], ids=lambda v: str(v))
def test_header_is_pils(H, W, quality):
    ref = pil_bytes(content('smooth', H, W), quality)
    hdr = JW.header(H, W, JW.quant_tables(quality))
    assert len(hdr) == JW.HEADER_BYTES == 623 and hdr == ref[:623]
    assert ref.endswith(b'\xff\xd9') and JW.wrap(b'ab', H, W, JW.quant_tables(quality)) == hdr + b'ab\xff\xd9'


def test_descriptor_of_jpeg_encode():
    """The slots sit where include/cutie_hip.h says (PROB_TO_ID, ABI 11)."""
    H, W = 21, 37
    big = torch.zeros((H, 40, 3), dtype=torch.uint8)
    frame = big[:, :W]                                                        # a padded row stride
    ids, colors = torch.zeros((H, W), dtype=torch.uint8), torch.zeros((256, 4), dtype=torch.uint8)
    qt = torch.from_numpy(JW.quant_tables().view(np.int16))
    stream = torch.empty(O.OpList.jpeg_enc_capacity(H, W), dtype=torch.uint8)
    status, scratch = torch.empty(4, dtype=torch.int32), torch.empty(O.OpList.jpeg_enc_scratch_words(H, W), dtype=torch.int32)
    ol = O.OpList()
    ol.jpeg_encode(frame, ids, colors, qt, stream, status, scratch, H=H, W=W)
    ol.jpeg_encode(frame, None, None, qt, stream, status, scratch, H=H, W=W)
    recs = ol.finalize()
    for rec, with_ids in zip(recs, (True, False)):
        assert rec['kind'] == O.PROB_TO_ID and rec['flags'] == 128
        i, p = rec['i'], [int(v) for v in rec['p']]
        assert (i[1], i[2], i[4], i[7], i[8]) == (H, W, 120, stream.numel(), scratch.numel()) and i[0] == i[3] == i[5] == i[6] == 0 and not i[9:].any()
        assert p[0] == frame.data_ptr() and p[1] == 0 and p[3] == stream.data_ptr() and p[4] == status.data_ptr() and p[5] == scratch.data_ptr()
        assert p[2] == (ids.data_ptr() if with_ids else 0) and p[6] == (colors.data_ptr() if with_ids else 0) and p[7] == qt.data_ptr()
        assert not any(p[8:])
    B = 6 * 2 * 3
    assert O.OpList.jpeg_enc_blocks(H, W) == B
    U = 52 * B + 16
    assert O.OpList.jpeg_enc_scratch_words(H, W) == 16 + 32 * B + 4 * B + U + 4 * -(-U // 16)
    assert O.OpList.jpeg_enc_capacity(H, W, worst=True) == 2 * -(-1660 * B // 8) >= O.OpList.jpeg_enc_capacity(H, W)
    assert O.OpList.jpeg_enc_capacity(480, 854) == 1024 + 480 * 854 * 3 // 2
    with pytest.raises(ValueError):
        ol.jpeg_encode(frame.float(), None, None, qt, stream, status, scratch, H=H, W=W)
    with pytest.raises(ValueError):
        ol.jpeg_encode(frame, ids[:, :5], colors, qt, stream, status, scratch, H=H, W=W)
    with pytest.raises(ValueError):
        ol.jpeg_encode(frame, ids, None, qt, stream, status, scratch, H=H, W=W)
    assert len(ol) == 2 and _lib.ABI_VERSION == 11


# ---- saver modes ------------------------------------------------------------------------------------------------------------------
def _saver(tmp_path, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    om = ObjectManager()
    om.add_new_objects([5, 3])
    if kw.pop('with_processor', True):
        kw['processor'] = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om)
    kw.setdefault('use_long_id', False)
    return RU.ResultSaver(str(tmp_path), 'vid', dataset='generic', object_manager=om, visualize_output_root=str(tmp_path / 'vis'), **kw)


def test_saver_modes(tmp_path):
    assert RU.OVERLAY_MODES == ('host', 'device')
    for kw, want in ((dict(visualize=True, overlay='device', egress='device'), ('device', 'device')),
                     (dict(visualize=True, overlay='device', egress='host'), ('host', 'device')),
                     (dict(visualize=True, overlay='host', egress='device'), ('host', 'host')),        # today's fall-back
                     (dict(visualize=True, egress='device'), ('host', 'host')),
                     (dict(visualize=False, overlay='device', egress='device'), ('device', 'host')),
                     (dict(visualize=True, overlay='device', egress='device', use_long_id=True), ('host', 'host'))):
        s = _saver(tmp_path, **kw)
        try:
            assert (s.egress, s.overlay) == want, kw
        finally:
            s.end()
    with pytest.raises(ValueError, match='processor'):
        _saver(tmp_path, visualize=True, overlay='device', with_processor=False)
    with pytest.raises(ValueError, match='overlay'):
        _saver(tmp_path, visualize=True, overlay='gpu')


def test_eval_vos_parses_overlay(capsys):
    from cutie_amd.eval_vos import arg_parser
    base = ['--images', 'i', '--masks', 'm', '--output', 'o']
    assert arg_parser().parse_args(base).overlay == 'host'
    assert arg_parser().parse_args(base + ['--visualize', '--overlay', 'device']).overlay == 'device'
    with pytest.raises(SystemExit):
        arg_parser().parse_args(base + ['--overlay', 'gpu'])
    capsys.readouterr()


# ---- saver and driver through the model -----------------------------------------------------------------------------------------------
class OverlayMock(IngestMock):
    """The interpreter with the egress stages of PROB_TO_ID served from their models: flags&4 (resampled argmax), flags&8 (PNG stream,
    tests/png_ref.py); flags == 128 goes to jpeg_enc_ref.EncodeExecutor, which wraps this."""

    def _op_36(self, flags, i, f, p):
        if not flags & 12:
            return super()._op_36(flags, i, f, p)
        assert not flags & ~12
        P, H, W, plane, ldrow = i[:5]
        prob = view(p[0], F32, (P, H, W), (plane, ldrow, 1)).clone()
        OH, OW = (i[5], i[6]) if flags & 4 else (H, W)
        if flags & 4 and (OH, OW) != (H, W):
            prob = F.interpolate(prob.unsqueeze(1), (OH, OW), mode='bilinear', align_corners=False)[:, 0]
        ids = view(p[1], I32, (P,)).long()[prob.argmax(0)].to(torch.uint8)
        view(p[2], U8, (OH, OW)).copy_(ids)
        if flags & 8:
            data, adler = png_ref.encode(ids.numpy())
            fits = len(data) <= i[7]
            view(p[4], I32, (4,)).copy_(torch.tensor([len(data), adler - (1 << 32) if adler >= 1 << 31 else adler, 0 if fits else 1, 0], dtype=torch.int32))
            if fits:
                view(p[3], U8, (len(data),)).copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))


@pytest.fixture(scope='module')
def overlay_net():
    from cutie_amd.model.cutie import CUTIE
    mx = OverlayMock()
    mx.per_sample_conv = True
    ex = R.EncodeExecutor(mx)
    _lib.set_executor_for_testing(ex)
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net, ex
    _lib.set_executor_for_testing(None)


def _files(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), 'rb').read()
    return out


def _decoded(files):
    return {k: np.array(Image.open(io.BytesIO(v))).tolist() for k, v in files.items()}


@pytest.fixture(scope='module')
def video(tmp_path_factory, overlay_net):
    """A 4-frame video and what the host overlay writes for it (once)."""
    from cutie_amd.eval_vos import process_video
    net, _ = overlay_net
    root = str(tmp_path_factory.mktemp('overlay'))
    _make_video(root, 'vA', n=4, ids=(1, 2), seed=21)
    cfg = default_config(mem_every=2)
    with torch.inference_mode():
        rd = next(iter(_dataset(root).get_datasets()))
        process_video(net, cfg, rd, os.path.join(root, 'host', 'm'), visualize=True, visualize_output_root=os.path.join(root, 'host', 'v'))
    host = (_files(os.path.join(root, 'host', 'm')), _files(os.path.join(root, 'host', 'v')))
    assert len(host[0]) == 4 and sorted(host[1]) == [f'vA/{t:05d}.jpg' for t in range(4)]
    return root, cfg, host


@pytest.mark.parametrize('ingest', [None, 'device'])
@pytest.mark.parametrize('egress', ['host', 'device'])
def test_driver_device_overlay_writes_the_host_files(video, overlay_net, egress, ingest):
    from cutie_amd.eval_vos import process_video
    net, ex = overlay_net
    root, cfg, (host_masks, host_jpgs) = video
    out = os.path.join(root, f'dev_{egress}_{ingest}')
    calls = ex.calls
    with torch.inference_mode():
        rd = next(iter(_dataset(root).get_datasets()))
        r = process_video(net, cfg, rd, os.path.join(out, 'm'), visualize=True, visualize_output_root=os.path.join(out, 'v'),
                          overlay='device', egress=egress, ingest=ingest)
    assert r['frames'] == 4 and ex.calls == calls + 4
    assert _files(os.path.join(out, 'v')) == host_jpgs                       # the same .jpg BYTES
    masks = _files(os.path.join(out, 'm'))
    if egress == 'host':
        assert masks == host_masks
    else:                                                                     # the device PNG path: the same images, other bytes
        assert _decoded(masks) == _decoded(host_masks) and masks != host_masks


def test_overflow_falls_back_to_the_host_encoder(video, overlay_net, monkeypatch, caplog):
    from cutie_amd.eval_vos import process_video
    net, ex = overlay_net
    root, cfg, (host_masks, host_jpgs) = video
    monkeypatch.setattr(O.OpList, 'jpeg_enc_capacity', classmethod(lambda cls, H, W, worst=False: 64))
    for egress in ('host', 'device'):
        out = os.path.join(root, f'tiny_{egress}')
        caplog.clear()
        with caplog.at_level(logging.WARNING), torch.inference_mode():
            rd = next(iter(_dataset(root).get_datasets()))
            process_video(net, cfg, rd, os.path.join(out, 'm'), visualize=True, visualize_output_root=os.path.join(out, 'v'),
                          overlay='device', egress=egress, ingest='device')
        assert _files(os.path.join(out, 'v')) == host_jpgs
        assert _decoded(_files(os.path.join(out, 'm'))) == _decoded(host_masks)
        warned = [r for r in caplog.records if r.levelno >= logging.WARNING]
        assert len(warned) == 1 and 'device JPEG encoder' in warned[0].getMessage()
