"""The GPU PNG decode without a GPU: the container parser (cutie_amd/inference/data/png_packet.py), the packet layout, the Python model of
the kernels (tests/png_dec_ref.py) against zlib and PIL on the whole corpus (tests/png_corpus.py), the model's error bits on the corrupt
set, and the kernel's serial core (csrc/png_inflate_core.h) compiled as a host program under -fsanitize=address,undefined and run over the
same corpus -- the step that comes before the kernel sees a GPU."""
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_corpus as C            # noqa: E402
import png_dec_ref as R           # noqa: E402

from cutie_amd import ops as O                                   # noqa: E402
from cutie_amd.inference.data import png_packet as P            # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CSRC = os.path.join(ROOT, 'cutie_amd', 'csrc')


@pytest.fixture(scope='module')
def accepted():
    """[(name, file bytes, packet, PIL's array)] -- parsed once, shared and left alone."""
    out = []
    for name, data in C.accepted(GOLDEN):
        pkt, why = P.parse(data, name)
        assert pkt is not None, f'{name}: declined ({why}) -- every accepted-format file of the corpus must be taken'
        out.append((name, data, pkt, np.array(Image.open(io.BytesIO(data)))))
    return out


def test_corpus_covers_the_tables(accepted):
    names = [a[0] for a in accepted]
    assert len(set(names)) == len(names)
    for want in ('golden/judo/00000.png', 'golden/judo/00005.png', 'golden/bike/00000.png', 'own_device_stream', 'far_window_32768'):
        assert want in names
    assert sum(n.startswith('golden/io/video/Annotations') for n in names) >= 3
    by = {a[0]: a for a in accepted}
    assert by['stored_noise_300_two_idat'][1].count(b'IDAT') == 2                          # PIL cuts 90 KB into two chunks
    assert by['pil_default_3_colours'][2].hdr[P.HDR_DEPTH] == 2                            # PIL packs a 3-colour mask at 2 bits
    assert {tuple(a[3].shape[2:]) for a in accepted} == {(), (3,)}                         # planes and RGB
    judo = by['golden/judo/00000.png'][1]
    assert b'zTXt' in judo and b'iCCP' in judo and b'iTXt' in judo and judo.index(b'iTXt') < judo.index(b'PLTE')      # ancillary chunks first
    # PIL's own writer picks filters 0, 1, 2 and 4 for palette masks and never 3 (Average): filter 3 is covered by the hand-written files only
    seen = set()
    for name, data, pkt, ref in accepted:
        if name.startswith('pil_') and data[25] == 3:                                       # colour type 3
            raw = zlib.decompress(pkt.buf[P.HDR_BYTES:].tobytes())
            seen |= set(raw[::int(pkt.hdr[P.HDR_ROWBYTES]) + 1])
    assert seen == {0, 1, 2, 4}, seen
    forced = set()
    for name, data, pkt, ref in accepted:
        if name.startswith('filter'):
            raw = zlib.decompress(pkt.buf[P.HDR_BYTES:].tobytes())
            forced |= set(raw[::int(pkt.hdr[P.HDR_ROWBYTES]) + 1])
    assert forced == {0, 1, 2, 3, 4}


def test_parser_accepts_and_packet_layout(accepted):
    before = sum(P.fallbacks.values())
    for name, data, pkt, ref in accepted:
        assert pkt.shape == ref.shape, name
        h = pkt.hdr
        W, H, depth, ch, rb = (int(h[k]) for k in (P.HDR_W, P.HDR_H, P.HDR_DEPTH, P.HDR_CHANNELS, P.HDR_ROWBYTES))
        assert int(h[P.HDR_MAGIC]) == P.MAGIC == R.MAGIC and (H, W) == ref.shape[:2] and ch == (3 if ref.ndim == 3 else 1)
        assert rb == (W * ch * depth + 7) // 8 and int(h[P.HDR_INFLATED]) == H * (rb + 1) == pkt.inflated
        stream = pkt.buf[P.HDR_BYTES:].tobytes()
        assert int(h[P.HDR_STREAM]) == len(stream) and pkt.buf.dtype == np.uint8 and pkt.buf.nbytes == P.HDR_BYTES + len(stream)
        assert len(zlib.decompress(stream)) == pkt.inflated                                  # all IDAT chunks, in order, nothing else
        assert R.header(pkt.buf) is not None
    assert sum(P.fallbacks.values()) == before                                               # parse itself counts nothing


def test_parser_declines_with_reason():
    table = C.declined()
    assert {r for _, _, r in table} >= {'interlaced', '16 bits', 'alpha', 'grey below 8 bits', 'bad CRC', 'no IDAT', 'bad zlib header'}
    for name, data, reason in table:
        pkt, why = P.parse(data, name)
        assert pkt is None and why == reason, (name, why)
    assert P.parse(b'nothing', 'x') == (None, 'not a PNG')
    P.fallbacks.clear()
    P.count_fallback('alpha'), P.count_fallback('alpha'), P.count_fallback('interlaced')
    assert dict(P.fallbacks) == {'alpha': 2, 'interlaced': 1}
    P.fallbacks.clear()


def test_model_equals_zlib_and_pil(accepted):
    kinds = set()
    for name, data, pkt, ref in accepted:
        stream = pkt.buf[P.HDR_BYTES:].tobytes()
        want = zlib.decompress(stream)
        got, st = R.inflate(stream, pkt.inflated)
        assert st[0] == 0 and bytes(got) == want and st[1] == len(want), (name, st)
        arr, st2 = R.decode(pkt)
        assert st2 == st and arr.dtype == np.uint8 and arr.shape == ref.shape and np.array_equal(arr, ref), name
        assert st[2] >= 1 and st[3] >= 1
    # the code tables zlib's deflate never writes: ONE distance code of length 1 (incomplete, allowed) and no distance code at all --
    # the model must have seen them as incomplete codes, and nowhere else in the corpus (zlib always sends two distance codes)
    by_name = {a[0]: a for a in accepted}
    for name, want in (('single_distance_code', [(1, 1)]), ('empty_distance_code', [(1, 0)]), ('rle_runs_two_distance_codes', []), ('one_symbol', [])):
        R.incomplete.clear()
        assert R.decode(by_name[name][2])[1][0] == 0 and R.incomplete == want, (name, R.incomplete)
    assert R.decode(by_name['single_distance_code'][2])[1][3] == 22                       # 16 literals + 6 matches of distance 1
    by = {a[0]: R.decode(a[2])[1] for a in accepted if a[0].startswith(('flush', 'stored', 'far'))}
    assert by['stored_noise_300_two_idat'][2] >= 2 and by['flush_sync_every_1_rows'][2] >= 100 and by['far_window_32768'][3] == 129


def test_model_error_bits_on_the_corrupt_set():
    table = C.corrupt()
    assert len(table) == 13
    want = dict((n, b) for n, _, b in table)
    assert want['missing_distance_code'] == want['distance_with_empty_code'] == R.E_SYMBOL   # the unused half of a one-code table; any code of an empty one
    for name, data, bit in table:
        pkt, why = P.parse(data, name)
        assert pkt is not None, (name, why)                     # the container is fine: the stream is what is wrong
        arr, st = R.decode(pkt)
        assert st[0] == bit and arr is None, (name, st)
        assert 0 <= st[1] <= pkt.inflated
    bad = np.array(P.parse(table[0][1])[0].buf)
    bad[4 * P.HDR_ROWBYTES] ^= 1
    assert R.decode(bad)[1] == [R.E_HEADER, 0, 0, 0]


def test_png_layout_and_descriptors():
    import torch
    pk = [P.parse(d, n)[0] for n, d in C.accepted(None)[:3]]
    table, pb, ib, ob = O.OpList.png_layout(pk, guard=16)
    assert table.dtype == np.int32 and table.shape == (3, 4) and not table[:, 3].any()
    for k in range(3):
        assert table[k, 0] % 16 == 0 and table[k, 1] % 16 == 0 and table[k, 2] % 16 == 0
        if k:
            assert table[k, 0] >= table[k - 1, 0] + pk[k - 1].buf.nbytes and table[k, 1] >= table[k - 1, 1] + pk[k - 1].inflated
            assert table[k, 2] >= table[k - 1, 2] + pk[k - 1].nbytes_out + 16
    assert table[0, 2] == 16 and pb >= table[2, 0] + pk[2].buf.nbytes and ib >= table[2, 1] + pk[2].inflated and ob >= table[2, 2] + pk[2].nbytes_out
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)                      # noqa: E731
    packets, infl, out, status, tab = u8(pb), u8(ib), u8(ob), torch.zeros((3, 4), dtype=torch.int32), torch.from_numpy(table)
    ol = O.OpList()
    ol.png_inflate(packets, tab, infl, status, n=3)
    ol.png_unfilter(packets, tab, infl, out, status, n=3)
    recs = ol.finalize()
    assert [int(r['kind']) for r in recs] == [O.RESIZE, O.RESIZE] and [int(r['flags']) for r in recs] == [64, 128]
    for r in recs:
        assert [int(v) for v in r['i'][:4]] == [3, pb, ib, ob if r['flags'] == 128 else 0] and not r['i'][4:].any()
        p = [int(v) for v in r['p']]
        assert p[:3] == [packets.data_ptr(), tab.data_ptr(), infl.data_ptr()] and p[4] == status.data_ptr() and not any(p[5:])
        assert p[3] == (out.data_ptr() if r['flags'] == 128 else 0)
    with pytest.raises(ValueError):
        ol.png_inflate(packets, tab, infl, status.float(), n=3)
    with pytest.raises(ValueError):
        ol.png_inflate(packets, tab, infl, status, n=0)


def _host_compiler():
    for cc in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


def test_serial_core_under_sanitizers(accepted, tmp_path):
    """png_dec_host.cpp = the kernel's serial core with its own main, built with -fsanitize=address,undefined: the whole corpus and the
    corrupt set go through it on the CPU; its status lines equal the model's and its pixels PIL's."""
    cc = _host_compiler()
    if cc is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'png_dec_host')
    subprocess.run([cc, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(CSRC, 'png_dec_host.cpp'), '-o', exe], check=True)
    records = [(name, pkt, ref) for name, _, pkt, ref in accepted]
    for name, data, bit in C.corrupt():
        records.append((name, P.parse(data, name)[0], None))
    broken = np.array(records[0][1].buf)
    broken[4 * P.HDR_INFLATED] ^= 1
    records.append(('header', P.Packet(broken, records[0][1].shape, 'header'), None))
    corpus = tmp_path / 'corpus.bin'
    with open(corpus, 'wb') as f:
        for _, pkt, _ in records:
            f.write(struct.pack('<I', pkt.buf.nbytes) + pkt.buf.tobytes())
    run = subprocess.run([exe, str(corpus)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in run.stdout.splitlines()]
    assert len(lines) == len(records)
    for (name, pkt, ref), ln in zip(records, lines):
        arr, st = R.decode(pkt)
        assert ln[1:5] == st, (name, ln, st)
        if ref is not None:
            assert ln[1] == 0 and ln[5] == zlib.adler32(np.ascontiguousarray(ref).tobytes()) & 0xffffffff, name
        else:
            assert ln[1] != 0 and ln[5] == 0, name


def test_scorer_declined_ground_truth_takes_the_host_route(tmp_path):
    """SequenceScorer(gt_decode='device') on a ground truth the parser declines (a real Adam7 file): PIL decodes it as in host mode, the
    frame is counted by reason, the scores equal host mode's.  No decode kernel is needed, so the interpreter of the tests carries it."""
    import torch
    import jf_ref
    from mock_exec import MockExecutor
    from cutie_amd import _lib
    from cutie_amd.inference.utils import davis_metrics as M
    lace = str(tmp_path / 'lace')
    os.makedirs(os.path.join(lace, 'v'))
    for t in range(3):
        ids = C.mask(96, 136, 20 + t)
        with open(os.path.join(lace, 'v', f'{t:05d}.png'), 'wb') as f:
            f.write(C.interlaced_file(ids))
        assert np.array_equal(np.array(Image.open(os.path.join(lace, 'v', f'{t:05d}.png'))), ids)
        assert P.parse_file(os.path.join(lace, 'v', f'{t:05d}.png'))[1] == 'interlaced'
    pred = torch.from_numpy(C.mask(96, 136, 30))
    _lib.set_executor_for_testing(jf_ref.ScoreExecutor(MockExecutor()))
    try:
        P.fallbacks.clear()
        tables = {}
        for mode in ('host', 'device'):
            sc = M.SequenceScorer(lace, 'v', 'cpu', gt_decode=mode, skip_first_last=False)
            for t in range(3):
                sc.add(f'{t:05d}.png', pred)
            tables[mode] = sc.finish()
            assert sc.gt_fallbacks == ({'interlaced': 3} if mode == 'device' else {}) and sc.gt_device_frames == 0
        assert tables['host'] == tables['device'] and tables['host'] is not None and len(tables['host']['frames']) == 3
        assert dict(P.fallbacks) == {'interlaced': 3}
    finally:
        _lib.set_executor_for_testing(None)
        P.fallbacks.clear()


@pytest.fixture
def png_executor():
    """The interpreter of the tests with the PNG decode stages (the model) and the J&F stage (its model) on top."""
    import jf_ref
    from mock_exec import MockExecutor
    from cutie_amd import _lib
    ex = R.PngExecutor(jf_ref.ScoreExecutor(MockExecutor()))
    _lib.set_executor_for_testing(ex)
    yield ex
    _lib.set_executor_for_testing(None)


def _folders(root, H=40, W=70, videos=2, T=6):
    rng = np.random.default_rng(4)
    for v in range(videos):
        for d in ('GT', 'Pred'):
            os.makedirs(os.path.join(root, d, f'vid{v}'))
        for t in range(T):
            ids = C.mask(H, W, 100 * v + t, objects=v + 1)
            for d, arr in (('GT', ids), ('Pred', np.roll(ids, (1, 2), (0, 1)))):
                im = Image.fromarray(arr)
                im.putpalette(bytes(rng.integers(0, 256, 768, dtype=np.uint8)))
                im.save(os.path.join(root, d, f'vid{v}', f'{t:05d}.png'))
    return os.path.join(root, 'GT'), os.path.join(root, 'Pred')


def _read(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith('.csv') or f == 'scores.json'}


def test_png_to_device_wiring(accepted, png_executor):
    from cutie_amd.inference.data import device_ingest as DI
    some = [a for a in accepted if a[3].size < 20000][:12]
    views, chk = DI.png_to_device([a[2] for a in some], 'cpu', check=False, guard=16)
    chk()
    for (name, _, pkt, ref), v in zip(some, views):
        assert tuple(v.shape) == ref.shape and np.array_equal(v.numpy(), ref), name
    assert chk.status.numpy()[:, 0].tolist() == [0] * len(some) and png_executor.images == len(some)
    bad = P.parse(C.corrupt()[1][1], 'dir/cut_half.png')[0]
    with pytest.raises(ValueError, match='dir/cut_half.png'):
        DI.png_to_device([some[0][2], bad], 'cpu')


def test_consumers_device_decode_equals_host(tmp_path, png_executor):
    import torch
    from cutie_amd import score_masks as S
    from cutie_amd.inference.utils import davis_metrics as M
    gt, pred = _folders(str(tmp_path))
    tables = {}
    for mode in ('host', 'device'):
        sc = M.SequenceScorer(gt, 'vid1', 'cpu', gt_decode=mode)
        for t in range(6):
            sc.add(f'{t:05d}.png', torch.from_numpy(np.array(Image.open(os.path.join(pred, 'vid1', f'{t:05d}.png')))))
        tables[mode] = (sc.finish(), sc.table.numpy().copy())
        assert sc.gt_fallbacks == {} and sc.gt_device_frames == (6 if mode == 'device' else 0)
    assert tables['host'][0] == tables['device'][0] and np.array_equal(tables['host'][1], tables['device'][1])
    outs = {}
    for mode in ('host', 'device'):
        for batch in (16, 4):
            keep, S.DECODE_BATCH = S.DECODE_BATCH, batch
            try:
                out = str(tmp_path / f'{mode}{batch}')
                res = S.score_folders(pred, gt, dataset='syn', output=out, device='cpu', decode=mode, score_all_frames=batch == 4)
            finally:
                S.DECODE_BATCH = keep
            outs[mode, batch] = (_read(out), res)
    assert len(outs['host', 16][0]) == 3 and outs['host', 16] == outs['device', 16] and outs['host', 4] == outs['device', 4]
    assert S.decode_fallbacks == {} and png_executor.images == 6 + 2 * 2 * 2 * 6
    # a corrupt ground-truth stream in a fine container: ValueError naming the file, from finish at the latest
    f4 = os.path.join(gt, 'vid1', '00004.png')
    pkt = P.parse_file(f4)[0]
    stream = pkt.buf[P.HDR_BYTES:].tobytes()
    with open(f4, 'wb') as f:
        f.write(C.png_file(70, 40, int(pkt.hdr[P.HDR_DEPTH]), 3, stream[:len(stream) // 2]))
    with pytest.raises(ValueError, match='00004.png'):
        S.score_folders(pred, gt, dataset='syn', output=str(tmp_path / 'bad'), device='cpu', decode='device')
    with pytest.raises(ValueError):
        S.score_folders(pred, gt, decode='gpu')


def test_saver_scorer_choice_and_command_lines(tmp_path, png_executor):
    """The choice travels through ResultSaver(scorer=...), as eval_vos --score --gt-decode and process_video --gt-decode pass it."""
    import torch
    from cutie_amd import eval_vos as E, process_video as PV
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils import davis_metrics as M
    from cutie_amd.inference.utils.results_utils import ResultSaver
    gt, _ = _folders(str(tmp_path), videos=2, T=5)
    rng = np.random.default_rng(1)
    probs = [torch.from_numpy(rng.random((3, 40, 70)).astype(np.float32)) for _ in range(5)]
    scores = {}
    for mode in ('host', 'device'):
        om = ObjectManager()
        om.add_new_objects([1, 2])
        scorer = M.SequenceScorer(gt, 'vid1', 'cpu', gt_decode=mode)
        saver = ResultSaver(str(tmp_path / ('out_' + mode)), 'vid1', dataset='d17-val', object_manager=om, use_long_id=False, scorer=scorer)
        for t in range(5):
            saver.process(probs[t], f'{t:05d}.jpg')
        saver.end()
        scores[mode] = saver.scores
        assert scorer.gt_device_frames == (5 if mode == 'device' else 0)
    assert scores['host'] is not None and scores['host'] == scores['device']
    ap = E.arg_parser()
    a = ap.parse_args(['--images', 'I', '--masks', 'M', '--output', 'O', '--dataset', 'd17-val', '--score', '--gt-decode', 'device'])
    assert a.gt_decode == 'device'
    assert ap.parse_args(['--images', 'I', '--masks', 'M', '--output', 'O', '--dataset', 'd17-val', '--score']).gt_decode == 'host'
    import inspect
    for fn in (E._saver, E.process_video, E.process_video_multiscale, E.process_videos_lockstep, PV.process_video):
        assert inspect.signature(fn).parameters['gt_decode'].default == 'host', fn.__name__


def test_eval_vos_score_gt_decode_device_through_the_interpreter(tmp_path):
    """eval_vos.run_dataset --score --gt-decode device on the interpreter of the descriptors: the same result files as --gt-decode host."""
    import jf_ref
    from mock_exec import MockExecutor
    from cutie_amd import _lib, eval_vos as E
    from cutie_amd.config import default_config
    from cutie_amd.inference.utils.results_utils import davis_palette
    from cutie_amd.model.cutie import CUTIE
    from cutie_amd.utils.synth import SyntheticClip
    from oracle.weights import make_state_dict
    root = str(tmp_path)
    clip = SyntheticClip(64, 96, 2, 4, seed=9)
    for d in ('JPEGImages', 'Annotations', 'GT'):
        os.makedirs(os.path.join(root, d, 'vid'))
    m0 = clip.first_mask().numpy().astype(np.uint8)
    for t in range(4):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'JPEGImages', 'vid', f'{t:05d}.jpg'), quality=95)
        for d in ('GT',) + (('Annotations',) if t == 0 else ()):
            png = Image.fromarray(np.roll(m0, t, 1))
            png.putpalette(davis_palette)
            png.save(os.path.join(root, d, 'vid', f'{t:05d}.png'))
    mx = MockExecutor()
    mx.per_sample_conv = True
    ex = R.PngExecutor(jf_ref.ScoreExecutor(mx))
    _lib.set_executor_for_testing(ex)
    try:
        net = CUTIE(default_config())
        net.load_weights(make_state_dict(seed=0))
        files = {}
        for mode in ('host', 'device'):
            out = os.path.join(root, 'out_' + mode)
            ap = E.arg_parser()
            args = ap.parse_args(['--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations'), '--gt',
                                  os.path.join(root, 'GT'), '--output', out, '--dataset', 'd17-val', '--score', '--score-all-frames',
                                  '--size', '-1', '--gt-decode', mode])
            E.check_args(ap, args)
            before = ex.images
            res = E.run_dataset(net, default_config(mem_every=2), args)
            assert res[0]['frames'] == 4 and len(res[0]['scores']['frames']) == 4
            assert ex.images - before == (4 if mode == 'device' else 0)
            files[mode] = _read(out)
        assert len(files['host']) == 3 and files['host'] == files['device']
    finally:
        _lib.set_executor_for_testing(None)
