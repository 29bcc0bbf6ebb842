"""Multi-scale merge (PROB_TO_ID flags&16, ABI 8) without a GPU: the numpy model (tests/merge_ref.py) against the real file route
(score dumps + cutie_amd.merge_multi_scale) and against torch's own F.interpolate, the --sizes rules, ResultSaver.process_merged's
argument checks and the descriptor OpList.prob_to_id_merged encodes."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import merge_ref as M


# ---- the model against the file route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [2, 3])
def test_model_equals_the_file_route(tmp_path, S):
    from cutie_amd.merge_multi_scale import merge
    srcs = [(37, 53), (48, 64), (75, 101)][:S]
    OH, OW = 61, 83
    P = 4
    backward = {5: 1, 3: 2, 9: 3}                                # {object id: tmp id}, not the identity
    lut = [0, 5, 3, 9]
    runs = []
    frames = ['00000', '00001']
    want = {}
    for fi, f in enumerate(frames):
        probs = [M.smooth_probs(P, h, w, seed=10 * fi + s).numpy() for s, (h, w) in enumerate(srcs)]
        for s, q in enumerate(M.member_scores(probs, OH, OW)):
            d = os.path.join(tmp_path, f'run{s}', 'Scores', 'vid')
            os.makedirs(d, exist_ok=True)
            np.savez_compressed(os.path.join(d, f + '.npz'), prob=q)
            if fi == 0:
                runs.append(os.path.join(tmp_path, f'run{s}'))
                ids = sorted((t, o) for o, t in backward.items())
                np.savez(os.path.join(d, 'backward.npz'), obj_ids=np.array([o for _, o in ids], dtype=np.int64),
                         tmp_ids=np.array([t for t, _ in ids], dtype=np.int64))
        want[f] = M.merge(probs, lut, OH, OW)
    out = os.path.join(tmp_path, 'merged')
    assert merge(runs, out, 'D', num_proc=1) == len(frames)
    for f in frames:
        got = np.array(Image.open(os.path.join(out, 'vid', f + '.png')))
        assert got.shape == (OH, OW) and np.array_equal(got, want[f])
        assert len(np.unique(got)) > 2                           # (several objects win somewhere: the map matters)
    assert not np.array_equal(want['00000'], want['00001'])


# ---- the model against torch's interpolate ----------------------------------------------------------------------------------------
TORCH_CASES = [(4, [(60, 107), (75, 133), (90, 160)], (120, 214)),
               (3, [(48, 64), (37, 53)], (101, 149)),
               (8, [(30, 40), (40, 53), (50, 67), (60, 80)], (61, 83)),
               (4, [(480, 854), (600, 1067), (720, 1280)], (1080, 1920))]


@pytest.mark.parametrize('P,srcs,dst', TORCH_CASES, ids=[f'P{c[0]}x{len(c[1])}to{c[2][0]}' for c in TORCH_CASES])
def test_model_against_torch_interpolate(P, srcs, dst):
    """Route: torch's fp32 F.interpolate per member -> (x * 255).to(uint8) -> integer sum -> argmax.  Every member can move a plane's
    quantised score by at most 1 against the model, a sum by at most S and the gap between two sums by at most 2 S: ids may differ only
    where that route's two largest sums lie within 2 S, and on at most 0.1 % of the pixels (a condition, not a measurement)."""
    S = len(srcs)
    probs = [M.smooth_probs(P, h, w, seed=7 * s + P) for s, (h, w) in enumerate(srcs)]
    tq = [(F.interpolate(p[None], size=dst, mode='bilinear', align_corners=False)[0] * 255).to(torch.uint8).numpy() for p in probs]
    mq = M.member_scores([p.numpy() for p in probs], *dst)
    for s in range(S):
        d = np.abs(tq[s].astype(np.int32) - mq[s].astype(np.int32))
        assert d.max() <= 1
        print(f'member {s}: {int((d != 0).sum())} of {d.size} quantised scores differ')
    total = sum(q.astype(np.int32) for q in tq)
    ids_t = total.argmax(0)
    ids_m = sum(q.astype(np.int32) for q in mq).argmax(0)
    srt = np.sort(total, axis=0)
    gap = srt[-1] - srt[-2]
    diff = ids_t != ids_m
    print(f'{int(diff.sum())} of {diff.size} ids differ; {float((gap <= 2 * S).mean()):.4%} of the pixels within the 2 S gap')
    assert bool((gap[diff] <= 2 * S).all())
    assert diff.sum() <= 0.001 * diff.size
    assert (gap <= 2 * S).any()                                  # (the condition is not vacuous on these inputs)


def test_model_sampling_properties():
    p = M.smooth_probs(3, 9, 13, seed=1).numpy()
    assert np.array_equal(M.resize(p, 9, 13), p)                 # a source of the output's size samples itself exactly
    assert np.array_equal(M.quantise(np.array([1.0, 0.5001, 0.5019, 0.0], dtype=np.float32)), [255, 127, 127, 0])
    flat = np.full((4, 5, 7), 0.25, dtype=np.float32)
    assert (M.merge([flat, flat[:, :3, :4]], [7, 1, 2, 3], 11, 9) == 7).all()      # all equal -> plane 0


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def _parse(argv):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(['--images', 'a', '--masks', 'b', '--output', 'c'] + argv)
    E.check_args(ap, args)
    return args


def test_sizes_rules(capsys):
    assert _parse(['--sizes', '480', '600', '720']).sizes == [480, 600, 720]
    assert _parse(['--sizes', '-1', '480', '--clips-in-flight', '2', '--flip-aug', '--egress', 'device', '--ingest', 'device']).sizes == [-1, 480]
    assert _parse([]).sizes is None
    for bad, word in ((['--sizes', '480'], 'two distinct'), (['--sizes', '480', '480'], 'two distinct'), (['--sizes', '480', '0'], 'positive'),
                      (['--sizes', '480', '600', '--size', '480'], '--size'), (['--sizes', '480', '600', '--save-scores'], '--save-scores'),
                      (['--sizes', '480', '600', '--lockstep', '2'], '--lockstep'),
                      (['--sizes'] + [str(100 + k) for k in range(9)], 'at most 8')):
        with pytest.raises(SystemExit) as e:
            _parse(bad)
        assert e.value.code == 2
        assert word in capsys.readouterr().err


def _saver(tmp_path, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    om.add_new_objects([5, 3])
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device('cpu')), object_manager=om)
    return ResultSaver(str(tmp_path), 'vid', dataset='generic', object_manager=om, use_long_id=False, processor=proc, **kw), om


def test_process_merged_argument_checks(tmp_path):
    probs = [torch.full((3, 4, 6), 1 / 3), torch.full((3, 8, 12), 1 / 3)]
    saver, om = _saver(tmp_path)
    try:
        own = {t: o.id for t, o in om.tmp_id_to_obj.items()}
        assert own == {1: 5, 2: 3}
        with pytest.raises(ValueError, match='disagree'):
            saver.process_merged(probs, '00000.jpg', (8, 12), id_maps=[own, {1: 3, 2: 5}])
        with pytest.raises(ValueError, match='disagree'):
            saver.process_merged(probs, '00000.jpg', (8, 12), id_maps=[own, {1: 5}])
        with pytest.raises(ValueError, match='planes'):
            saver.process_merged([probs[0], probs[1][:2]], '00000.jpg', (8, 12), id_maps=[own, own])
        with pytest.raises(ValueError, match='members'):
            saver.process_merged([probs[0]] * 9, '00000.jpg', (8, 12))
    finally:
        saver.end()
    saver, _ = _saver(tmp_path, save_scores=True, score_output_root=str(tmp_path / 's'))
    try:
        with pytest.raises(ValueError, match='save_scores'):
            saver.process_merged(probs, '00000.jpg', (8, 12))
    finally:
        saver.end()
    assert not os.path.exists(tmp_path / 's') and not os.path.exists(tmp_path / 'vid')


def test_process_video_multiscale_refuses_save_scores():
    from cutie_amd.eval_vos import process_video_multiscale
    with pytest.raises(ValueError, match='save_scores'):
        process_video_multiscale(None, None, [], 'out', save_scores=True, score_output_root='s')


def test_descriptor_of_prob_to_id_merged():
    """S, the two tables and the flags sit where include/cutie_hip.h says (PROB_TO_ID, ABI 8)."""
    from cutie_amd import ops as O
    big = torch.rand(3, 20, 32)
    probs = [big[:, 2:17, 3:29], torch.rand(3, 7, 9), torch.rand(3, 30, 41)]
    lut = torch.tensor([0, 4, 9], dtype=torch.int32)
    for dtype, code in ((torch.uint8, 0), (torch.int32, 1)):
        out = torch.empty((30, 41), dtype=dtype)
        ol = O.OpList()
        ol.prob_to_id_merged(probs, lut, out, out_hw=(30, 41))
        rec = ol.finalize()[0]
        assert rec['kind'] == O.PROB_TO_ID and rec['flags'] == (code | 4 | 16)
        i, p = rec['i'], rec['p']
        assert (i[0], i[5], i[6], i[9]) == (3, 30, 41, 3) and not i[1:5].any() and not i[7:9].any()
        ptrs, geom = O.OpList.merge_tables(probs)
        assert p[0] == ptrs.data_ptr() and p[1] == lut.data_ptr() and p[2] == out.data_ptr() and p[6] == geom.data_ptr() and not p[3:6].any()
        assert ptrs.dtype == torch.int64 and ptrs.tolist() == [t.data_ptr() for t in probs]
        assert geom.dtype == torch.int32 and geom.tolist() == [[15, 26, 640, 32], [7, 9, 63, 9], [30, 41, 1230, 41]]
        assert O.OpList.merge_tables(probs)[0] is ptrs            # cached per (data_ptr, shape, strides)
        assert O.OpList.merge_tables([probs[0], probs[1], probs[2][:, :29]])[1] is not geom
    out = torch.empty((30, 41), dtype=torch.uint8)
    stream, status, scratch = torch.empty(O.OpList.png_capacity(30, 41), dtype=torch.uint8), torch.empty(4, dtype=torch.int32), \
        torch.empty(O.OpList.png_scratch_words(30, 41), dtype=torch.int32)
    ol = O.OpList()
    ol.prob_to_id_merged(probs, lut, out, out_hw=(30, 41), png=(stream, status, scratch))
    rec = ol.finalize()[0]
    assert rec['flags'] == (4 | 8 | 16) and (rec['i'][7], rec['i'][8], rec['i'][9]) == (stream.numel(), scratch.numel(), 3)
    assert [int(v) for v in rec['p'][3:6]] == [stream.data_ptr(), status.data_ptr(), scratch.data_ptr()]
    ol = O.OpList()
    for bad in ([], [probs[1]] * 9):
        with pytest.raises(ValueError):
            ol.prob_to_id_merged(bad, lut, out, out_hw=(30, 41))
    with pytest.raises(ValueError):
        ol.prob_to_id_merged(probs, lut, torch.empty((30, 41), dtype=torch.int64), out_hw=(30, 41))
    with pytest.raises(ValueError):
        ol.prob_to_id_merged(probs, lut, out, out_hw=(31, 41))
    with pytest.raises(ValueError):
        ol.prob_to_id_merged([probs[1], torch.rand(4, 7, 9)], lut, out, out_hw=(30, 41))
    assert len(ol) == 0
    assert O.OpList.MERGE_MAX_SOURCES == 8
