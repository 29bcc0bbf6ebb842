"""DAVIS J&F scoring without a GPU: the numpy / scipy model of the device counts (tests/jf_ref.py) against hand-worked planes, the float
arithmetic on the counts and the result files (cutie_amd/inference/utils/davis_metrics.py), the argument checks of OpList.jf_counts and
eval_vos, and the host wiring -- ResultSaver(scorer=...) and score_masks -- through an executor that answers PROB_TO_ID flags == 64 with
the model (jf_ref.ScoreExecutor around tests/mock_exec.py)."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.inference.utils import davis_metrics as M

import jf_ref as R


# ---- the model against hand-worked planes --------------------------------------------------------------------------------------------------
def test_boundary_map_of_a_block_in_4x4():
    seg = np.array([[0, 0, 0, 0],
                    [0, 1, 1, 0],
                    [0, 1, 1, 0],
                    [0, 0, 0, 0]])
    want = np.array([[1, 1, 1, 0],             # the boundary lies on the pixel whose east / south / south-east neighbour differs
                     [1, 0, 1, 0],
                     [1, 1, 1, 0],
                     [0, 0, 0, 0]], dtype=bool)
    assert np.array_equal(R.seg2bmap(seg), want)
    assert not R.seg2bmap(np.ones((4, 4))).any() and not R.seg2bmap(np.zeros((1, 1))).any() and not R.seg2bmap(np.ones((1, 1))).any()
    # last row: s ^ e only; last column: s ^ so only; the bottom-right pixel is 0
    assert R.seg2bmap(np.array([[0, 1, 1, 0, 1]])).tolist() == [[True, False, True, True, False]]
    assert R.seg2bmap(np.array([[0, 1, 1, 0, 1]]).T).T.tolist() == [[True, False, True, True, False]]
    full = np.array([[1, 1], [1, 1]])
    assert not R.seg2bmap(full).any()
    assert R.seg2bmap(np.array([[0, 0], [0, 1]])).tolist() == [[True, True], [True, False]]


GT6 = np.array([[0, 0, 0, 0, 0, 0],
                [0, 2, 2, 0, 0, 0],
                [0, 2, 2, 0, 255, 255],
                [0, 0, 0, 0, 255, 255],
                [0, 0, 0, 0, 1, 1],
                [0, 0, 0, 0, 1, 1]], dtype=np.uint8)
PRED6 = np.array([[0, 0, 0, 0, 0, 0],
                  [0, 2, 2, 0, 0, 0],
                  [0, 2, 2, 0, 1, 1],
                  [0, 0, 0, 0, 1, 1],
                  [0, 0, 0, 0, 1, 1],
                  [0, 0, 0, 0, 1, 1]], dtype=np.uint8)


def test_counts_of_a_6x6_pair_with_a_void_region():
    b_gt1 = np.zeros((6, 6), dtype=bool)
    for y, x in ((3, 3), (3, 4), (3, 5), (4, 3), (5, 3)):       # object 1 touches the last row and column: s ^ so there, s ^ e below
        b_gt1[y, x] = True
    assert np.array_equal(R.seg2bmap(GT6 == 1), b_gt1)
    b_pr1 = np.zeros((6, 6), dtype=bool)
    for y, x in ((1, 3), (1, 4), (1, 5), (2, 3), (3, 3), (4, 3), (5, 3)):
        b_pr1[y, x] = True
    assert np.array_equal(R.seg2bmap(PRED6 == 1), b_pr1)
    got = R.counts(PRED6, GT6, [1, 2, 3], 1)
    # object 1: the prediction also covers the void region -- 255 is background for every object, as davis2017's get_all_masks makes it
    assert got[0].tolist() == [4, 8, 7, 5, 4, 4, 8, 4]
    assert got[1].tolist() == [4, 4, 8, 8, 8, 8, 4, 4]
    assert got[2].tolist() == [0] * 8                           # listed, absent from both planes
    assert R.counts(PRED6, GT6, [1], 2)[0].tolist() == [4, 8, 7, 5, 7, 5, 8, 4]      # within 2 everything matches
    assert R.disk(2).astype(int).tolist() == [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]
    # an image smaller than the radius: nothing outside it takes part
    assert R.counts(np.array([[1, 0, 0]], dtype=np.uint8), np.array([[0, 0, 1]], dtype=np.uint8), [1], 4)[0].tolist() == [0, 2, 1, 1, 1, 1, 1, 1]


def test_the_batched_masked_dilation_is_the_plain_one():
    """jf_ref.matched asks scipy for the dilation at the mask's pixels only, over a stack: the same sums as the full dilation per plane"""
    rng = np.random.default_rng(2)
    for H, W, r in ((1, 1, 1), (5, 3, 4), (37, 70, 3), (66, 130, 8), (30, 90, 40)):
        a, b = rng.random((3, H, W)) < 0.1, rng.random((3, H, W)) < 0.03
        b[2] = False
        want = [int((a[q] & R.dilate(b[q], r)).sum()) for q in range(3)]
        assert R.matched(a, b, r).tolist() == want and want[2] == 0


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_j_and_f_special_cases():
    rows = np.array([[0, 0, 0, 0, 0, 0, 0, 0],                  # nothing anywhere: J = 1, F = 1
                     [0, 5, 0, 4, 0, 0, 0, 5],                  # no prediction, a ground truth: J = 0, (p, r) = (1, 0): F = 0
                     [0, 5, 4, 0, 0, 0, 5, 0],                  # a prediction, no ground truth: (0, 1): F = 0
                     [3, 6, 4, 8, 2, 2, 4, 5],                  # p = 0.5, r = 0.25: F = 2 * .125 / .75
                     [2, 4, 4, 4, 0, 0, 3, 3],                  # boundaries that never meet: p + r == 0
                     [9, 9, 0, 0, 0, 0, 9, 9]])                 # the object fills the image: no boundary in either: F = 1
    assert M.j_from_counts(rows).tolist() == [1.0, 0.0, 0.0, 0.5, 0.5, 1.0]
    assert M.f_from_counts(rows).tolist() == [1.0, 0.0, 0.0, 2 * 0.5 * 0.25 / 0.75, 0.0, 1.0]
    assert M.j_from_counts(rows).dtype == np.float64 and M.f_from_counts(rows.reshape(2, 3, 8)).shape == (2, 3)


def test_bound_pix():
    assert [M.bound_pix(*hw) for hw in ((480, 854), (1080, 1920), (2160, 3840), (37, 70), (1, 1))] == [8, 18, 36, 1, 1]
    assert M.bound_pix(2160, 3840) <= O.OpList.JF_MAX_RADIUS == 40


def test_statistics_on_hand_numbers():
    assert M.statistics([0.7]) == (0.7, 1.0, 0.0)
    m, r, d = M.statistics([0.2, 0.8])                          # edges 0 0 1 1 1: first bin [0.2], last bin [0.8]
    assert (m, r) == (0.5, 0.5) and d == pytest.approx(-0.6, abs=1e-15)
    m, r, d = M.statistics([0.9, 0.6, 0.3])                     # edges 0 1 1 2 2: first bin [0.9, 0.6], last bin [0.3]
    assert m == pytest.approx(0.6, abs=1e-15) and r == pytest.approx(2 / 3, abs=1e-15) and d == pytest.approx(0.45, abs=1e-15)
    m, r, d = M.statistics([1.0, 0.8, 0.4, 0.2])                # edges 0 1 2 2 3: first bin [1, 0.8], last bin [0.4, 0.2]
    assert m == pytest.approx(0.6, abs=1e-15) and r == 0.5 and d == pytest.approx(0.6, abs=1e-15)
    m, r, d = M.statistics([1.0, 0.8, 0.6, 0.4, 0.2])           # edges 0 1 2 3 4: first bin [1, 0.8], last bin [0.4, 0.2]
    assert m == pytest.approx(0.6, abs=1e-15) and r == 0.6 and d == pytest.approx(0.6, abs=1e-15)
    v = np.arange(300) / 299.0                                  # edges 0 75 150 224 299 -- as uint8 the last would wrap to 43
    m, r, d = M.statistics(v)
    assert m == pytest.approx(0.5, abs=1e-15) and r == 150 / 300
    assert d == pytest.approx((np.arange(0, 76).mean() - np.arange(224, 300).mean()) / 299.0, abs=1e-15) and d < -0.7
    with pytest.raises(ValueError):
        M.statistics([])


def test_result_files_text(tmp_path):
    seqs = {'b': None,                                          # a sequence without a scored frame is left out
            'a': {'objects': [1, 2], 'frames': ['00001.png', '00002.png'], 'counts': [[[0] * 8] * 2] * 2,
                  'J': [[1.0, 0.45], [0.5, 0.25]], 'F': [[0.8, 0.4], [0.6, 0.2]]},
            'c': {'objects': [1], 'frames': ['00001.png'], 'counts': [[[0] * 8]], 'J': [[0.55]], 'F': [[0.7]]}}
    glob = M.write_results(str(tmp_path), 'd17-val', seqs)
    # per object (mean, recall, decay): a_1 J (.75, .5, .5) F (.7, 1, .2); a_2 J (.35, 0, .2) F (.3, 0, .2); c_1 J (.55, 1, 0) F (.7, 1, 0)
    assert open(tmp_path / 'global_results-d17-val.csv').read() == \
        'J&F-Mean,J-Mean,J-Recall,J-Decay,F-Mean,F-Recall,F-Decay\n0.558,0.550,0.500,0.233,0.567,0.667,0.133\n'
    assert open(tmp_path / 'per-sequence_results-d17-val.csv').read() == 'Sequence,J-Mean,F-Mean\na_1,0.750,0.700\na_2,0.350,0.300\nc_1,0.550,0.700\n'
    back = json.load(open(tmp_path / 'scores.json'))
    assert back['dataset'] == 'd17-val' and sorted(back['sequences']) == ['a', 'c'] and back['sequences']['a'] == seqs['a']
    assert back['global'] == glob and glob['J&F-Mean'] == pytest.approx((glob['J-Mean'] + glob['F-Mean']) / 2, abs=1e-15)
    assert back['per_object']['a_2'] == {'J-Mean': pytest.approx(0.35), 'F-Mean': pytest.approx(0.3)}
    with pytest.raises(ValueError, match='no sequence'):
        M.write_results(str(tmp_path), 'x', {'b': None})


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def test_jf_counts_validation():
    H, W = 5, 70
    pred, gt = torch.zeros((H, W), dtype=torch.uint8), torch.zeros((H, W), dtype=torch.uint8)
    counts = torch.zeros((2, 8), dtype=torch.int32)
    assert O.OpList.jf_scratch_words(H, W, 2) == 4 * 2 * 5 * 2 and O.OpList.jf_scratch_words(480, 854, 3) == 4 * 3 * 480 * 14
    good = dict(pred=pred, gt=gt, objects=[1, 2], counts=counts, H=H, W=W, radius=1)
    ol = O.OpList()
    ol.jf_counts(**good)
    arr = ol.finalize()
    assert int(arr['kind'][0]) == O.PROB_TO_ID and int(arr['flags'][0]) == 64
    assert arr['i'][0][[1, 2, 5, 9]].tolist() == [H, W, 1, 2] and int(arr['i'][0][8]) >= 80
    assert int(arr['p'][0][2]) == pred.data_ptr() and int(arr['p'][0][3]) == gt.data_ptr() and int(arr['p'][0][7]) == counts.data_ptr()
    for change, msg in ((dict(objects=[0, 1]), '1 .. 254'), (dict(objects=[1, 255]), '1 .. 254'), (dict(objects=[1, 256]), '1 .. 254'),
                        (dict(objects=[2, 2]), 'duplicate'), (dict(objects=[], counts=counts[:0]), '0 objects'),
                        (dict(radius=0), 'radius 0'), (dict(radius=41), 'radius 41'), (dict(H=0), 'H, W >= 1'),
                        (dict(pred=pred.int()), 'pred is a contiguous uint8'), (dict(gt=gt[:, :69]), 'gt is a contiguous uint8'),
                        (dict(pred=torch.zeros((W, H), dtype=torch.uint8).t()), 'pred is a contiguous uint8'),
                        (dict(counts=counts[:1]), 'counts is a contiguous int32'), (dict(counts=counts.long()), 'counts is a contiguous int32'),
                        (dict(scratch=torch.zeros(79, dtype=torch.int32)), 'scratch is int32'),
                        (dict(objects=torch.tensor([1, 2])), 'int32')):
        with pytest.raises(ValueError, match=msg):
            O.OpList().jf_counts(**dict(good, **change))
    O.OpList().jf_counts(**dict(good, objects=torch.tensor([1, 2], dtype=torch.int32)))      # a device table is taken as it is


def _args(argv):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(argv)
    E.check_args(ap, args)
    return args


def test_check_args_of_the_score_switches(tmp_path, capsys):
    base = ['--images', 'I', '--output', 'O']
    a = _args(base + ['--masks', 'M', '--score'])
    assert a.score and a.gt == 'M' and not a.score_all_frames
    a = _args(base + ['--masks', 'M', '--score', '--gt', 'G', '--score-all-frames'])
    assert a.gt == 'G' and a.score_all_frames
    assert not _args(base + ['--masks', 'M']).score
    rgb = tmp_path / 'long' / 'vid'
    rgb.mkdir(parents=True)
    Image.fromarray(np.zeros((4, 4, 3), dtype=np.uint8)).save(rgb / '00000.png')
    for bad, word in ((base + ['--dataset', 'burst-val', '--json', 'J', '--score'], 'BURST'),
                      (base + ['--masks', str(tmp_path / 'long'), '--score'], 'long-id'),
                      (base + ['--masks', 'M', '--gt', 'G'], '--score'),
                      (base + ['--masks', 'M', '--score-all-frames'], '--score')):
        with pytest.raises(SystemExit) as e:
            _args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err


# ---- host wiring ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def score_executor():
    from mock_exec import MockExecutor
    ex = R.ScoreExecutor(MockExecutor())
    _lib.set_executor_for_testing(ex)
    yield ex
    _lib.set_executor_for_testing(None)


def _blobs(rng, H, W, ids, cell=6):
    low = rng.choice(ids, size=(-(-H // cell), -(-W // cell)))
    return low.astype(np.uint8).repeat(cell, 0).repeat(cell, 1)[:H, :W]


def _dataset(root, names, H=40, W=70, T=5):
    """ground truth: per video T frames of blobs of objects 1 and 2 (frame 2 has a void region), and the probabilities of a prediction"""
    rng = np.random.default_rng(5)
    probs = {}
    for name in names:
        os.makedirs(os.path.join(root, 'gt', name))
        for t in range(T):
            gt = _blobs(rng, H, W, [0, 0, 1, 2])
            if t == 2:
                gt[5:12, 50:70] = 255
            im = Image.fromarray(gt)
            im.putpalette(bytes(range(256)) * 3)
            im.save(os.path.join(root, 'gt', name, f'{t:05d}.png'))
            shifted = np.roll(np.where(gt == 255, 0, gt), (1, t), (0, 1))
            p = torch.full((3, H, W), 0.1)
            p.scatter_(0, torch.from_numpy(shifted.astype(np.int64))[None], 0.8)
            probs[name, t] = p
    return probs


def _model_scores(results, gt, name, frames):
    rows = []
    objects = None
    for f in frames:
        g = np.array(Image.open(os.path.join(gt, name, f)))
        if objects is None:
            first = np.array(Image.open(os.path.join(gt, name, sorted(os.listdir(os.path.join(gt, name)))[0])))
            objects = list(range(1, int(first[first != 255].max()) + 1))
        p = np.array(Image.open(os.path.join(results, name, f)))
        rows.append(R.counts(p, g, objects, M.bound_pix(*g.shape)))
    c = np.stack(rows)
    return {'objects': objects, 'frames': list(frames), 'counts': c.tolist(), 'J': M.j_from_counts(c).tolist(), 'F': M.f_from_counts(c).tolist()}


def _read(d):
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith('.csv') or f == 'scores.json'}


def test_saver_and_score_masks_through_the_model(tmp_path, score_executor):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    from cutie_amd.score_masks import score_folders
    root = str(tmp_path)
    names = ('vidA', 'vidB')
    probs = _dataset(root, names)
    gt, out = os.path.join(root, 'gt'), os.path.join(root, 'out')
    scores = {}
    for name in names:
        om = ObjectManager()
        om.add_new_objects([1, 2])
        scorer = M.SequenceScorer(gt, name, 'cpu')
        assert scorer.objects == [1, 2] and tuple(scorer.table.shape) == (5, 2, 8)
        saver = ResultSaver(out, name, dataset='d17-val', object_manager=om, use_long_id=False, scorer=scorer)
        for t in range(5):
            saver.process(probs[name, t], f'{t:05d}.jpg')
        saver.process(probs[name, 0], '00009.jpg')                  # no ground truth for this frame: skipped
        saver.end()
        scores[name] = saver.scores
        assert scores[name] == _model_scores(out, gt, name, ['00001.png', '00002.png', '00003.png'])
        assert 0 < np.mean(scores[name]['J']) < 1 and 0 < np.mean(scores[name]['F']) < 1
    assert score_executor.calls == 10
    a, b, c = (os.path.join(root, d) for d in 'abc')
    M.write_results(a, 'd17-val', scores)
    M.write_results(b, 'd17-val', {n: _model_scores(out, gt, n, ['00001.png', '00002.png', '00003.png']) for n in names})
    glob, per = score_folders(out, gt, dataset='d17-val', output=c, device='cpu')
    assert _read(a) == _read(b) == _read(c) and len(_read(a)) == 3 and per == scores
    assert len(open(os.path.join(a, 'per-sequence_results-d17-val.csv')).read().splitlines()) == 5
    # every frame scored
    _, per_all = score_folders(out, gt, dataset='all', output=os.path.join(root, 'd'), score_all_frames=True, device='cpu')
    assert per_all['vidA'] == _model_scores(out, gt, 'vidA', [f'{t:05d}.png' for t in range(5)])
    # refusals
    om = ObjectManager()
    with pytest.raises(ValueError, match='long ids'):
        ResultSaver(out, 'vidA', dataset='d17-val', object_manager=om, use_long_id=True, scorer=M.SequenceScorer(gt, 'vidA', 'cpu'))
    with pytest.raises(ValueError, match='40 x 70'):
        M.SequenceScorer(gt, 'vidA', 'cpu').add('00001.png', torch.zeros((40, 71), dtype=torch.uint8))
    with pytest.raises(ValueError, match='no ground-truth folder'):
        M.SequenceScorer(gt, 'nope', 'cpu')
    only_first = M.SequenceScorer(gt, 'vidA', 'cpu')
    only_first.add('00000.png', torch.zeros((40, 70), dtype=torch.uint8))
    assert only_first.finish() is None                                # the first frame alone: nothing is scored


# ---- process_video --gt --------------------------------------------------------------------------------------------------------------------
def test_process_video_scores_its_video(tmp_path, capsys, monkeypatch):
    """cutie_amd.process_video(gt_dir=...) on the interpreter of the descriptors: every frame that has a ground-truth file named like the
    outputs (7 digits) is scored, the first and last one included, against the masks the run wrote; ``main`` prints the J&F line."""
    import sys
    from mock_exec import MockExecutor
    from cutie_amd import process_video as PV
    from cutie_amd.inference.utils.results_utils import davis_palette
    from cutie_amd.model.cutie import CUTIE
    from cutie_amd.utils.synth import SyntheticClip
    from oracle.weights import make_state_dict
    mx = MockExecutor()
    mx.per_sample_conv = True
    ex = R.ScoreExecutor(mx)
    _lib.set_executor_for_testing(ex)
    try:
        cfg = PV.video_config(mem_every=2, max_internal_size=-1)
        net = CUTIE(cfg)
        net.load_weights(make_state_dict(seed=0))
        clip = SyntheticClip(64, 96, 2, 3, seed=4)
        frames, masks, gt, out = (os.path.join(str(tmp_path), d) for d in ('frames', 'masks', 'gt', 'out'))
        for d in (frames, masks, gt):
            os.makedirs(d)
        m0 = clip.first_mask().numpy().astype(np.uint8)
        for t in range(3):
            Image.fromarray((clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(os.path.join(frames, f'{t:07d}.png'))
        png = Image.fromarray(m0)
        png.putpalette(davis_palette)
        png.save(os.path.join(masks, '0000000.png'))
        for t in (0, 2):                                              # frame 1 has no ground truth: it is skipped
            png = Image.fromarray(np.roll(m0, t, 1))
            png.putpalette(davis_palette)
            png.save(os.path.join(gt, f'{t:07d}.png'))
        r = PV.process_video(net, cfg, frames, masks, out, gt_dir=gt)
        names = ['0000000.png', '0000002.png']
        assert r['frames'] == 3 and ex.calls == 2 and r['scores']['frames'] == names and r['scores']['objects'] == [1, 2]
        rows = np.stack([R.counts(np.array(Image.open(os.path.join(out, f))), np.array(Image.open(os.path.join(gt, f))), [1, 2], M.bound_pix(64, 96))
                         for f in names])
        assert r['scores']['counts'] == rows.tolist() and r['scores']['J'] == M.j_from_counts(rows).tolist()
        assert r['scores']['J'][0] == [1.0, 1.0]                      # frame 0 comes back as its mask, which is its ground truth
        # the command line: the same figures, printed
        monkeypatch.setattr(PV, 'process_video', lambda *a, **k: dict(r, seconds=1.0))
        monkeypatch.setattr('cutie_amd.model.cutie.CUTIE', lambda cfg: type('N', (), {'cuda': lambda s: s, 'eval': lambda s: s})())
        monkeypatch.setattr(torch.cuda, 'max_memory_allocated', lambda: 0)
        monkeypatch.setattr(sys, 'argv', ['process_video', '-v', frames, '-m', masks, '-o', out, '--gt', gt])
        PV.main()
        glob, _ = M.summarize({'frames': r['scores']})
        assert 'J&F: ' + M.global_line(glob) in capsys.readouterr().out
    finally:
        _lib.set_executor_for_testing(None)
