"""BURST evaluation without a GPU: the COCO RLE codec (cutie_amd/inference/utils/coco_rle.py) on hand-made vectors and round trips,
BURSTVideoReader / BURSTTestDataset on a sequence json over the tests/golden/bike frames, ResultSaver's json writer (egress='host') with
BURSTResultHandler, and the eval_vos route through the torch interpreter of the descriptors (tests/mock_exec.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib
from cutie_amd.config import default_config
from cutie_amd.inference.utils import coco_rle as R

import burst_fixture as BF


# ---- codec -------------------------------------------------------------------------------------------------------------------------------
def _hand_vectors():
    a = np.zeros((5, 7), dtype=np.uint8)
    a[1:4, 2:5] = 1
    b = np.zeros((4, 3), dtype=np.uint8)
    b[0, 0] = b[3, 2] = 1
    return [(np.zeros((3, 4), dtype=np.uint8), [12], '<'), (np.ones((3, 4), dtype=np.uint8), [0, 12], '0<'),
            (a, [11, 3, 2, 3, 2, 3, 11], ';320009'), (b, [0, 1, 10, 1], '01:0')]


def test_hand_vectors_both_directions():
    for mask, counts, string in _hand_vectors():
        assert R.counts_of(mask) == counts
        assert R.to_string(counts) == string and R.encode(mask) == string
        assert R.from_string(string) == counts
        got = R.decode(string, *mask.shape)
        assert got.dtype == np.uint8 and np.array_equal(got, mask)


def test_round_trips_on_random_masks():
    rng = np.random.default_rng(2024)
    for shape in ((1, 1), (1, 9), (9, 1), (37, 53)):
        for p in (0.0, 0.03, 0.5, 0.97, 1.0):
            m = (rng.random(shape) < p).astype(np.uint8)
            c = R.counts_of(m)
            assert sum(c) == m.size and all(v > 0 for v in c[1:]) and (c[0] == 0) == bool(m[0, 0])
            assert R.from_string(R.to_string(c)) == c
            assert np.array_equal(R.decode(R.encode(m), *shape), m)


def test_a_20_bit_count_and_negative_differences():
    m = np.zeros((720, 1280), dtype=np.uint8)
    m[-1, -1] = 1
    s = R.encode(m)
    assert R.from_string(s) == [720 * 1280 - 1, 1] and len(s) == 6               # 921599 needs 4 groups of 5 bits + the sign group's room
    assert np.array_equal(R.decode(s, 720, 1280), m)
    rng = np.random.default_rng(5)
    counts = [0] + [int(v) for v in rng.integers(1, 5000, size=40)]
    diffs = [counts[i] - counts[i - 2] for i in range(3, len(counts))]
    assert min(diffs) < -1024 and max(diffs) > 1024                              # several groups, both signs
    assert R.from_string(R.to_string(counts)) == counts
    for value, string in ((-1, 'O'), (-16, '@'), (-17, '_O'), (15, '?'), (16, '`0'), (31, 'o0'), (-1024, 'PPO')):
        # worked by hand from the format: c = x & 31, x >>= 5, more = x != -1 if c & 16 else x != 0, chr(c + 32 more + 48)
        assert R.to_string([0, 0, 0, value])[3:] == string, (value, R.to_string([0, 0, 0, value]))
        assert R.from_string('000' + string) == [0, 0, 0, value]
    with pytest.raises(ValueError):
        R.decode('<', 3, 5)                                                      # 12 pixels are not 3 x 5


# ---- reader ------------------------------------------------------------------------------------------------------------------------------
def test_reader_semantics(tmp_path):
    from cutie_amd.inference.data.burst_test_dataset import BURSTTestDataset
    from cutie_amd.inference.data.burst_video_reader import BURSTVideoReader
    from cutie_amd.inference.utils.results_utils import davis_palette
    import cutie.inference.data.burst_test_dataset as alias
    assert alias.BURSTTestDataset is BURSTTestDataset
    images, json_path, meta = BF.make(tmp_path)
    first = BF.first_mask()
    ds = BURSTTestDataset(images, json_path)
    assert len(ds) == 1
    rd = next(iter(ds.get_datasets()))
    assert isinstance(rd, BURSTVideoReader) and rd.vid_name == 'bike' and len(rd) == 4
    assert not rd.use_long_id and rd.get_palette() == davis_palette and rd.sequence_json == meta['sequences'][0]
    recs = [rd[i] for i in range(4)]
    assert [r['info']['frame'] for r in recs] == BF.FRAMES and [r['info']['save'] for r in recs] == [True, False, True, False]
    assert [r['info']['time_index'] for r in recs] == [0, 1, 2, 3] and all(tuple(r['info']['shape']) == (480, 854) for r in recs)
    assert not recs[0]['info']['resize_needed'] and recs[0]['rgb'].shape == (3, 480, 854) and recs[0]['rgb'].dtype == torch.float32
    assert 'mask' not in recs[1] and 'mask' not in recs[3]
    assert recs[0]['mask'].dtype == torch.int64 and np.array_equal(recs[0]['mask'].numpy(), np.where(first == 1, 1, 0))
    assert recs[0]['valid_labels'].tolist() == [1]
    assert np.array_equal(recs[2]['mask'].numpy(), np.where(first == 2, 2, 0)) and recs[2]['valid_labels'].tolist() == [2]   # the second object
    # two objects in one frame, dict order: the later one overwrites
    seq = copy.deepcopy(meta['sequences'][0])
    both = np.zeros((480, 854), dtype=np.uint8)
    both[100:200, 100:300] = 1
    seq['segmentations'][0] = {'7': {'rle': R.encode(both)}, '3': {'rle': R.encode(first == 1)}}
    d0 = BURSTVideoReader(images, seq)[0]
    want = np.where(both == 1, 7, 0)
    want[first == 1] = 3
    assert np.array_equal(d0['mask'].numpy(), want) and d0['valid_labels'].tolist() == [7, 3]
    # skip_frames: every third frame and the annotated ones, sorted
    rd3 = BURSTVideoReader(images, meta['sequences'][0], skip_frames=3)
    assert rd3.frames == ['00000.jpg', '00002.jpg', '00003.jpg'] and [rd3[i]['info']['time_index'] for i in range(3)] == [0, 1, 2]
    assert [rd3[i]['info']['save'] for i in range(3)] == [True, True, False]
    # size: every frame is resized (shorter side), the mask by nearest neighbour
    rs = BURSTVideoReader(images, meta['sequences'][0], size=120)
    r0 = rs[0]
    assert r0['info']['resize_needed'] and tuple(r0['info']['shape']) == (480, 854) and r0['rgb'].shape == (3, 120, 213)
    near = np.array(Image.fromarray(np.where(first == 1, 1, 0).astype(np.uint8)).resize((213, 120), Image.NEAREST))
    assert np.array_equal(r0['mask'].numpy(), near)
    big = BURSTVideoReader(images, meta['sequences'][0], size=600)[1]            # also upwards, unlike VideoReader
    assert big['info']['resize_needed'] and big['rgb'].shape == (3, 600, 1067)
    # the device-ingest record of the same frame
    du = rs.get(0, ingest='device')
    assert du['rgb_u8'].shape == (480, 854, 3) and du['info']['rgb_shape'] == (120, 213) and torch.equal(du['mask'], r0['mask'])
    with pytest.raises(ValueError):
        rs.get(0, ingest='gpu')


# ---- saver -------------------------------------------------------------------------------------------------------------------------------
def _saver_run(tmp_path, name, init_json, frames, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    om.add_new_objects([1, 2, 5])
    out = os.path.join(str(tmp_path), name)
    saver = ResultSaver(out, 'bike', dataset='burst-val', object_manager=om, use_long_id=False, init_json=init_json, **kw)
    for frame, prob in frames:
        saver.process(prob, frame)
    saver.end()
    return saver, out


def _probs(seed, H=40, W=56):
    """[4, H, W]: background, objects 1 and 2 as blocks, object 5 never wins"""
    rng = np.random.default_rng(seed)
    p = torch.full((4, H, W), 0.1)
    p[0] = 0.4
    y, x = int(rng.integers(0, 10)), int(rng.integers(0, 10))
    p[1, y:y + 17, x:x + 20] = 0.9
    p[2, H - 15:, W - 30 + x:] = 0.8
    p[2, :3, :2] = 0.95
    return p


def test_saver_writes_the_burst_json(tmp_path):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.burst_utils import BURSTResultHandler
    from cutie_amd.inference.utils.results_utils import ResultSaver
    import cutie.inference.utils.burst_utils as alias
    assert alias.BURSTResultHandler is BURSTResultHandler
    seq = BF.sequence('bike')
    seq['segmentations'] = [{'1': {'rle': 'given-as-input'}}, {}]
    loaded = json.loads(json.dumps(seq))                                        # keys are strings, as from a file
    frames = [(f, _probs(k)) for k, f in enumerate(BF.FRAMES)]
    saver, out = _saver_run(tmp_path, 'loaded', loaded, frames)
    lut = np.array([0, 1, 2, 5])
    assert saver.video_json['segmentations'] is saver.segmentations and 'segmentations' in saver.video_json
    assert {k: v for k, v in saver.video_json.items() if k != 'segmentations'} == {k: v for k, v in loaded.items() if k != 'segmentations'}
    assert len(saver.segmentations) == 2
    for index, frame in enumerate(BF.ANNOTATED):
        ids = lut[frames[BF.FRAMES.index(frame)][1].argmax(0).numpy()]
        seg = saver.segmentations[index]
        assert sorted(seg) == [1, 2]                                            # int keys; object 5 is empty and left out; object 1 is
        for oid in (1, 2):                                                      # ENCODED: the int 1 is not among the string keys of the input
            assert list(seg[oid]) == ['rle'] and np.array_equal(R.decode(seg[oid]['rle'], 40, 56), ids == oid)
        assert np.array_equal(np.array(Image.open(os.path.join(out, 'bike', frame[:-4] + '.png'))), ids)
    assert sorted(os.listdir(os.path.join(out, 'bike'))) == ['00000.png', '00001.png', '00002.png', '00003.png']      # save_mask is unchanged
    # an init_json built in memory with int keys: the copy branch fires for object 1 on frame 0
    mem = dict(seq, segmentations=[{1: {'rle': 'given-as-input'}}, {}])
    saver2, _ = _saver_run(tmp_path, 'mem', mem, frames)
    assert saver2.segmentations[0][1] == {'rle': 'given-as-input'} and saver2.segmentations[0][2] == saver.segmentations[0][2]
    assert saver2.segmentations[1] == saver.segmentations[1]
    # non-annotated frames alone write nothing into the json
    saver3, _ = _saver_run(tmp_path, 'none', loaded, [frames[1], frames[3]])
    assert saver3.segmentations == [{}, {}]
    # the handler: metadata kept, sequences replaced, keys become strings at dump
    meta = {'split': 'val', 'sequences': [loaded, loaded]}
    handler = BURSTResultHandler(meta)
    handler.add_sequence(saver.video_json)
    handler.dump(str(tmp_path))
    assert len(meta['sequences']) == 2                                          # the caller's json is not touched
    back = json.load(open(os.path.join(str(tmp_path), 'predictions.json')))
    assert back['split'] == 'val' and len(back['sequences']) == 1
    got = back['sequences'][0]
    assert got['annotated_image_paths'] == BF.ANNOTATED and len(got['segmentations']) == len(got['annotated_image_paths'])
    assert [sorted(s) for s in got['segmentations']] == [['1', '2'], ['1', '2']]
    assert got['segmentations'][1]['2']['rle'] == saver.segmentations[1][2]['rle']
    # refusals
    om = ObjectManager()
    with pytest.raises(NotImplementedError, match='init_json'):
        ResultSaver(out, 'v', dataset='burst-val', object_manager=om, use_long_id=False)
    s4 = ResultSaver(out, 'v', dataset='burst-test', object_manager=om, use_long_id=False, init_json=loaded, processor=object())
    with pytest.raises(ValueError, match='BURST'):
        s4.process_merged([_probs(0)], '00000.jpg', (40, 56))
    s4.end()


# ---- driver ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def product_net():
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    from mock_exec import MockExecutor
    mx = MockExecutor()
    mx.per_sample_conv = True
    _lib.set_executor_for_testing(mx)
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net
    _lib.set_executor_for_testing(None)


def _args(argv):
    from cutie_amd import eval_vos as E
    ap = E.arg_parser()
    args = ap.parse_args(argv)
    E.check_args(ap, args)
    return args


def check_predictions(out, names, hw=(480, 854)):
    """predictions.json of a run over BF.make(names): layout, and every RLE string is the PNG of its frame"""
    pred = json.load(open(os.path.join(out, 'predictions.json')))
    assert pred['split'] == 'val' and [s['seq_name'] for s in pred['sequences']] == list(names)
    for seq in pred['sequences']:
        assert seq['annotated_image_paths'] == BF.ANNOTATED and len(seq['segmentations']) == 2 and seq['dataset'] == BF.DATASET
        assert sorted(os.listdir(os.path.join(out, 'Annotations', seq['seq_name']))) == ['00000.png', '00002.png']   # save_all is False
        assert sorted(seq['segmentations'][0]) == ['1'] and set(seq['segmentations'][1]) <= {'1', '2'} and '2' in seq['segmentations'][1]
        for frame, seg in zip(BF.ANNOTATED, seq['segmentations']):
            png = np.array(Image.open(os.path.join(out, 'Annotations', seq['seq_name'], frame[:-4] + '.png')))
            assert png.shape == hw and sorted(int(k) for k in seg) == [int(v) for v in np.unique(png) if v != 0]
            for oid, s in seg.items():
                assert np.array_equal(R.decode(s['rle'], *hw), png == int(oid)), (frame, oid)
    return pred


def test_eval_vos_burst_route(tmp_path, product_net, capsys):
    from cutie_amd import eval_vos as E
    images, json_path, _ = BF.make(tmp_path, names=('bikeA', 'bikeB'))
    base = ['--dataset', 'burst-val', '--images', images, '--json', json_path, '--size', '64']
    cfg = default_config(mem_every=2)
    out = os.path.join(str(tmp_path), 'out')
    res = E.run_dataset(product_net, cfg, _args(base + ['--output', out]))
    assert sorted(res) == [0, 1] and all(r['frames'] == 4 for r in res.values())
    pred = check_predictions(out, ('bikeA', 'bikeB'))
    first = BF.first_mask()                                                     # the first frame comes back as its input mask, at the 64-pixel size's precision
    got = R.decode(pred['sequences'][0]['segmentations'][0]['1']['rle'], 480, 854)
    assert (got != (first == 1)).mean() < 0.02
    out2 = os.path.join(str(tmp_path), 'ls')
    res2 = E.run_dataset(product_net, cfg, _args(base + ['--output', out2, '--lockstep', '2']))
    assert sorted(res2) == [0, 1]
    assert check_predictions(out2, ('bikeA', 'bikeB')) == pred                  # one saver per clip, the same strings
    for bad, word in ((['--dataset', 'burst-val', '--images', images, '--output', out], '--json'),
                      (base + ['--output', out, '--sizes', '240', '320'], '--sizes'),
                      (['--images', images, '--output', out], '--masks')):
        with pytest.raises(SystemExit) as e:
            _args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err
