"""Lock step for clips with DIFFERENT object counts (LockstepCores(mixed_objects=True), plans built with clips=(K_0, K_1, ..)) without a GPU:
the host wiring through the descriptor interpreter with the mixed forms (tests/mock_exec_mixed.py) -- every clip of a mixed group gets the
probabilities and the bank of its own InferenceCore run, bit for bit, on ONE plan per stage."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib
from cutie_amd.config import default_config
from cutie_amd.inference.utils.results_utils import davis_palette
from oracle import scenarios as S
from oracle.weights import make_state_dict

from mock_exec_mixed import MixedMockExecutor

SIZE = (48, 80)


@pytest.fixture(scope='module')
def product_net():
    from cutie_amd.model.cutie import CUTIE
    mx = MixedMockExecutor()
    mx.per_sample_conv = True          # (torch's CPU conv may sum differently per batch size; the HIP tiles of one K-order class do not)
    _lib.set_executor_for_testing(mx)
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net
    _lib.set_executor_for_testing(None)


def _banks(proc):
    return {k: (b.n_long, b.n_perm, b.n_work) for k, b in proc.memory.buckets.items()}


def _clips(counts, T, seed):
    from cutie_amd.utils.synth import SyntheticClip
    clips = [SyntheticClip(SIZE[0], SIZE[1], k, T, seed=seed + c) for c, k in enumerate(counts)]
    return clips, [[cl.frame(t) for t in range(T)] for cl in clips]


def _mixed_case(net, cfg_kw, counts, T, hinted, mixed_objects=True, window=None):
    """(sequential per-clip (probabilities, bank), lock-step ones, LockstepCores): test_host_wiring_cpu._lockstep_case with a count per clip."""
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.inference.lockstep import LockstepCores
    clips, frames = _clips(counts, T, 140)
    C = len(counts)
    seq = []
    for c, cl in enumerate(clips):
        proc = InferenceCore(net, cfg=default_config(**cfg_kw))
        outs = [proc.step(frames[c][0], cl.first_mask(), objects=cl.objects)]
        for t in range(1, T):
            outs.append(proc.step(frames[c][t], end=(t == T - 1)))
        seq.append((torch.stack(outs), _banks(proc)))
    ls = LockstepCores(net, default_config(**cfg_kw), C, mixed_objects=mixed_objects)
    if window is not None:
        ls.WINDOW, ls.WINDOW_LEAD = window
    outs = [ls.step([f[0] for f in frames], [cl.first_mask() for cl in clips], [cl.objects for cl in clips])]
    for t in range(1, T):
        hint = dict(next_images=[f[t + 1:t + 10] for f in frames]) if hinted and t + 1 < T else {}
        outs.append(ls.step([f[t] for f in frames], end=(t == T - 1), **hint))
    got = [(torch.stack([o[c] for o in outs]), _banks(ls.cores[c])) for c in range(C)]
    return seq, got, ls


CASES = [((1, 3, 2), dict(mem_every=3), 9),
         ((7, 1), dict(mem_every=2, use_long_term=True, long_term=dict(S.LT_SMALL)), 15)]


@pytest.mark.parametrize('hinted', [False, True])
@pytest.mark.parametrize('counts, cfg_kw, T', CASES, ids=['1-3-2', '7-1-longterm'])
def test_mixed_group_matches_every_clips_own_run(product_net, counts, cfg_kw, T, hinted):
    """Counts (1, 3, 2) with FIFO memory and (7, 1) with long-term memory and consolidations, with and without look-ahead hints: every frame
    but the first (masks) and the last (end=True) is one plan per stage, and every clip has the bits and the bank of its own run."""
    with torch.inference_mode():
        seq, got, ls = _mixed_case(product_net, cfg_kw, counts, T, hinted, window=(4, 1) if hinted else None)
    assert ls.batched_steps == T - 2, ls.batched_steps
    assert ls.joint_passes == 0 and ls.stacked_steps == 0           # (a mixed group reads every bank in its clip's own lane)
    assert not cfg_kw.get('use_long_term') or all(v[0] > 0 for v in seq[0][1].values()), 'the long-term case must consolidate'
    for c in range(len(counts)):
        assert seq[c][0].shape[1] == counts[c] + 1
        assert seq[c][1] == got[c][1], (counts, c, seq[c][1], got[c][1])
        assert torch.equal(seq[c][0], got[c][0]), (counts, hinted, c, float((seq[c][0] - got[c][0]).abs().max()))


def test_without_the_switch_a_mixed_group_runs_clip_by_clip(product_net):
    """mixed_objects=False is the behaviour from before: clips that differ in their object count never share a plan (and still get their bits)."""
    counts, cfg_kw, T = CASES[0]
    with torch.inference_mode():
        seq, got, ls = _mixed_case(product_net, cfg_kw, counts, T, True, mixed_objects=False)
    assert ls.batched_steps == 0
    for c in range(len(counts)):
        assert torch.equal(seq[c][0], got[c][0]) and seq[c][1] == got[c][1]


def test_a_clip_that_loses_an_object_comes_back_to_the_batched_path(product_net):
    """A uniform group of 2 x 3 objects, delete_objects([[3], []]) in the middle: the step behind the deletion runs clip by clip (the last
    mask of clip 0 still carries the plane), the one after it is batched again -- now as a group of (2, 3) objects.  Both clips match
    their own runs."""
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.inference.lockstep import LockstepCores
    T, cfg_kw = 10, dict(mem_every=2)
    clips, frames = _clips((3, 3), T, 180)
    dele = [[3], []]
    with torch.inference_mode():
        seq = []
        for c, cl in enumerate(clips):
            proc = InferenceCore(product_net, cfg=default_config(**cfg_kw))
            outs = [proc.step(frames[c][0], cl.first_mask(), objects=cl.objects)]
            for t in range(1, T):
                if t == 5 and dele[c]:
                    proc.delete_objects(dele[c])
                outs.append(proc.step(frames[c][t]))
            seq.append(outs)
        ls = LockstepCores(product_net, default_config(**cfg_kw), 2, mixed_objects=True)
        got, steps = [ls.step([f[0] for f in frames], [cl.first_mask() for cl in clips], [cl.objects for cl in clips])], [0]
        for t in range(1, T):
            if t == 5:
                ls.delete_objects(dele)
            got.append(ls.step([f[t] for f in frames], **(dict(next_images=[f[t + 1:t + 6] for f in frames]) if t + 1 < T else {})))
            steps.append(ls.batched_steps)
    # batched: t = 1..4 (3 + 3 objects); clip by clip: t = 0 (masks) and t = 5 (the deletion); batched again from t = 6 (2 + 3 objects)
    assert steps == [0, 1, 2, 3, 4, 4, 5, 6, 7, 8], steps
    for c in range(2):
        for t in range(T):
            assert got[t][c].shape == seq[c][t].shape and torch.equal(got[t][c], seq[c][t]), (c, t)
    assert got[4][0].shape[0] == 4 and got[6][0].shape[0] == 3


def test_mixed_plans_have_the_launches_of_the_uniform_plans(product_net):
    """Counts (1, 3, 2) against three clips of 2 objects: the four plans of a mixed group hold as many launches as the uniform ones, plus
    the one copy per fusion block (pixel fuser, mask encoder) that expands the per-clip x_transform maps to a map per object
    (plans.MIXED_FUSION_EXTRA) -- the tile table holds no entry for these sizes, so no conv is cut at a K-order boundary."""
    from cutie_amd.model import plans
    from cutie_amd.ops import COPY2D
    assert plans.MIXED_FUSION_EXTRA == 1
    eng = product_net.engine()
    h, w = SIZE[0] // 16, SIZE[1] // 16
    H, W = SIZE
    builders = [(plans.build_pixel_fusion, lambda cl: (2, h, w, True, True, cl, 1, False), 1),
                (plans.build_pixel_fusion, lambda cl: (2, h, w, True, False, cl, 1, False), 1),
                (plans.build_readout_query, lambda cl: (2, h, w, False, True, cl), 0),
                (plans.build_segment, lambda cl: (2, h, w, True, True, True, cl, 1), 0),
                (plans.build_encode_mask, lambda cl: (2, H, W, H, W, 0, 0, True, True, cl, 1), 1)]
    for build, args, blocks in builders:
        uni, mix = build(eng, *args(3)), build(eng, *args((1, 3, 2)))
        assert len(mix.ol) == len(uni.ol) + blocks * plans.MIXED_FUSION_EXTRA, (build.__name__, len(mix.ol), len(uni.ol))
        assert sum(r[0] == COPY2D for r in mix.ol.recs) == blocks and mix.kref and all(k == 1 for k in mix.kref.values())      # (no conv cut: every one a twin of clip 0's plan)
    # equal counts handed over as a tuple ARE the uniform group
    same = plans.build_segment(eng, 2, h, w, True, True, True, (2, 2, 2), 1)
    assert same.mixed is None and same.korder_ref == 3 and len(same.ol) == len(plans.build_segment(eng, 2, h, w, True, True, True, 3, 1).ol)


def test_convs_are_cut_where_the_one_clip_tiles_sum_in_different_orders(product_net):
    """plans.Plan.conv: a clip's one-clip plan takes its conv tiles from the tile table by ITS geometry, and tiles of different K-order classes
    do not give the same bits.  With a table that puts the 3x3 convs of a 1-object clip on a halo tile (and leaves the others on the
    static stream tiles), the group (1, 3, 2) runs those convs as two launches -- clip 0 alone, clips 1 and 2 together -- and the
    launches' object ranges tile the group."""
    from cutie_amd import ops as O
    from cutie_amd.model import plans
    eng = product_net.engine()
    h, w = SIZE[0] // 16, SIZE[1] // 16
    base = plans.build_pixel_fusion(eng, 2, h, w, True, True, (1, 3, 2), 1, False)
    saved = dict(eng.tile_cache)
    try:
        for n, r in enumerate(base.ol.recs):
            i = r[2]
            if r[0] == O.CONV and i[11] == 3 and i[0] == 6:                       # the 3x3 convs over the whole group: their one-object geometry -> a halo tile
                eng.tile_cache[(1 * i[7] * i[8], i[9], i[3] + i[4], 3, i[13], r[1] & 3, i[1], i[2])] = (125, 1)
        cut = plans.build_pixel_fusion(eng, 2, h, w, True, True, (1, 3, 2), 1, False)
    finally:
        eng.tile_cache.clear()
        eng.tile_cache.update(saved)
    n3 = sum(r[0] == O.CONV and r[2][11] == 3 for r in base.ol.recs)
    assert n3 == 4 and len(cut.ol) == len(base.ol) + n3
    b3 = [r[2][0] for r in cut.ol.recs if r[0] == O.CONV and r[2][11] == 3]
    assert b3 == [1, 5] * n3
    assert sorted(cut.kref.values()) == [1] * (len(cut.kref) - n3) + [3] * n3     # (the launches over clips 1, 2 follow the 3-object plan; the uncut ones clip 0's)


def _make_video(root, name, n, ids, seed):
    from cutie_amd.utils.synth import SyntheticClip
    clip = SyntheticClip(64, 96, len(ids), n, seed=seed)
    os.makedirs(os.path.join(root, 'JPEGImages', name)); os.makedirs(os.path.join(root, 'Annotations', name))
    for t in range(n):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'JPEGImages', name, f'{t:05d}.jpg'), quality=95)
    lut = np.zeros(256, dtype=np.uint8)
    for k, oid in enumerate(ids):
        lut[k + 1] = oid
    png = Image.fromarray(lut[clip.first_mask().numpy()].astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'Annotations', name, '00000.png'))


def test_eval_vos_lockstep_mixed_writes_the_pngs_of_the_plain_run(tmp_path, product_net, monkeypatch):
    """eval_vos --lockstep 3 --lockstep-mixed over three videos of 1, 2 and 3 objects: ONE group (sorted by object count), the PNG bytes
    of the run without --lockstep; without --lockstep-mixed the three videos form no group at all."""
    from cutie_amd import eval_vos as E
    root = str(tmp_path)
    _make_video(root, 'vA', 5, (1, 2, 3), 31)
    _make_video(root, 'vB', 6, (4,), 32)
    _make_video(root, 'vC', 5, (2, 7), 33)
    base = ['--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations')]

    def args(extra, out):
        ap = E.arg_parser()
        a = ap.parse_args(base + ['--output', os.path.join(root, out)] + extra)
        E.check_args(ap, a)
        return a
    groups = []
    real = E.process_videos_lockstep

    def spy(network, cfg, vid_readers, *a, **kw):
        groups.append(([rd.vid_name for rd in vid_readers], kw.get('mixed_objects')))
        return real(network, cfg, vid_readers, *a, **kw)
    monkeypatch.setattr(E, 'process_videos_lockstep', spy)
    cfg = default_config(mem_every=2)
    assert not args([], 'x').lockstep_mixed
    res = E.run_dataset(product_net, cfg, args([], 'plain'))
    assert sorted(res) == [0, 1, 2] and not groups
    E.run_dataset(product_net, cfg, args(['--lockstep', '3'], 'uniform'))
    assert not groups                                                   # (three object counts: no two videos share lockstep_key)
    res = E.run_dataset(product_net, cfg, args(['--lockstep', '3', '--lockstep-mixed'], 'mixed'))
    assert groups == [(['vB', 'vC', 'vA'], True)], groups               # one group, by object count
    assert sorted(res) == [0, 1, 2] and [res[c]['frames'] for c in range(3)] == [5, 6, 5]
    for n, T in (('vA', 5), ('vB', 6), ('vC', 5)):
        fa = sorted(os.listdir(os.path.join(root, 'plain', 'Annotations', n)))
        assert fa == sorted(os.listdir(os.path.join(root, 'mixed', 'Annotations', n))) and len(fa) == T
        for f in fa:
            assert open(os.path.join(root, 'plain', 'Annotations', n, f), 'rb').read() == \
                open(os.path.join(root, 'mixed', 'Annotations', n, f), 'rb').read(), (n, f)
    rds = {rd.vid_name: rd for rd in E.VOSTestDataset(base[1], base[3], use_all_masks=False).get_datasets()}
    assert E.lockstep_key(rds['vA']) == ((64, 96), 3, False) and E.lockstep_key_mixed(rds['vA']) == E.lockstep_key_mixed(rds['vB']) == ((64, 96), False)
