"""Score probe: what the J&F counts of one frame cost on each route, and what `eval_vos --score` costs a run.  Writes
profiles/score_probe.md (header, tables and the figures derived from them).

    python tools/score_probe.py [--iters 200] [--frames 96] [--parent ROWS.md] [--out profiles/score_probe.md]
    python tools/score_probe.py --baseline --out ROWS.md        (in a checkout WITHOUT --score, e.g. the parent commit, with this file copied in)

  device   the stage alone (PROB_TO_ID flags == 64, three launches) over two id planes on the GPU: cutie_time_ops, median of 5 replays --
           at 480 x 854 with 3 objects and r = 8, and at 1080 x 1920 with 5 objects and r = 18
  host     what scoring the same frame away from the GPU pays: a blocking copy of the predicted plane to the host + the numpy / scipy
           model of the tests (tests/jf_ref.py); wall clock, median of 5
  decode   what SequenceScorer.add pays on the issuing thread per frame whatever the route: PIL's decode of the ground-truth PNG
  run      wall-clock frames/s of eval_vos.run_dataset over a local clip (the tests/golden/bike frames repeated to --frames frames, ground
           truth = shifted copies of the first mask) with and without --score, host and device egress; the second pass of each is kept
The counts of both routes are compared before anything is timed.
--baseline times the plain runs alone and writes their table rows to --out: that is what a checkout of the parent commit can run;
--parent ROWS.md puts those rows into the file next to this tree's, so the cost of --score and of carrying the feature are both on record."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

CASES = ((480, 854, 3, 8), (1080, 1920, 5, 18))


def planes(H, W, K, seed):
    """smooth blobs of K objects and a copy moved by a few pixels"""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.interpolate(torch.randn(1, K + 1, max(H // 60, 2), max(W // 60, 2), generator=g), size=(H, W), mode='bicubic',
                                        align_corners=False)[0]
    gt = x.argmax(0).to(torch.uint8).numpy()
    pred = np.roll(gt, (3, 5), (0, 1))
    return np.ascontiguousarray(pred), gt


def gt_decode_us(gt):
    """median wall time of davis_metrics.load_ids over a palette PNG of this plane"""
    from PIL import Image
    from cutie_amd.inference.utils.davis_metrics import load_ids
    fd, name = tempfile.mkstemp(suffix='.png')
    os.close(fd)
    try:
        im = Image.fromarray(gt)
        im.putpalette(bytes(range(256)) * 3)
        im.save(name)
        load_ids(name)
        ts = []
        for _ in range(9):
            t0 = time.perf_counter()
            load_ids(name)
            ts.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(ts)
    finally:
        os.remove(name)


def stage(iters):
    from cutie_amd import _lib, ops as O
    import jf_ref as R
    rows = []
    for H, W, K, r in CASES:
        pred, gt = planes(H, W, K, seed=H)
        objects = list(range(1, K + 1))
        pd, gd = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        counts = torch.empty((K, 8), dtype=torch.int32, device='cuda')
        scratch = torch.empty(O.OpList.jf_scratch_words(H, W, K), dtype=torch.int32, device='cuda')
        ol = O.OpList()
        ol.jf_counts(pd, gd, objects, counts, scratch, H=H, W=W, radius=r)
        arr = ol.finalize()
        ol.run()
        torch.cuda.synchronize()
        want = R.counts(pred, gt, objects, r)
        assert np.array_equal(counts.cpu().numpy(), want), (counts.cpu().tolist(), want.tolist())
        dev_us = statistics.median(_lib.get_executor().time_ops(arr, iters) for _ in range(5)) * 1e3

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = pd.cpu().numpy()
            t1 = time.perf_counter()
            R.counts(m, gt, objects, r)
            return (t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6
        host_route()
        runs = [host_route() for _ in range(5)]
        copy_us, model_us = statistics.median(v[0] for v in runs), statistics.median(v[1] for v in runs)
        decode_us = gt_decode_us(gt)
        rows += [f'| {W}x{H}, {K} objects, r = {r}: {int(want[:, 2].sum())} + {int(want[:, 3].sum())} boundary pixels | us per frame |', '|---|---|',
                 f'| device: the stage alone (cutie_time_ops, {iters} iterations, median of 5) | {dev_us:.1f} |',
                 f'| host: blocking copy of the predicted plane | {copy_us:.1f} |',
                 f'| host: numpy / scipy model over the {K} objects | {model_us:.1f} |',
                 f'| host: both | {copy_us + model_us:.1f} |',
                 f'| either route: PIL decode of the ground-truth PNG on the issuing thread (SequenceScorer.add) | {decode_us:.1f} |', '']
    return rows


def clip(root, frames):
    from PIL import Image
    src = os.path.join(HERE, '..', 'tests', 'golden', 'bike')
    first = Image.open(os.path.join(src, '00000.png'))
    ids = np.array(first)
    img, msk, gt = (os.path.join(root, d, 'bike') for d in ('JPEGImages', 'Annotations', 'GT'))
    for d in (img, msk, gt):
        os.makedirs(d)
    shutil.copy(os.path.join(src, '00000.png'), msk)
    for t in range(frames):
        k = t % 4 if (t // 4) % 2 == 0 else 3 - t % 4             # 0 1 2 3 3 2 1 0 ...: no jump in the clip
        shutil.copy(os.path.join(src, f'0000{k}.jpg'), os.path.join(img, f'{t:05d}.jpg'))
        im = Image.fromarray(np.roll(ids, (2 * k, 5 * k), (0, 1)))
        im.putpalette(first.getpalette())
        im.save(os.path.join(gt, f'{t:05d}.png'))


def runs(frames, baseline):
    from cutie_amd import eval_vos as E
    from cutie_amd.config import default_config
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    cfg = default_config()
    net = CUTIE(cfg).cuda().eval()
    net.load_weights(S.decisive_state_dict())
    root = tempfile.mkdtemp(prefix='score_probe_')
    rows = [f"| {'parent commit: ' if baseline else ''}eval_vos.run_dataset, {frames} frames of 854x480, wall clock of the second pass | frames/s |", '|---|---|']
    try:
        clip(root, frames)
        for egress in ('host', 'device'):
            for score in ((False,) if baseline else (False, True)):
                argv = ['--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations'), '--output',
                        os.path.join(root, f'out_{egress}_{int(score)}'), '--dataset', 'd17-val', '--egress', egress]
                if score:
                    argv += ['--score', '--gt', os.path.join(root, 'GT')]
                ap = E.arg_parser()
                args = ap.parse_args(argv)
                E.check_args(ap, args)
                best = None
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    E.run_dataset(net, cfg, args)
                    torch.cuda.synchronize()
                    best = frames / (time.perf_counter() - t0)
                rows.append(f"| --egress {egress}{' --score' if score else ''} | {best:.1f} |")
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return rows + ['']


HEADER = """# Score probe: the J&F counts of one frame, device stage against the host route, and what `--score` costs a run

Written by `python tools/score_probe.py` on one MI355X.  The planes are the argmax of smooth random logits (ground truth) and a copy moved by
(3, 5) pixels (prediction).  `device` is the stage alone (`PROB_TO_ID flags == 64`: clear, pack, match) timed with `cutie_time_ops`; `host` is
what scoring the same frame away from the GPU pays, a blocking copy of the predicted plane plus the numpy / scipy model of
`tests/jf_ref.py`; the PNG decode of the ground truth is paid by `SequenceScorer.add` on the issuing thread on either route.  The counts of
both routes are compared before anything is timed.  The `eval_vos` rows are wall-clock frames/s of `run_dataset` (decode, inference, egress
and, with `--score`, ground-truth decode + upload + the stage + the result files) over the `tests/golden/bike` frames repeated, second pass.

"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--no-run', action='store_true', help='the stage tables only')
    ap.add_argument('--baseline', action='store_true', help='only the plain eval_vos runs, as raw table rows (what a checkout without --score can measure)')
    ap.add_argument('--parent', help="the rows a --baseline run of the parent commit wrote: they join this tree's in the file")
    ap.add_argument('--out', help='default: profiles/score_probe.md (with --baseline: required)')
    a = ap.parse_args()
    if a.baseline:
        text = '\n'.join(runs(a.frames, True)) + '\n'
        print(text)
        with open(a.out, 'w') as f:
            f.write(text)
        return
    rows = stage(a.iters)
    if not a.no_run:
        rows += runs(a.frames, False)
    if a.parent:
        rows += open(a.parent).read().rstrip('\n').split('\n') + ['']
    text = HEADER + '\n'.join(rows) + '\n'
    print(text)
    out = a.out or os.path.join(HERE, '..', 'profiles', 'score_probe.md')
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
