"""Times the distance stage (PROB_TO_ID flags == 4096, csrc/edt.hip) on one MI355X and writes profiles/edt.md:

(1) the stage with cutie_time_ops at 854x480 and 1920x1080 on a three-blob mask and on 0.5-density noise, for the radii 4, 16, 64 and
    255 (limit = r^2 + 1, band only, as the saver runs it) with S = 1 and S = 3 sets, next to the region filter and the track statistics
    on planes of the same size, re-measured in the same process;
(2) the experiment of DESIGN.md section 15: eval_vos.run_dataset over four copies of a 96-frame 854x480 clip with --egress device
    --lockstep 4, wall-clock frames/s of the second pass, without the options, with --trimap 4 12 and -- with --parent DIR, a built
    checkout of the parent commit -- the parent's run; every sample in a fresh process, the legs interleaved, their order rotating
    from round to round.

    python tools/edt_probe.py [--frames 96] [--rounds 3] [--parent DIR] [--out profiles/edt.md]

Needs the GPU (no fall-back)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from tools.region_probe import planes        # noqa: E402  (the same planes as profiles/region_filter.md)
from tools.track_probe import clips          # noqa: E402  (the same clips as profiles/track_report.md)

RADII = (4, 16, 64, 255)


def stage_rows(iters=50):
    from cutie_amd import _lib, ops as O
    rows = []
    ex = _lib.get_executor()

    def timed(ol):
        arr = ol.finalize()
        us = [ex.time_ops(arr, iters) * 1e3 for _ in range(5)]
        return f'{statistics.median(us):.1f} | {min(us):.1f} - {max(us):.1f}'
    for H, W in ((480, 854), (1080, 1920)):
        named = dict((n, p) for n, p in planes(H, W))
        blobs = torch.from_numpy(named['three blobs']).cuda()
        table = torch.empty((3, 12), dtype=torch.int32, device='cuda')
        ol = O.OpList()
        ol.track_stats(blobs, [1, 2, 3], table)
        rows.append(f'| {W}x{H} | three blobs | track statistics, id plane only (3 launches) | {timed(ol)} |')
        ids = blobs.clone()
        ol = O.OpList()
        ol.region_filter(ids, torch.empty(O.OpList.region_scratch_words(H, W), dtype=torch.int32, device='cuda'),
                         torch.empty(4, dtype=torch.int32, device='cuda'), min_region=64, connectivity=8)
        rows.append(f'| {W}x{H} | three blobs | region filter A, islands (4 launches) | {timed(ol)} |')
        for name in ('three blobs', '0.5-density noise'):
            src = torch.from_numpy(named[name]).cuda()
            for S in (1, 3):
                sets = np.zeros((S, 256), dtype=np.uint8)
                sets[0, 1:] = 1                  # the union; then single objects
                for s in range(1, S):
                    sets[s, s] = 1
                sets_dev = torch.from_numpy(sets).cuda()
                scratch = torch.empty(O.OpList.edt_scratch_words(S, H, W), dtype=torch.int32, device='cuda')
                band = torch.empty((S, H, W), dtype=torch.uint8, device='cuda')
                for r in RADII:
                    ol = O.OpList()
                    ol.edt_band(src, sets_dev, scratch, band=band, inner=r * r, outer=r * r, mid=128)
                    rows.append(f'| {W}x{H} | {name} | distance stage, radius {r}, S = {S} (2 launches) | {timed(ol)} |')
    return rows


# one sample -- run_dataset twice, the second pass timed -- in a process of its own, from whatever tree is the working directory
LEG = '''
import json, os, shutil, sys, time, torch
sys.path.insert(0, '.')
from cutie_amd import eval_vos as E
from cutie_amd.config import default_config
from cutie_amd.model.cutie import CUTIE
from oracle import scenarios as S
root, frames, extra = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
cfg = default_config()
net = CUTIE(cfg).cuda().eval()
net.load_weights(S.decisive_state_dict())
out = os.path.join(root, 'out_leg')
ap = E.arg_parser()
args = ap.parse_args(['--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations'), '--output', out,
                      '--dataset', 'd17-val', '--egress', 'device', '--lockstep', '4'] + extra)
E.check_args(ap, args)
for _ in range(2):
    shutil.rmtree(out, ignore_errors=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = E.run_dataset(net, cfg, args)
    torch.cuda.synchronize(); fps = 4 * frames / (time.perf_counter() - t0)
trimaps = sum(len(os.listdir(os.path.join(out, 'Annotations', v, 'trimap'))) for v in os.listdir(os.path.join(out, 'Annotations'))
              if os.path.isdir(os.path.join(out, 'Annotations', v, 'trimap')))
print('LEG ' + json.dumps({'fps': fps, 'trimaps': trimaps}))
'''

TRIMAP = ['--trimap', '4', '12']


def leg(tree, root, frames, extra):
    p = subprocess.run([sys.executable, '-c', LEG, root, str(frames)] + extra, cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f'leg {extra} in {tree} failed ({p.returncode}): {p.stderr[-2000:]}')
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('LEG ')][-1][4:])
    assert r['trimaps'] == (4 * frames if extra else 0), r
    return r['fps']


def run_rows(frames, rounds, parent):
    legs = [('this tree, no options', ROOT, []), ('this tree, --trimap 4 12', ROOT, TRIMAP)]
    if parent:
        legs += [('parent commit', os.path.abspath(parent), [])]
    fps = {name: [] for name, _, _ in legs}
    root = tempfile.mkdtemp(prefix='edt_probe_')
    try:
        clips(root, frames)
        for k in range(rounds):                  # (the order rotates: every leg runs first, second, ... in turn)
            for name, tree, extra in legs[k % len(legs):] + legs[:k % len(legs)]:
                fps[name].append(leg(tree, root, frames, extra))
                print(f'{name}: {fps[name][-1]:.1f} frames/s', flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return [f'| {name} | ' + ' / '.join(f'{v:.1f}' for v in vs) + f' | {statistics.median(vs):.1f} |' for name, vs in fps.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edt.md'))
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its runs are measured next to this tree\'s')
    ap.add_argument('--notes', help='a file whose text is appended (what the figures mean)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'edt_probe needs the MI355X'
    lines = ['# Distance transform and bands: tools/edt_probe.py', '', f'device: {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} CPUs', '',
             'Stage time: cutie_time_ops, 50 back-to-back replays (warm caches), median of 5 (min - max), microseconds per replay of the whole chain; '
             'limit = r^2 + 1, band output only.', '',
             '| size | plane | launches | us | min - max |', '|---|---|---|---|---|'] + stage_rows()
    lines += ['', f'eval_vos.run_dataset over 4 clips of {args.frames} frames of 854x480 (--egress device --lockstep 4), wall-clock frames/s of the second pass; '
              f'every sample in a fresh process, the legs interleaved and their order rotating, {args.rounds} rounds:', '', '| run | frames/s per round | median |', '|---|---|---|']
    lines += run_rows(args.frames, args.rounds, args.parent)
    if not args.parent:
        lines += ['', 'No parent checkout was given (--parent): the parent commit\'s legs were not measured in this run.']
    if args.notes:
        lines += ['', open(args.notes).read().rstrip('\n')]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
