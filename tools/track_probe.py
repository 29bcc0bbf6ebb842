"""Times the track statistics (PROB_TO_ID flags == 1024, csrc/tracks.hip) on one MI355X and writes profiles/track_report.md:

(1) the stage with cutie_time_ops at 854x480 and 1920x1080 with 3 objects -- the whole chain with the probability planes, the chain
    without them (geometry only) -- next to the plain PROB_TO_ID kernel on the same planes, which reads the same probability bytes;
(2) the experiment of DESIGN.md section 15: eval_vos.run_dataset over four copies of a 96-frame 854x480 clip (device egress), wall-clock
    frames/s of the second pass, without and with --tracks, and -- with --parent DIR, a built checkout of the parent commit -- the parent's
    run without it; every sample in a fresh process, the legs interleaved, three rounds.

    python tools/track_probe.py [--frames 96] [--rounds 3] [--parent DIR] [--out profiles/track_report.md]

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
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)


def stage_rows(iters=200):
    from cutie_amd import _lib, ops as O
    rows = []
    ex = _lib.get_executor()
    for H, W in ((480, 854), (1080, 1920)):
        K = 3
        g = torch.Generator().manual_seed(H)
        low = torch.randn(K + 1, H // 16, W // 16 + 1, generator=g) * 3
        prob = torch.softmax(torch.nn.functional.interpolate(low[None], size=(H, W), mode='bilinear')[0], 0).cuda().contiguous()
        lut = torch.arange(K + 1, dtype=torch.int32).cuda()
        ids = torch.empty((H, W), dtype=torch.uint8, device='cuda')
        table = torch.empty((K, 12), dtype=torch.int32, device='cuda')
        lists = {}
        ol = O.OpList()
        ol.prob_to_id(prob, lut, ids, P=K + 1, H=H, W=W, plane=prob.stride(0), ldrow=prob.stride(1))
        lists['plain PROB_TO_ID (the yardstick: the same probability bytes)'] = ol
        ol.run()
        ol = O.OpList()
        ol.track_stats(ids, list(range(1, K + 1)), table, prob=prob, lut=lut)
        lists['track statistics, with the probability planes (4 launches)'] = ol
        ol = O.OpList()
        ol.track_stats(ids, list(range(1, K + 1)), table)
        lists['track statistics, id plane only (3 launches)'] = ol
        for name, ol in lists.items():
            arr = ol.finalize()
            us = [ex.time_ops(arr, iters) * 1e3 for _ in range(5)]
            rows.append(f'| {W}x{H}, {K} objects | {name} | {statistics.median(us):.1f} | {min(us):.1f} - {max(us):.1f} |')
    return rows


def clips(root, frames, copies=4):
    """`copies` videos of `frames` frames: the tests/golden/bike frames back and forth"""
    src = os.path.join(ROOT, 'tests', 'golden', 'bike')
    for c in range(copies):
        img, msk = (os.path.join(root, d, f'bike{c}') for d in ('JPEGImages', 'Annotations'))
        os.makedirs(img)
        os.makedirs(msk)
        shutil.copy(os.path.join(src, '00000.png'), msk)
        for t in range(frames):
            k = t % 4 if (t // 4) % 2 == 0 else 3 - t % 4
            shutil.copy(os.path.join(src, f'0000{k}.jpg'), os.path.join(img, f'{t:05d}.jpg'))


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
                      '--dataset', 'd17-val', '--egress', 'device'] + extra)
E.check_args(ap, args)
for _ in range(2):
    shutil.rmtree(out, ignore_errors=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    E.run_dataset(net, cfg, args)
    torch.cuda.synchronize(); fps = 4 * frames / (time.perf_counter() - t0)
print('LEG ' + json.dumps({'fps': fps, 'tracks': os.path.isdir(os.path.join(out, 'tracks'))}))
'''


def leg(tree, root, frames, extra):
    p = subprocess.run([sys.executable, '-c', LEG, root, str(frames)] + extra, cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f'leg {extra} in {tree} failed ({p.returncode}): {p.stderr[-2000:]}')
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('LEG ')][-1][4:])
    assert r['tracks'] == ('--tracks' in extra)
    return r['fps']


def run_rows(frames, rounds, parent):
    legs = [('this tree, one clip at a time, no --tracks', ROOT, []), ('this tree, one clip at a time, --tracks', ROOT, ['--tracks']),
            ('this tree, --lockstep 4, no --tracks', ROOT, ['--lockstep', '4']), ('this tree, --lockstep 4, --tracks', ROOT, ['--lockstep', '4', '--tracks'])]
    if parent:
        legs += [('parent commit, one clip at a time', os.path.abspath(parent), []), ('parent commit, --lockstep 4', os.path.abspath(parent), ['--lockstep', '4'])]
    fps = {name: [] for name, _, _ in legs}
    root = tempfile.mkdtemp(prefix='track_probe_')
    try:
        clips(root, frames)
        for _ in range(rounds):
            for name, tree, extra in legs:
                fps[name].append(leg(tree, root, frames, extra))
                print(f'{name}: {fps[name][-1]:.1f} frames/s', flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return [f'| {name} | ' + ' / '.join(f'{v:.1f}' for v in vs) + f' | {statistics.median(vs):.1f} |' for name, vs in fps.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_report.md'))
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its runs are measured next to this tree\'s')
    ap.add_argument('--notes', help='a file whose text is appended (what the figures mean)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'track_probe needs the MI355X'
    lines = ['# Per-object track report: tools/track_probe.py', '', f'device: {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} CPUs', '',
             'Stage time: cutie_time_ops, 200 back-to-back replays (warm caches), median of 5 (min - max), microseconds per replay of the whole chain.', '',
             '| planes | launches | us | min - max |', '|---|---|---|---|'] + stage_rows()
    lines += ['', f'eval_vos.run_dataset over 4 clips of {args.frames} frames of 854x480 (device egress), wall-clock frames/s of the second pass; every sample '
              f'in a fresh process, the legs interleaved, {args.rounds} rounds:', '', '| run | frames/s per round | median |', '|---|---|---|']
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
