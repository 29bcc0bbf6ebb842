"""Times the region filter (PROB_TO_ID flags == 2048, csrc/regions.hip) on one MI355X and writes profiles/region_filter.md:

(1) the stage with cutie_time_ops at 854x480 and 1920x1080 on a three-blob mask and on 0.5-density noise -- stage A alone (islands) and
    stages A + B (islands, then holes) -- next to the plain PROB_TO_ID kernel and the track statistics (geometry and confidence, 3
    objects) on planes of the same size, re-measured in the same process;
(2) the experiment of DESIGN.md section 15: eval_vos.run_dataset over four copies of a 96-frame 854x480 clip with --egress device
    --lockstep 4, wall-clock frames/s of the second pass, without and with --min-region / --fill-holes, and -- with --parent DIR, a built
    checkout of the parent commit -- the parent's run without them; every sample in a fresh process, the legs interleaved.

    python tools/region_probe.py [--frames 96] [--rounds 3] [--parent DIR] [--out profiles/region_filter.md]

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

from tools.track_probe import clips          # noqa: E402  (the same clips as profiles/track_report.md)


def planes(H, W):
    yy, xx = np.mgrid[:H, :W]
    blobs = np.zeros((H, W), dtype=np.uint8)
    for oid, (cy, cx, ry, rx) in ((1, (0.25, 0.23, 0.17, 0.18)), (2, (0.62, 0.7, 0.31, 0.1)), (3, (0.83, 0.12, 0.12, 0.07))):
        blobs[((yy / H - cy) / ry) ** 2 + ((xx / W - cx) / rx) ** 2 <= 1.0] = oid
    rng = np.random.default_rng(H)
    speck = blobs.copy()
    speck[rng.random((H, W)) < 0.001] = 2
    speck[rng.random((H, W)) < 0.001] = 0
    noise = (rng.random((H, W)) < 0.5).astype(np.uint8)
    return (('three blobs', blobs), ('three blobs, 0.1 % specks and pinholes', speck), ('0.5-density noise', noise))


def stage_rows(iters=200):
    from cutie_amd import _lib, ops as O
    rows = []
    ex = _lib.get_executor()

    def timed(ol):
        arr = ol.finalize()
        us = [ex.time_ops(arr, iters) * 1e3 for _ in range(5)]
        return f'{statistics.median(us):.1f} | {min(us):.1f} - {max(us):.1f}'
    for H, W in ((480, 854), (1080, 1920)):
        K = 3
        g = torch.Generator().manual_seed(H)
        low = torch.randn(K + 1, H // 16, W // 16 + 1, generator=g) * 3
        prob = torch.softmax(torch.nn.functional.interpolate(low[None], size=(H, W), mode='bilinear')[0], 0).cuda().contiguous()
        lut = torch.arange(K + 1, dtype=torch.int32).cuda()
        ids = torch.empty((H, W), dtype=torch.uint8, device='cuda')
        table = torch.empty((K, 12), dtype=torch.int32, device='cuda')
        ol = O.OpList()
        ol.prob_to_id(prob, lut, ids, P=K + 1, H=H, W=W, plane=prob.stride(0), ldrow=prob.stride(1))
        rows.append(f'| {W}x{H} | softmax planes | plain PROB_TO_ID (1 launch) | {timed(ol)} |')
        ol = O.OpList()
        ol.track_stats(ids, list(range(1, K + 1)), table, prob=prob, lut=lut)
        rows.append(f'| {W}x{H} | the ids of those planes | track statistics, with the probability planes (4 launches) | {timed(ol)} |')
        ol = O.OpList()
        ol.track_stats(ids, list(range(1, K + 1)), table)
        rows.append(f'| {W}x{H} | the ids of those planes | track statistics, id plane only (3 launches) | {timed(ol)} |')
        scratch = torch.empty(O.OpList.region_scratch_words(H, W), dtype=torch.int32, device='cuda')
        counts = torch.empty(4, dtype=torch.int32, device='cuda')
        for name, plane in planes(H, W):
            src = torch.from_numpy(plane).cuda()
            for what, kw in (('A, islands (4 launches)', dict(min_region=64)), ('A + B, islands then holes (8 launches)', dict(min_region=64, fill_holes=64))):
                # (the replays run on the plane the first run left: the thresholds' work is done once, the labelling every time; the
                # noise plane after min_region = 64 keeps its large components)
                ids.copy_(src)
                ol = O.OpList()
                ol.region_filter(ids, scratch, counts, connectivity=8, **kw)
                t = timed(ol)
                rows.append(f'| {W}x{H} | {name} | region filter {what} | {t} |')
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
print('LEG ' + json.dumps({'fps': fps, 'regions': [r.get('regions') for r in res.values()]}))
'''

FILTER = ['--min-region', '64', '--fill-holes', '64']


def leg(tree, root, frames, extra):
    p = subprocess.run([sys.executable, '-c', LEG, root, str(frames)] + extra, cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f'leg {extra} in {tree} failed ({p.returncode}): {p.stderr[-2000:]}')
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('LEG ')][-1][4:])
    assert all((g is not None) == bool(extra) for g in r['regions'])
    return r['fps'], r['regions']


def run_rows(frames, rounds, parent):
    legs = [('this tree, no options', ROOT, []), ('this tree, --min-region 64 --fill-holes 64', ROOT, FILTER)]
    if parent:
        legs += [('parent commit', os.path.abspath(parent), [])]
    fps = {name: [] for name, _, _ in legs}
    changed = None
    root = tempfile.mkdtemp(prefix='region_probe_')
    try:
        clips(root, frames)
        for _ in range(rounds):
            for name, tree, extra in legs:
                v, regions = leg(tree, root, frames, extra)
                fps[name].append(v)
                if extra:
                    changed = regions
                print(f'{name}: {v:.1f} frames/s', flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rows = [f'| {name} | ' + ' / '.join(f'{v:.1f}' for v in vs) + f' | {statistics.median(vs):.1f} |' for name, vs in fps.items()]
    if changed:
        t = {k: sum(g[k] for g in changed) for k in ('frames', 'islands_removed', 'pixels_cleared', 'holes_filled', 'pixels_filled')}
        rows += ['', f"The filtered run removed {t['islands_removed']} islands ({t['pixels_cleared']} pixels) and filled {t['holes_filled']} holes "
                     f"({t['pixels_filled']} pixels) on {t['frames']} frames."]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'region_filter.md'))
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its runs are measured next to this tree\'s')
    ap.add_argument('--notes', help='a file whose text is appended (what the figures mean)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'region_probe needs the MI355X'
    lines = ['# Region filter: tools/region_probe.py', '', f'device: {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} CPUs', '',
             'Stage time: cutie_time_ops, 200 back-to-back replays (warm caches), median of 5 (min - max), microseconds per replay of the whole chain.', '',
             '| size | plane | launches | us | min - max |', '|---|---|---|---|---|'] + stage_rows()
    lines += ['', f'eval_vos.run_dataset over 4 clips of {args.frames} frames of 854x480 (--egress device --lockstep 4), wall-clock frames/s of the second pass; '
              f'every sample in a fresh process, the legs interleaved, {args.rounds} rounds:', '', '| run | frames/s per round | median |', '|---|---|---|']
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
