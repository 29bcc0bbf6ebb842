#!/usr/bin/env python
"""The colour guided filter (PROB_TO_ID flags == 32768, csrc/guided.hip) measured; writes profiles/guided.md.

(1) Device time of the stage -- its two launches, one op -- at 854 x 480 and 1920 x 1080, for r = 4, 16, 64 and S = 1, 4 planes: device
    events around one op per sample with the caches cold (a 512 MB buffer is rewritten between the samples, as in tools/matte_probe.py),
    median / min / max, and the warm figure (cutie_time_ops, back-to-back replays).  Next to it, in the same process and measured the
    same way: the ``matte_composite('alpha')`` launch that produces the stage's input, and a plain device-to-device copy that moves the
    bytes the stage must at least move -- guide and planes in, planes out, the coefficient scratch written once and read once; a copy
    of n bytes reads n and writes n, so the copy is of half that total.  With --kernels FILE (the kernel statistics csv of a
    ``rocprofv3 --kernel-trace --stats`` run of ``--stage-only``) the two kernels' averages are added.
(2) Wall clock of process_video --alpha --cutout on a synthetic 1920 x 1080 clip (3 objects, random-init weights, --ingest device --egress
    device) without and with --refine-matte 16: a fresh process per sample, the legs interleaved.  Both numbers are reported; there is no
    threshold.

    python tools/guided_probe.py [--frames 24] [--repeats 3] [--kernels FILE] [--stage-only] [--no-driver] [--out profiles/guided.md]

Needs the GPU (no fall-back)."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from cutie_amd import _lib, ops as O                                         # noqa: E402
from matte_probe import _time, make_clip                                     # noqa: E402

KERNELS = ('gf_coef_kernel', 'gf_apply_kernel')
RADII, PLANES = (4, 16, 64), (1, 4)


def inputs(H, W, S, dev):
    """A photograph-like guide (the bike fixture, resized) and S soft planes: ellipses with ramps a few pixels wide."""
    im = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bike', '00000.jpg')).convert('RGB').resize((W, H), Image.BICUBIC)
    yy, xx = np.mgrid[0:H, 0:W]
    planes = np.stack([np.clip(255 * (8.0 - 8.0 * np.hypot((yy - H / 2) / (H / (3 + s)), (xx - W / 2) / (W / (3 + s)))), 0, 255).astype(np.uint8)
                       for s in range(S)])
    return torch.from_numpy(np.array(im)).to(dev), torch.from_numpy(planes).to(dev)


def moved_bytes(H, W, S):
    """guide + planes in, planes out, 16 bytes of coefficients per plane and pixel written and read"""
    return 3 * H * W + S * H * W + S * H * W + 2 * 16 * S * H * W


def stage_times(H, W, dev, flush, samples=30):
    rows = {}
    for S in PLANES:
        guide, planes = inputs(H, W, S, dev)
        out = torch.empty_like(planes)
        scratch = torch.empty(O.OpList.guided_scratch_words(S, H, W), dtype=torch.int32, device=dev)
        for r in RADII:
            ol = O.OpList()
            ol.guided_filter(guide, planes, out, scratch, radius=r, eps=1e-4)
            rows[f'guided filter, S = {S}, r = {r}'] = dict(_time(ol, flush, samples), bytes=moved_bytes(H, W, S))
        n = moved_bytes(H, W, S) // 2
        src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        cold = []
        for k in range(samples):
            flush.fill_(k & 255)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            cold.append(e0.elapsed_time(e1) * 1e3)
        rows[f'device-to-device copy of {n} bytes (the traffic of S = {S})'] = {
            'cold_us': round(statistics.median(cold), 1), 'cold_us_min': round(min(cold), 1), 'cold_us_max': round(max(cold), 1), 'warm_us': None,
            'bytes': 2 * n}
    # the launch that produces the stage's input: the alpha matte of 3 objects from planes at the internal size
    h, w = (480, 854) if H > 480 else (H, W)
    prob = torch.softmax(torch.randn(4, h, w, generator=torch.Generator().manual_seed(H)) * 3, 0).to(dev)
    matte = torch.empty((H, W), dtype=torch.uint8, device=dev)
    ol = O.OpList()
    ol.matte_composite('alpha', None, out_hw=(H, W), planes=prob, targets=[1, 2, 3], matte=matte)
    rows[f"matte_composite('alpha'), 4 planes of {w} x {h}"] = dict(_time(ol, flush, samples), bytes=prob.numel() * 4 + H * W)
    return rows


def kernel_shares(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            for k in KERNELS:
                if k in name:
                    calls, total = int(row['Calls']), int(float(row['TotalDurationNs']))
                    c0, t0 = out.get(k, (0, 0))
                    out[k] = (c0 + calls, t0 + total)
    return out


def stage_only(dev):
    """What a profiler run wraps: the stage at 1920 x 1080, S = 1, r = 4, 16 and 64, twenty times each."""
    H, W = 1080, 1920
    guide, planes = inputs(H, W, 1, dev)
    out = torch.empty_like(planes)
    scratch = torch.empty(O.OpList.guided_scratch_words(1, H, W), dtype=torch.int32, device=dev)
    for r in RADII:
        ol = O.OpList()
        ol.guided_filter(guide, planes, out, scratch, radius=r, eps=1e-4)
        for _ in range(20):
            ol.run()
    torch.cuda.synchronize()
    print('stage-only', int(out.sum()))


# one sample of process_video --alpha --cutout in a process of its own; argv: the clip, the radius (0: without --refine-matte)
LEG = '''
import json, sys, tempfile, time, torch
sys.path.insert(0, '.')
from cutie_amd.model.cutie import CUTIE
from cutie_amd.process_video import process_video, video_config
data, r = sys.argv[1], int(sys.argv[2])
cfg = video_config()
net = CUTIE(cfg).cuda().eval()
kw = dict(matte_refine=(r, 1e-4)) if r else {}
out = []
with torch.inference_mode():
    for k in range(2):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = process_video(net, cfg, data + '/frames', data + '/masks', tmp, ingest='device', egress='device', alpha_matte=True, cutout=True, **kw)
            torch.cuda.synchronize(); out.append(res['frames'] / (time.perf_counter() - t0))
print('LEG ' + json.dumps({'fps': out[1]}))
'''


def leg(data, r):
    p = subprocess.run([sys.executable, '-c', LEG, data, str(r)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f'leg r = {r} failed ({p.returncode}): {p.stderr[-2000:]}')
    return json.loads([l for l in p.stdout.splitlines() if l.startswith('LEG ')][-1][4:])['fps']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernels', help='kernel statistics csv of a profiler run of --stage-only: the two kernels\' averages')
    ap.add_argument('--stage-only', action='store_true', help='run the stage at 1920 x 1080 twenty times per radius and exit (for a profiler)')
    ap.add_argument('--no-driver', action='store_true', help='skip the process_video legs')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guided.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'guided_probe needs the MI355X'
    dev = torch.device('cuda:0')
    if args.stage_only:
        return stage_only(dev)
    res = {'stage': {}}
    with torch.inference_mode():
        flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        for H, W in ((480, 854), (1080, 1920)):
            res['stage'][f'{W}x{H}'] = stage_times(H, W, dev, flush)
        del flush
    torch.cuda.empty_cache()
    if not args.no_driver:
        with tempfile.TemporaryDirectory() as data:
            make_clip(data, args.frames, h=1080, w=1920)
            res['driver'] = {'plain': [], 'refine 16': []}
            for _ in range(args.repeats):
                res['driver']['plain'].append(round(leg(data, 0), 2))
                res['driver']['refine 16'].append(round(leg(data, 16), 2))
    lines = ['# The colour guided filter on the device (tools/guided_probe.py)', '',
             f'One MI355X, {len(os.sched_getaffinity(0))} CPUs.  Cold: device events around one op (both launches), a 512 MB buffer rewritten between '
             'the samples (median of 30, min - max); warm: cutie_time_ops, 50 back-to-back replays.  The guide is the bike fixture resized, the '
             'planes soft ellipses.  "bytes" is what the stage must at least move: guide and planes in, planes out, 16 bytes of coefficients '
             'per plane and pixel written and read; the copy row moves the same total (it reads and writes half of it).', '']
    for geom, rows in res['stage'].items():
        lines += [f'## {geom}', '', '| what | cold us (min - max) | warm us | bytes | cold / copy |', '|---|---|---|---|---|']
        copies = {int(name.split('S = ')[1].rstrip(')')): r['cold_us'] for name, r in rows.items() if name.startswith('device-to-device')}
        for name, r in rows.items():
            ratio = ''
            if name.startswith('guided filter'):
                ratio = f"{r['cold_us'] / copies[int(name.split('S = ')[1].split(',')[0])]:.1f}"
            lines.append(f"| {name} | {r['cold_us']} ({r['cold_us_min']} - {r['cold_us_max']}) | {r['warm_us'] if r['warm_us'] is not None else ''} | {r['bytes']} | {ratio} |")
        lines.append('')
    if args.kernels:
        lines += ['## The two kernels, 1920 x 1080, S = 1, r = 4, 16, 64 together (profiler run of --stage-only, 60 ops)', '', '| kernel | calls | average us |', '|---|---|---|']
        for k, (calls, total) in kernel_shares(args.kernels).items():
            lines.append(f'| {k} | {calls} | {total / max(calls, 1) / 1e3:.1f} |')
        lines.append('')
    if 'driver' in res:
        lines += [f'## process_video --alpha --cutout, {args.frames} synthetic 1920 x 1080 frames, 3 objects, --ingest device --egress device', '',
                  'Wall clock, a fresh process per sample (its second run of the clip is the sample), the legs interleaved.', '',
                  '| leg | frames/s per sample | median |', '|---|---|---|']
        for k, v in res['driver'].items():
            lines.append(f'| {k} | {v} | {statistics.median(v)} |')
        lines.append('')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
