#!/usr/bin/env python
"""The visualisation / soft-mask stages (PROB_TO_ID flags == 256 / 512, csrc/matte.hip) measured; writes profiles/matte.md.

(1) Device time of ONE composite launch per mode (popup with the matte, layer, fade), of the matte alone and of the soft-mask launch, at
    854 x 480 with 3 objects and 1920 x 1080 with 5, planes stored at the output size: device events around one op per sample with the
    caches cold (a 512 MB buffer is rewritten between the samples, as in tools/visualize_bench.py), median / min / max, the warm figure
    (cutie_time_ops, back-to-back replays) next to it, and the bytes the launch must move as a fraction of the time at 8 TB/s.  The JPEG
    stage it feeds (flags == 128 on a plain frame, eight launches) is measured the same way in the same session.
(2) Wall-clock frames/s of process_video on a synthetic 854 x 480 clip (3 objects, random-init weights, --ingest device --egress device)
    without the new options and with --vis popup --soft-masks, the legs alternating after a warm-up of each.
(3) With --parent DIR (a built checkout of the parent commit): the run without the new options in a fresh process per sample, this tree
    and the parent alternating -- the comparison for "nothing existing got slower".

    python tools/matte_probe.py [--frames 200] [--repeats 3] [--parent DIR] [--out profiles/matte.md]

Needs the GPU (no fall-back)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from cutie_amd import _lib, ops as O                                         # noqa: E402
from cutie_amd.inference.utils import jpeg_writer as JW                      # noqa: E402
from cutie_amd.inference.utils.results_utils import davis_palette, davis_palette_np   # noqa: E402

HBM = 8e12      # bytes / s


def _time(ol, flush, samples):
    arr = ol.finalize()
    for _ in range(3):
        ol.run()
    torch.cuda.synchronize()
    cold = []
    for k in range(samples):
        flush.fill_(k & 255)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ol.run()
        e1.record()
        torch.cuda.synchronize()
        cold.append(e0.elapsed_time(e1) * 1e3)
    warm = statistics.median(_lib.get_executor().time_ops(arr, 50) for _ in range(5)) * 1e3
    return {'cold_us': round(statistics.median(cold), 1), 'cold_us_min': round(min(cold), 1), 'cold_us_max': round(max(cold), 1),
            'warm_us': round(warm, 1)}


def stage_times(H, W, K, dev, flush, samples=30):
    P, N = K + 1, H * W
    g = torch.Generator().manual_seed(H)
    prob = torch.softmax(torch.randn(P, H, W, generator=g) * 3, 0).to(dev)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    layer = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=g).to(dev)
    ids = prob.argmax(0).to(torch.uint8)
    colors = torch.from_numpy(JW.color_table(davis_palette_np, list(range(1, P)))).to(dev)
    out, matte = torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev)
    soft = torch.empty((K, H, W), dtype=torch.uint8, device=dev)
    targets = list(range(1, P))
    rows = {}

    def add(name, build, nbytes):
        ol = O.OpList()
        build(ol)
        r = _time(ol, flush, samples)
        r['bytes'] = nbytes
        r['roof_us'] = round(nbytes / HBM * 1e6, 2)
        r['fraction_of_8TBs'] = round(r['roof_us'] / r['cold_us'], 3)
        rows[name] = r
    add('popup + matte', lambda ol: ol.matte_composite('popup', out, out_hw=(H, W), frame=frame, planes=prob, targets=targets, matte=matte), N * (4 * K + 3 + 3 + 1))
    add('layer', lambda ol: ol.matte_composite('layer', out, out_hw=(H, W), frame=frame, planes=prob, targets=targets, layer=layer), N * (4 * K + 3 + 4 + 3))
    add('fade', lambda ol: ol.matte_composite('fade', out, out_hw=(H, W), frame=frame, ids=ids, colors=colors), N * (3 + 1 + 3))
    add('alpha alone', lambda ol: ol.matte_composite('alpha', None, out_hw=(H, W), planes=prob, targets=targets, matte=matte), N * (4 * K + 1))
    add('soft masks', lambda ol: ol.matte_soft(prob, soft, out_hw=(H, W)), N * (4 * K + K))
    qt = torch.from_numpy(JW.quant_tables().view(np.int16)).to(dev)
    stream = torch.empty(O.OpList.jpeg_enc_capacity(H, W, worst=True), dtype=torch.uint8, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(O.OpList.jpeg_enc_scratch_words(H, W), dtype=torch.int32, device=dev)
    ol = O.OpList()
    ol.jpeg_encode(out, None, None, qt, stream, status, scratch, H=H, W=W)
    rows['JPEG stage (8 launches, the popup frame)'] = _time(ol, flush, samples)
    return rows


def make_clip(root, n, h=480, w=854, objects=3, seed=9):
    from cutie_amd.utils.synth import SyntheticClip
    clip = SyntheticClip(h, w, objects, n, seed=seed)
    os.makedirs(os.path.join(root, 'frames')); os.makedirs(os.path.join(root, 'masks'))
    for t in range(n):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'frames', f'{t:07d}.jpg'), quality=95)
    png = Image.fromarray(clip.first_mask().numpy().astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'masks', '0000000.png'))


# one sample of the run without the new options, in a process of its own, from whatever tree is the working directory
PLAIN_LEG = '''
import json, sys, tempfile, time, torch
sys.path.insert(0, '.')
from cutie_amd.model.cutie import CUTIE
from cutie_amd.process_video import process_video, video_config
data = sys.argv[1]
cfg = video_config()
net = CUTIE(cfg).cuda().eval()
out = []
with torch.inference_mode():
    for k in range(2):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = process_video(net, cfg, data + '/frames', data + '/masks', tmp, ingest='device', egress='device')
            torch.cuda.synchronize(); out.append(r['frames'] / (time.perf_counter() - t0))
print('LEG ' + json.dumps({'fps': out[1]}))
'''


def plain_leg(tree, data):
    p = subprocess.run([sys.executable, '-c', PLAIN_LEG, data], cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f'plain leg in {tree} failed ({p.returncode}): {p.stderr[-2000:]}')
    return json.loads([l for l in p.stdout.splitlines() if l.startswith('LEG ')][-1][4:])['fps']


def driver_legs(dev, data, repeats):
    from cutie_amd.model.cutie import CUTIE
    from cutie_amd.process_video import process_video, video_config
    cfg = video_config()
    net = CUTIE(cfg).to(dev).eval()
    legs = {'plain': {}, 'vis popup + soft masks': dict(vis_modes=('popup',), soft_masks=True)}
    fps = {k: [] for k in legs}

    def leg(kw):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = process_video(net, cfg, os.path.join(data, 'frames'), os.path.join(data, 'masks'), tmp, ingest='device', egress='device', **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            files = sum(len(fs) for _, _, fs in os.walk(tmp))
        return r['frames'] / wall, r['frames'] / r['seconds'], files
    for kw in legs.values():
        leg(kw)
    extra = {}
    for _ in range(repeats):
        for name, kw in legs.items():
            f, model, files = leg(kw)
            fps[name].append(round(f, 1))
            extra[name] = {'model_fps': round(model, 1), 'files': files}
    return {name: {'fps': v, 'fps_median': statistics.median(v), **extra[name]} for name, v in fps.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its run without the new options is measured next to this tree\'s')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matte.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'matte_probe needs the MI355X'
    dev = torch.device('cuda:0')
    res = {'stage': {}}
    with torch.inference_mode(), tempfile.TemporaryDirectory() as data:
        flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        for H, W, K in ((480, 854, 3), (1080, 1920, 5)):
            res['stage'][f'{W}x{H}, {K} objects'] = stage_times(H, W, K, dev, flush)
        del flush
        make_clip(data, args.frames)
        res['driver'] = driver_legs(dev, data, args.repeats)
        if args.parent:
            trees = {'this tree': ROOT, 'parent': os.path.abspath(args.parent)}
            res['plain_fresh_process'] = {k: [] for k in trees}
            for _ in range(args.repeats):
                for k, tree in trees.items():
                    res['plain_fresh_process'][k].append(round(plain_leg(tree, data), 1))
    lines = ['# Visualisation modes, alpha matte and soft masks on the device (tools/matte_probe.py)', '',
             f'One MI355X, {len(os.sched_getaffinity(0))} CPUs.  Cold: device events around one op, a 512 MB buffer rewritten between the samples '
             '(median of 30, min - max); warm: cutie_time_ops, 50 back-to-back replays.  Roof: the bytes the launch must move at 8 TB/s.', '']
    for geom, rows in res['stage'].items():
        lines += [f'## {geom} (planes stored at the output size)', '', '| launch | cold us (min - max) | warm us | bytes | roof us | cold as a fraction of 8 TB/s |',
                  '|---|---|---|---|---|---|']
        for name, r in rows.items():
            lines.append(f"| {name} | {r['cold_us']} ({r['cold_us_min']} - {r['cold_us_max']}) | {r['warm_us']} | {r.get('bytes', '')} | {r.get('roof_us', '')} | "
                         f"{r.get('fraction_of_8TBs', '')} |")
        lines.append('')
    lines += [f'## process_video, {args.frames} synthetic 854 x 480 frames, 3 objects, --ingest device --egress device', '',
              '| leg | frames/s per repeat (wall clock, legs alternating) | median | model frames/s | files written |', '|---|---|---|---|---|']
    for name, r in res['driver'].items():
        lines.append(f"| {name} | {r['fps']} | {r['fps_median']} | {r['model_fps']} | {r['files']} |")
    if args.parent:
        lines += ['', '## The run without the new options, a fresh process per sample, this tree and the parent commit alternating', '',
                  '| tree | frames/s per sample | median |', '|---|---|---|']
        for k, v in res['plain_fresh_process'].items():
            lines.append(f'| {k} | {v} | {statistics.median(v)} |')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
