#!/usr/bin/env python
"""The filtered, dynamic-Huffman PNG stage (PROB_TO_ID flags == 16384, csrc/png_photo.hip) measured; writes profiles/png_photo.md.

(1) Device time of the stage -- its five launches, one op -- at 854 x 480 and 1920 x 1080, for RGBA (a photograph with a soft matte) and
    for L (the matte alone): device events around one op per sample with the caches cold (a 512 MB buffer is rewritten between the
    samples, as in tools/matte_probe.py), median / min / max, and the warm figure (cutie_time_ops, back-to-back replays).  With
    --kernels FILE (the kernel statistics csv of a ``rocprofv3 --kernel-trace --stats`` run of ``--stage-only``) the share of each of
    the five kernels is added.  Next to it, for the same planes: the id planes' encoder (flags 8), the stream sizes, and the host route
    on this machine -- the RGBA frame copied back and saved by PIL at compress_level=1.
(2) Wall-clock frames/s of process_video on a synthetic 854 x 480 clip (3 objects, random-init weights, --ingest device --egress device)
    without the new options and with --cutout, the legs alternating after a warm-up of each.
(3) With --parent DIR (a built checkout of the parent commit): the run without the new options in a fresh process per sample, this tree
    and the parent alternating -- the comparison for "nothing existing got slower".

    python tools/png_photo_probe.py [--frames 200] [--repeats 3] [--parent DIR] [--kernels FILE] [--stage-only] [--out profiles/png_photo.md]

Needs the GPU (no fall-back)."""
import argparse
import csv
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from cutie_amd import _lib, ops as O                                         # noqa: E402
from matte_probe import _time, make_clip, plain_leg                          # noqa: E402

KERNELS = ('pph_filter_kernel', 'pph_token_kernel', 'pph_codes_kernel', 'pph_scan_kernel', 'pph_emit_kernel')


def photo(H, W):
    """A photograph-like frame (the bike fixture, resized) and a soft matte."""
    im = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bike', '00000.jpg')).convert('RGB').resize((W, H), Image.BICUBIC)
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.hypot((yy - H / 2) / (H / 3), (xx - W / 2) / (W / 3))
    return np.array(im), np.clip(255 * (1.6 - 1.2 * d), 0, 255).astype(np.uint8)


def stage_times(H, W, dev, flush, samples=30):
    rgb, alpha = photo(H, W)
    frame, matte = torch.from_numpy(rgb).to(dev), torch.from_numpy(alpha).to(dev)
    rows = {}
    status = torch.empty(4, dtype=torch.int32, device=dev)

    def add(name, B, build, cap, words):
        stream = torch.empty(cap, dtype=torch.uint8, device=dev)
        scratch = torch.empty(words, dtype=torch.int32, device=dev)
        ol = O.OpList()
        build(ol, stream, scratch)
        r = _time(ol, flush, samples)
        torch.cuda.synchronize()
        st = status.cpu().tolist()
        assert st[2] == 0, st
        r['stream_bytes'], r['raw_bytes'] = st[0], H * W * B
        rows[name] = r
    add('RGBA, filters + dynamic codes (5 launches)', 4, lambda ol, s, c: ol.png_photo(frame, s, status, c, last=matte),
        O.OpList.png_photo_capacity(H, W, 4), O.OpList.png_photo_scratch_words(H, W, 4))
    add('L (the matte), filters + dynamic codes (5 launches)', 1, lambda ol, s, c: ol.png_photo(matte, s, status, c),
        O.OpList.png_photo_capacity(H, W, 1), O.OpList.png_photo_scratch_words(H, W, 1))
    add('L (the matte), the id planes\' encoder (flags 8, 3 launches)', 1, lambda ol, s, c: ol.png_deflate(matte, s, status, c, H=H, W=W),
        O.OpList.png_capacity(H, W), O.OpList.png_scratch_words(H, W))
    # the host route: the RGBA frame copied back and saved by PIL at compress_level=1
    host = []
    size = 0
    rgba = torch.cat([frame, matte[..., None]], dim=2).contiguous()
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        arr = rgba.cpu().numpy()
        buf = io.BytesIO()
        Image.fromarray(arr, 'RGBA').save(buf, 'PNG', compress_level=1)
        host.append((time.perf_counter() - t0) * 1e3)
        size = len(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(rgba.cpu().numpy(), 'RGBA').save(buf, 'PNG')
    rows['host route'] = {'ms_median': round(statistics.median(host), 1), 'file_bytes': size, 'pil_default_bytes': len(buf.getvalue())}
    return rows


def kernel_shares(path):
    """name -> (calls, total ns, average ns) of the stage's kernels from a rocprofv3 kernel statistics csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            for k in KERNELS:
                if name.startswith(k):
                    out[k] = (int(row['Calls']), int(float(row['TotalDurationNs'])), float(row['AverageNs']))
    return out


def stage_only(dev):
    """What a profiler run wraps: the RGBA stage at 854 x 480, 20 times."""
    H, W = 480, 854
    rgb, alpha = photo(H, W)
    frame, matte = torch.from_numpy(rgb).to(dev), torch.from_numpy(alpha).to(dev)
    stream = torch.empty(O.OpList.png_photo_capacity(H, W, 4), dtype=torch.uint8, device=dev)
    scratch = torch.empty(O.OpList.png_photo_scratch_words(H, W, 4), dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    ol = O.OpList()
    ol.png_photo(frame, stream, status, scratch, last=matte)
    for _ in range(20):
        ol.run()
    torch.cuda.synchronize()
    print('stage-only', status.cpu().tolist())


def driver_legs(dev, data, repeats):
    from cutie_amd.model.cutie import CUTIE
    from cutie_amd.process_video import process_video, video_config
    cfg = video_config()
    net = CUTIE(cfg).to(dev).eval()
    legs = {'plain': {}, 'cutout': dict(cutout=True)}
    fps = {k: [] for k in legs}

    def leg(kw):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = process_video(net, cfg, os.path.join(data, 'frames'), os.path.join(data, 'masks'), tmp, ingest='device', egress='device', **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            files = sum(len(fs) for _, _, fs in os.walk(tmp))
            nbytes = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(tmp) for f in fs)
        return r['frames'] / wall, r['frames'] / r['seconds'], files, nbytes
    for kw in legs.values():
        leg(kw)
    extra = {}
    for _ in range(repeats):
        for name, kw in legs.items():
            f, model, files, nbytes = leg(kw)
            fps[name].append(round(f, 1))
            extra[name] = {'model_fps': round(model, 1), 'files': files, 'bytes': nbytes}
    return {name: {'fps': v, 'fps_median': statistics.median(v), **extra[name]} for name, v in fps.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--parent', help='a built checkout of the parent commit: its run without the new options is measured next to this tree\'s')
    ap.add_argument('--kernels', help='kernel statistics csv of a profiler run of --stage-only: the five kernels\' shares')
    ap.add_argument('--stage-only', action='store_true', help='run the RGBA stage at 854 x 480 twenty times and exit (for a profiler)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_photo.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'png_photo_probe needs the MI355X'
    dev = torch.device('cuda:0')
    if args.stage_only:
        return stage_only(dev)
    res = {'stage': {}}
    with torch.inference_mode(), tempfile.TemporaryDirectory() as data:
        flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        for H, W in ((480, 854), (1080, 1920)):
            res['stage'][f'{W}x{H}'] = stage_times(H, W, dev, flush)
        del flush
        make_clip(data, args.frames)
        res['driver'] = driver_legs(dev, data, args.repeats)
        if args.parent:
            trees = {'this tree': ROOT, 'parent': os.path.abspath(args.parent)}
            res['plain_fresh_process'] = {k: [] for k in trees}
            for _ in range(args.repeats):
                for k, tree in trees.items():
                    res['plain_fresh_process'][k].append(round(plain_leg(tree, data), 1))
    lines = ['# PNG with scanline filters and dynamic Huffman codes on the device (tools/png_photo_probe.py)', '',
             f'One MI355X, {len(os.sched_getaffinity(0))} CPUs.  Cold: device events around one op (all its launches), a 512 MB buffer rewritten '
             'between the samples (median of 30, min - max); warm: cutie_time_ops, 50 back-to-back replays.  The frame is the bike fixture '
             'resized, the matte a soft ellipse.', '']
    for geom, rows in res['stage'].items():
        lines += [f'## {geom}', '', '| stage | cold us (min - max) | warm us | stream bytes | raw bytes |', '|---|---|---|---|---|']
        for name, r in rows.items():
            if name != 'host route':
                lines.append(f"| {name} | {r['cold_us']} ({r['cold_us_min']} - {r['cold_us_max']}) | {r['warm_us']} | {r['stream_bytes']} | {r['raw_bytes']} |")
        h = rows['host route']
        lines += ['', f"Host route on this machine (RGBA copied back, PIL compress_level=1): {h['ms_median']} ms per frame, {h['file_bytes']} bytes; "
                  f"PIL's default level gives {h['pil_default_bytes']} bytes.", '']
    if args.kernels:
        lines += ['## The five kernels, RGBA 854 x 480 (profiler run of --stage-only, 20 ops)', '', '| kernel | calls | average us |', '|---|---|---|']
        for k, (calls, total, avg) in kernel_shares(args.kernels).items():
            lines.append(f'| {k} | {calls} | {avg / 1e3:.1f} |')
        lines.append('')
    lines += [f'## process_video, {args.frames} synthetic 854 x 480 frames, 3 objects, --ingest device --egress device', '',
              '| leg | frames/s per repeat (wall clock, legs alternating) | median | model frames/s | files written | bytes written |', '|---|---|---|---|---|---|']
    for name, r in res['driver'].items():
        lines.append(f"| {name} | {r['fps']} | {r['fps_median']} | {r['model_fps']} | {r['files']} | {r['bytes']} |")
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
