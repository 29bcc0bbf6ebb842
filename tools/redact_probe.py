#!/usr/bin/env python
"""The redaction stage (PROB_TO_ID flags == 65536, csrc/redact.hip) measured alone; writes profiles/redact.md.

Device time of the stage -- one op: three launches for blur and pixelate, one for fill -- at 854 x 480 and 1920 x 1080: blur for r = 4, 12,
64, pixelate for c = 4, 16, 64, fill.  Device events around one op per sample with the caches cold (a 512 MB buffer is rewritten between
the samples, as in tools/matte_probe.py), after three warm-up runs; median / min / max of 30 samples, and the warm figure (cutie_time_ops,
back-to-back replays).  Next to every mode, in the same process and measured the same way: a plain device-to-device copy that moves the
bytes the stage must at least move -- for blur the frame in, two intermediate images written and read, the weight plane in, the frame again
for the blend and the output out (``moved_bytes``); a copy of n bytes reads n and writes n, so the copy is of half that total.  There is no threshold: the numbers are reported as they are.

    python tools/redact_probe.py [--samples 30] [--out profiles/redact.md]

Needs the GPU (no fall-back)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from cutie_amd import _lib, ops as O                                         # noqa: E402
from matte_probe import _time                                                # noqa: E402

CASES = [('blur', 4), ('blur', 12), ('blur', 64), ('pixelate', 4), ('pixelate', 16), ('pixelate', 64), ('fill', 0)]


def inputs(H, W, dev):
    """A photograph (the bike fixture, resized) and a 0 | 255 ellipse over a third of it."""
    im = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bike', '00000.jpg')).convert('RGB').resize((W, H), Image.BICUBIC)
    yy, xx = np.mgrid[0:H, 0:W]
    w = (255 * (np.hypot((yy - H / 2) / (H / 3), (xx - W / 2) / (W / 3)) <= 1.0)).astype(np.uint8)
    return torch.from_numpy(np.array(im)).to(dev), torch.from_numpy(w).to(dev)


def moved_bytes(mode, H, W, c):
    """bytes read + written at the least: blur 3 (frame) + 3 + 3 (A written, read) + 3 + 3 (B written, read) + 3 (frame for the blend) + 1
    (weight) + 3 (out) per pixel; pixelate 3 (frame) + the column sums written and read + 3 (frame) + 1 + 3; fill 3 + 1 + 3"""
    n = H * W
    if mode == 'blur':
        return 22 * n
    if mode == 'pixelate':
        return 10 * n + 2 * 4 * 3 * W * -(-H // c)
    return 7 * n


def copy_time(n, dev, flush, samples):
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    cold = []
    for k in range(samples):
        flush.fill_(k & 255)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        cold.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(cold), 1)


def stage_times(H, W, dev, flush, samples):
    frame, weight = inputs(H, W, dev)
    out = torch.empty_like(frame)
    rows = []
    for mode, s in CASES:
        scratch = torch.empty(O.OpList.redact_scratch_words(mode, H, W, s), dtype=torch.int32, device=dev)
        ol = O.OpList()
        ol.redact(frame, weight, out, scratch, mode=mode, strength=s, color=(0, 0, 0))
        t = _time(ol, flush, samples)
        n = moved_bytes(mode, H, W, s)
        rows.append((mode, s, t, n, copy_time(n // 2, dev, flush, samples)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'redact.md'))
    args = ap.parse_args()
    assert torch.cuda.is_available() and _lib.has_redact(), 'needs the GPU and a library with the stage'
    dev = torch.device('cuda:0')
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    lines = ['# The redaction stage alone (`tools/redact_probe.py`)', '',
             f'{torch.cuda.get_device_name(0)}; `PROB_TO_ID` flags == 65536, one op; device events, 3 warm-up runs, caches cold (512 MB rewritten between '
             f'samples), median (min .. max) of {args.samples} samples; warm = `cutie_time_ops`, median of 5 x 50 replays; copy = a device-to-device copy of '
             'half the bytes the stage must read and write, same process, same method.', '']
    for H, W in ((480, 854), (1080, 1920)):
        lines += [f'## {W} x {H}', '', '| mode | strength | cold us | warm us | bytes moved at the least | copy us | stage / copy |', '|---|---|---|---|---|---|---|']
        for mode, s, t, n, cp in stage_times(H, W, dev, flush, args.samples):
            lines.append(f"| {mode} | {s if mode != 'fill' else '-'} | {t['cold_us']} ({t['cold_us_min']} .. {t['cold_us_max']}) | {t['warm_us']} | {n} | {cp} | "
                         f"{t['cold_us'] / cp:.1f} |")
            print(lines[-1], flush=True)
        lines.append('')
    lines += ['Not measured: the kernels\' shares inside an op (no profiler run), hardware counters, the wall clock of `process_video --redact`.', '']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('wrote', args.out)


if __name__ == '__main__':
    main()
