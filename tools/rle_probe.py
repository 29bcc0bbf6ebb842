"""RLE probe (profiles/rle_probe.md): what the BURST strings of one frame cost on each route, at 720 x 1280 with 8 objects (smooth
blobs, made like `_probs` of tests/test_gpu_egress.py).

    python tools/rle_probe.py [--iters 200] [--out FILE.md]

  device   the RLE stage alone (PROB_TO_ID flags == 32, six launches) over the finished id plane: cutie_time_ops, median of 5 replays
  host     what egress='host' pays for the same strings: a blocking copy of the id plane to the host + the numpy codec
           (cutie_amd/inference/utils/coco_rle.py) over the 8 objects; wall clock, median of 9
The strings of both routes are compared before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

H, W, OBJECTS = 720, 1280, 8


def blobs(P, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.randn(1, P, max(h // 16, 2), max(w // 16, 2), generator=g), size=(h, w), mode='bicubic', align_corners=False)[0] * 4
    return torch.softmax(x + torch.randn(P, h, w, generator=g) * 0.3, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out')
    a = ap.parse_args()
    from cutie_amd import _lib, ops as O
    from cutie_amd.inference.utils import coco_rle
    ids = blobs(OBJECTS + 1, H, W, seed=1).argmax(0).to(torch.uint8).cuda()
    objects = list(range(1, OBJECTS + 1))
    objs = torch.tensor(objects, dtype=torch.int32).cuda()
    stream = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    table = torch.empty((OBJECTS, 4), dtype=torch.int32, device='cuda')
    status = torch.empty(4, dtype=torch.int32, device='cuda')
    scratch = torch.empty(O.OpList.rle_scratch_words(H, W, OBJECTS), dtype=torch.int32, device='cuda')
    ol = O.OpList()
    ol.rle_encode(ids, objs, stream, table, status, scratch, H=H, W=W, n_objects=OBJECTS)
    arr = ol.finalize()
    ol.run()
    torch.cuda.synchronize()
    plane = ids.cpu().numpy()
    want = [coco_rle.encode(plane == o) for o in objects]
    raw = stream.cpu().numpy().tobytes()
    got = [raw[off:off + ln].decode('ascii') for off, ln, _, _ in table.cpu().tolist()]
    assert got == want and status.cpu().tolist()[:2] == [sum(len(s) for s in want), 0]
    ex = _lib.get_executor()
    dev_us = statistics.median(ex.time_ops(arr, a.iters) for _ in range(5)) * 1e3

    def host_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = ids.cpu().numpy()
        t1 = time.perf_counter()
        for o in objects:
            coco_rle.encode(m == o)
        return (t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6
    host_route()
    runs = [host_route() for _ in range(9)]
    copy_us, enc_us = statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)
    counts = int(status.cpu()[2])
    rows = [f'| {W}x{H}, {OBJECTS} objects: {counts} counts, {sum(len(s) for s in want)} bytes | us per frame |', '|---|---|',
            f'| device: RLE stage alone (cutie_time_ops, {a.iters} iterations, median of 5) | {dev_us:.1f} |',
            f'| host: blocking copy of the id plane | {copy_us:.1f} |',
            f'| host: numpy codec over the {OBJECTS} objects | {enc_us:.1f} |',
            f'| host: both | {copy_us + enc_us:.1f} |']
    text = '\n'.join(rows) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
