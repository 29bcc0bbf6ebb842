#!/usr/bin/env python
"""Result egress, host against device (ResultSaver(egress=...)): a fixed seeded sequence of probability frames (K = 3 objects) goes through
ResultSaver into a temporary directory, (a) 854 x 480 as it is and (b) 854 x 480 resampled to 1920 x 1080, each with egress='host' (the id
plane is copied, PIL encodes) and egress='device' (fused resample + argmax, PNG stream written by the GPU), the legs alternating in one
process.  Reported per case and leg: end-to-end frames/s (wall clock from the first `process` to the return of `end()`), the time the
stepping thread spends inside `process` per frame, bytes copied to the host per frame, and file sizes; per case the device time of the
egress launches (cutie_time_ops, median of the replays): the RESIZE + PROB_TO_ID pair against the fused kernel, and the deflate stages.

    python tools/egress_bench.py [--frames 300] [--repeats 5] [--out profiles/egress.json]

Needs the GPU (no fall-back).  The golden masks' device / PIL file sizes are recorded as well (information, not a gate)."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from cutie_amd import _lib, ops as O                                         # noqa: E402
from cutie_amd.inference.inference_core import InferenceCore                 # noqa: E402
from cutie_amd.inference.utils import png as png_container                   # noqa: E402
from cutie_amd.inference.utils.results_utils import ResultSaver, davis_palette  # noqa: E402

K, H0, W0 = 3, 480, 854


def make_frames(n, dev):
    """n probability frames [K + 1, 480, 854]: smooth seeded logits that drift a few pixels per frame (object-like masks)."""
    g = torch.Generator().manual_seed(0)
    low = torch.randn(1, K + 1, 12, 20, generator=g)
    base = (F.interpolate(low, size=(H0 + 64, W0 + 64), mode='bicubic', align_corners=False)[0] * 6).to(dev)
    base[0] += 2.0                                                            # mostly background
    out = []
    for t in range(n):
        dy, dx = (t * 3) % 64, (t * 5) % 64
        out.append(torch.softmax(base[:, dy:dy + H0, dx:dx + W0], 0).contiguous())
    return out


class _Obj:
    def __init__(self, i):
        self.id = i


def make_processor(dev):
    """What ResultSaver needs of an InferenceCore: the device, the object table and InferenceCore.output_prob_to_mask itself."""
    objs = [_Obj(i) for i in (1, 2, 3)]
    om = types.SimpleNamespace(tmp_id_to_obj={k + 1: o for k, o in enumerate(objs)}, obj_to_tmp_id={o: k + 1 for k, o in enumerate(objs)},
                               all_obj_ids=[o.id for o in objs])
    core = types.SimpleNamespace(network=types.SimpleNamespace(device=dev), object_manager=om)
    core.output_prob_to_mask = types.MethodType(InferenceCore.output_prob_to_mask, core)
    return core


class CountingSaver(ResultSaver):
    """ResultSaver that counts the device-to-host bytes of the masks: the id plane on the host path; the slab, and the rest of a
    stream longer than the slab, on the device path."""
    copied = 0

    def process(self, prob, frame_name, resize_needed=False, shape=None, **kw):
        if self.egress == 'host':
            h, w = shape if resize_needed else prob.shape[-2:]
            self.copied += int(h) * int(w)
        return super().process(prob, frame_name, resize_needed=resize_needed, shape=shape, **kw)

    def _fetch(self, b):
        data = super()._fetch(b)
        self.copied += b.host.numel() + max(0, len(data) - (b.host.numel() - 16))
        return data


def run_leg(frames, core, egress, shape, out_dir):
    saver = CountingSaver(out_dir, 'v', dataset='d17-val', object_manager=core.object_manager, use_long_id=False, palette=davis_palette,
                        processor=core, egress=egress)
    assert saver.egress == egress
    torch.cuda.synchronize()
    inside = 0.0
    t0 = time.perf_counter()
    for t, prob in enumerate(frames):
        a = time.perf_counter()
        saver.process(prob, f'{t:05d}.jpg', resize_needed=shape is not None, shape=shape, last_frame=(t == len(frames) - 1))
        inside += time.perf_counter() - a
    saver.end()
    wall = time.perf_counter() - t0
    files = sorted(os.listdir(os.path.join(out_dir, 'v')))
    assert len(files) == len(frames)
    size = sum(os.path.getsize(os.path.join(out_dir, 'v', f)) for f in files) / len(files)
    return {'fps': len(frames) / wall, 'process_ms_per_frame': 1e3 * inside / len(frames), 'bytes_to_host_per_frame': saver.copied / len(frames),
            'file_bytes_mean': size}


def device_times(prob, shape, dev, iters=50, replays=7):
    ex = _lib.get_executor()
    P, h, w = prob.shape
    H, W = shape or (h, w)
    lut = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=dev)
    ids = torch.empty((H, W), dtype=torch.uint8, device=dev)
    stream = torch.empty(O.OpList.png_capacity(H, W), dtype=torch.uint8, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(O.OpList.png_scratch_words(H, W), dtype=torch.int32, device=dev)
    kw = dict(P=P, H=h, W=w, plane=prob.stride(0), ldrow=prob.stride(1))

    def med(build):
        ol = O.OpList()
        build(ol)
        arr = ol.finalize()
        return statistics.median(ex.time_ops(arr, iters) for _ in range(replays))
    out = {}
    if shape is not None:
        full = torch.empty((P, H, W), dtype=torch.float32, device=dev)

        def pair(ol):
            ol.resize(prob, full, C=P, H=h, W=w, OH=H, OW=W, plane=prob.stride(0), ldrow=prob.stride(1))
            ol.prob_to_id(full, lut, ids, P=P, H=H, W=W, plane=H * W, ldrow=W)
        out['resize_plus_prob_to_id_ms'] = med(pair)
        out['fused_resample_argmax_ms'] = med(lambda ol: ol.prob_to_id(prob, lut, ids, out_hw=(H, W), **kw))
    else:
        out['prob_to_id_ms'] = med(lambda ol: ol.prob_to_id(prob, lut, ids, **kw))
    out['deflate_stages_ms'] = med(lambda ol: ol.png_deflate(ids, stream, status, scratch, H=H, W=W))     # (on the ids the line above left)
    out['egress_op_ms'] = med(lambda ol: ol.prob_to_id(prob, lut, ids, out_hw=shape, png=(stream, status, scratch), **kw))
    torch.cuda.synchronize()
    out['stream_bytes'] = int(status[0])
    return out


def golden_sizes(dev):
    """Per golden palette mask: bytes of the device-made file against PIL's."""
    rows = {}
    gold = os.path.join(ROOT, 'tests', 'golden')
    for dp, _, fs in sorted(os.walk(gold)):
        for f in sorted(fs):
            if not f.endswith('.png'):
                continue
            im = Image.open(os.path.join(dp, f))
            if im.mode != 'P':
                continue
            a = np.array(im, dtype=np.uint8)
            Hh, Ww = a.shape
            stream = torch.empty(O.OpList.png_capacity(Hh, Ww), dtype=torch.uint8, device=dev)
            status = torch.empty(4, dtype=torch.int32, device=dev)
            scratch = torch.empty(O.OpList.png_scratch_words(Hh, Ww), dtype=torch.int32, device=dev)
            ol = O.OpList()
            ol.png_deflate(torch.from_numpy(a).to(dev), stream, status, scratch, H=Hh, W=Ww)
            ol.run()
            torch.cuda.synchronize()
            assert int(status[2]) == 0
            mine = len(png_container.assemble(stream[:int(status[0])].cpu().numpy().tobytes(), Hh, Ww, im.getpalette()))
            ref = Image.fromarray(a)
            ref.putpalette(im.getpalette())
            buf = io.BytesIO()
            ref.save(buf, format='PNG')
            rows[os.path.relpath(os.path.join(dp, f), gold)] = {'device_bytes': mine, 'pil_bytes': len(buf.getvalue()),
                                                                 'ratio': round(mine / len(buf.getvalue()), 2)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'egress.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'egress_bench needs the MI355X'
    dev = torch.device('cuda:0')
    frames = make_frames(args.frames, dev)
    core = make_processor(dev)
    result = {'frames': args.frames, 'repeats': args.repeats, 'cpus': len(os.sched_getaffinity(0)), 'cases': {}}
    with torch.inference_mode():
        for case, shape in (('a_480p', None), ('b_480p_to_1080p', (1080, 1920))):
            legs = {'host': [], 'device': []}
            with tempfile.TemporaryDirectory() as tmp:                       # warm-up: code objects, pinned buffers, the allocator
                for eg in legs:
                    run_leg(frames[:20], core, eg, shape, os.path.join(tmp, eg))
            for rep in range(args.repeats):
                for eg in legs:
                    with tempfile.TemporaryDirectory() as tmp:
                        legs[eg].append(run_leg(frames, core, eg, shape, tmp))
            c = {'device_time': device_times(frames[0], shape, dev)}
            for eg, runs in legs.items():
                c[eg] = {'fps': [round(r['fps'], 1) for r in runs], 'fps_median': round(statistics.median(r['fps'] for r in runs), 1),
                         'fps_best': round(max(r['fps'] for r in runs), 1),
                         'process_ms_per_frame': [round(r['process_ms_per_frame'], 4) for r in runs],
                         'process_ms_per_frame_median': round(statistics.median(r['process_ms_per_frame'] for r in runs), 4),
                         'bytes_to_host_per_frame': runs[0]['bytes_to_host_per_frame'], 'file_bytes_mean': round(runs[0]['file_bytes_mean'])}
            c['device_median_fps_above_host_best'] = c['device']['fps_median'] > c['host']['fps_best']
            c['device_process_time_below_host_best'] = c['device']['process_ms_per_frame_median'] < min(c['host']['process_ms_per_frame'])
            result['cases'][case] = c
        result['golden_file_sizes'] = golden_sizes(dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
