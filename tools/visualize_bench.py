#!/usr/bin/env python
"""--visualize overlays, host against device (ResultSaver(overlay=...), PROB_TO_ID flags == 128, csrc/jpeg_enc.hip).

(1) Device time of the blend + JPEG stage per frame at 854 x 480 and 1920 x 1080, from device events around ONE op per sample with the
    caches cold: a 512 MB buffer (twice the Infinity Cache) is rewritten between the samples; median, min and max of the samples, and
    the warm figure (cutie_time_ops, back-to-back replays) next to it.  The frame is smooth content with a textured region, the id
    plane three discs: what an overlay looks like.
(2) Wall-clock frames/s of eval_vos.process_video(visualize=True) on a synthetic 854 x 480 video (cutie_amd/utils/synth.py, JPEG
    quality 95, 3 objects, random-init weights), ingest='device', egress='device': overlay='host' -- the code path the project had
    before the device overlay, which also takes the masks back to the host path -- against overlay='device', the legs alternating after
    a warm-up of each; plus the equality of the .jpg bytes of the two legs.

    python tools/visualize_bench.py [--frames 200] [--repeats 3] [--out profiles/visualize.json]

Needs the GPU (no fall-back)."""
import argparse
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
from cutie_amd import _lib, ops as O                                         # noqa: E402
from cutie_amd.inference.utils import jpeg_writer as JW                      # noqa: E402
from cutie_amd.inference.utils.results_utils import davis_palette, davis_palette_np   # noqa: E402


def overlay_inputs(H, W):
    y, x = np.mgrid[0:H, 0:W]
    rs = np.random.RandomState(H)
    a = np.stack([(y // 3 + x // 2) % 256, (x * y // 512) % 256, (y + 2 * x) // 7 % 256], -1).astype(np.uint8)
    a[H // 4:H // 2, W // 3:W // 2] = rs.randint(0, 256, (H // 2 - H // 4, W // 2 - W // 3, 3))
    ids = np.zeros((H, W), np.uint8)
    for k, (cy, cx) in enumerate(((0.3, 0.3), (0.6, 0.5), (0.5, 0.8))):
        ids[(y - cy * H) ** 2 + (x - cx * W) ** 2 < (0.15 * H) ** 2] = k + 1
    return a, ids


def host_blend(image_np, out_mask, all_obj_ids, colors):
    """results_utils.py _write_overlay: the host overlay's blend."""
    rgb_mask = np.zeros((*out_mask.shape, 3), dtype=np.uint8)
    for oid in all_obj_ids:
        rgb_mask[out_mask == oid] = colors[oid % len(colors)]
    alpha = ((out_mask == 0).astype(np.float32) * 0.5 + 0.5)[:, :, None]
    return (image_np * alpha + rgb_mask * (1 - alpha)).astype(np.uint8)


def stage_times(H, W, dev, samples=40):
    frame, ids = overlay_inputs(H, W)
    qt = JW.quant_tables()
    t = dict(frame=torch.from_numpy(frame).to(dev), ids=torch.from_numpy(ids).to(dev),
             colors=torch.from_numpy(JW.color_table(davis_palette_np, [1, 2, 3])).to(dev), qt=torch.from_numpy(qt.view(np.int16)).to(dev),
             stream=torch.empty(O.OpList.jpeg_enc_capacity(H, W), dtype=torch.uint8, device=dev), status=torch.empty(4, dtype=torch.int32, device=dev),
             scratch=torch.empty(O.OpList.jpeg_enc_scratch_words(H, W), dtype=torch.int32, device=dev))
    ol = O.OpList()
    ol.jpeg_encode(t['frame'], t['ids'], t['colors'], t['qt'], t['stream'], t['status'], t['scratch'], H=H, W=W)
    arr = ol.finalize()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
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
        cold.append(e0.elapsed_time(e1))
    warm = statistics.median(_lib.get_executor().time_ops(arr, 50) for _ in range(5))
    n = int(t['status'][0])
    assert int(t['status'][2]) == 0
    ref = io.BytesIO()
    Image.fromarray(host_blend(frame, ids, [1, 2, 3], davis_palette_np)).save(ref, 'JPEG')
    same = JW.wrap(t['stream'][:n].cpu().numpy().tobytes(), H, W, qt) == ref.getvalue()
    return {'cold_ms_median': round(statistics.median(cold), 4), 'cold_ms_min': round(min(cold), 4), 'cold_ms_max': round(max(cold), 4),
            'samples': samples, 'warm_ms_time_ops': round(warm, 4), 'stream_bytes': n, 'kernels': 8, 'equals_pil_of_host_blend': bool(same)}


def make_video(root, n, h=480, w=854, ids=(1, 2, 3), seed=9):
    from cutie_amd.utils.synth import SyntheticClip
    clip = SyntheticClip(h, w, len(ids), n, seed=seed)
    os.makedirs(os.path.join(root, 'JPEGImages', 'v')); os.makedirs(os.path.join(root, 'Annotations', 'v'))
    for t in range(n):
        arr = (clip.frame(t).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(root, 'JPEGImages', 'v', f'{t:05d}.jpg'), quality=95)
    lut = np.zeros(256, dtype=np.uint8)
    for k, oid in enumerate(ids):
        lut[k + 1] = oid
    png = Image.fromarray(lut[clip.first_mask().numpy()].astype(np.uint8))
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'Annotations', 'v', '00000.png'))


def _jpgs(root):
    return {f: open(os.path.join(dp, f), 'rb').read() for dp, _, fs in os.walk(root) for f in fs if f.endswith('.jpg')}


def driver_legs(dev, frames, repeats):
    from cutie_amd import eval_vos as E
    from cutie_amd.config import default_config
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from cutie_amd.model.cutie import CUTIE
    cfg = default_config()
    net = CUTIE(cfg).to(dev).eval()
    legs = {'host': [], 'device': []}
    files = {}
    with tempfile.TemporaryDirectory() as data:
        make_video(data, frames)

        def leg(overlay, out):
            rd = next(iter(VOSTestDataset(os.path.join(data, 'JPEGImages'), os.path.join(data, 'Annotations'), use_all_masks=False,
                                          ingest='device').get_datasets()))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = E.process_video(net, cfg, rd, os.path.join(out, 'm'), visualize=True, visualize_output_root=os.path.join(out, 'v'),
                                ingest='device', egress='device', overlay=overlay)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            return {'wall_s': wall, 'fps': r['frames'] / wall, 'model_fps': r['frames'] / r['seconds'], 'frames': r['frames']}
        for ov in legs:                                                      # warm-up: plans, code objects, pinned buffers
            with tempfile.TemporaryDirectory() as tmp:
                leg(ov, tmp)
        for rep in range(repeats):
            for ov in legs:
                with tempfile.TemporaryDirectory() as tmp:
                    legs[ov].append(leg(ov, tmp))
                    if rep == 0:
                        files[ov] = _jpgs(os.path.join(tmp, 'v'))
    out = {'frames': frames, 'frame': [480, 854], 'objects': 3, 'ingest': 'device', 'egress': 'device'}
    for ov, runs in legs.items():
        out[ov] = {k: [round(r[k], 3) for r in runs] for k in ('wall_s', 'fps', 'model_fps')}
        out[ov]['fps_median'] = round(statistics.median(r['fps'] for r in runs), 2)
    out['same_jpg_bytes'] = files['host'] == files['device'] and len(files['host']) == frames
    out['jpg_bytes_mean'] = round(sum(len(v) for v in files['device'].values()) / max(1, len(files['device'])))
    out['device_not_slower'] = out['device']['fps_median'] >= out['host']['fps_median']
    out['speedup'] = round(out['device']['fps_median'] / out['host']['fps_median'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'visualize.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'visualize_bench needs the MI355X'
    dev = torch.device('cuda:0')
    result = {'cpus': len(os.sched_getaffinity(0)), 'stage': {}}
    with torch.inference_mode():
        for H, W in ((480, 854), (1080, 1920)):
            result['stage'][f'{W}x{H}'] = stage_times(H, W, dev)
        result['driver'] = driver_legs(dev, args.frames, args.repeats)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
