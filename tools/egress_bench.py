#!/usr/bin/env python
"""Result egress, host against device (ResultSaver(egress=...)): a fixed seeded sequence of probability frames (K = 3 objects) goes through
ResultSaver into a temporary directory, (a) 854 x 480 as it is and (b) 854 x 480 resampled to 1920 x 1080, each with egress='host' (the id
plane is copied, PIL encodes) and egress='device' (fused resample + argmax, PNG stream written by the GPU), the legs alternating in one
process.  Reported per case and leg: end-to-end frames/s (wall clock from the first `process` to the return of `end()`), the time the
stepping thread spends inside `process` per frame, bytes copied to the host per frame, and file sizes; per case the device time of the
egress launches (cutie_time_ops, median of the replays): the RESIZE + PROB_TO_ID pair against the fused kernel, and the deflate stages.

    python tools/egress_bench.py [--frames 300] [--repeats 5] [--out profiles/egress.json]

    python tools/egress_bench.py --multiscale [--repeats 5] [--out profiles/multiscale.json]

--multiscale: the multi-scale merge instead (PROB_TO_ID flags&16): the device time of the merge op against the chain it replaces, and the
whole protocol -- S runs with save_scores + merge_multi_scale against one process_video_multiscale run -- on copies of the bike example.

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

    def _mask_stream(self, b):
        data = super()._mask_stream(b)
        head = b.png.host.numel()
        self.copied += head + max(0, len(data) - (head - 16))
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


# ---- multi-scale leg (--multiscale): the one-pass merge against the file route --------------------------------------------------------
MS_SIZES = (240, 320, 400)


def merge_op_times(dev, repeats, iters=20):
    """Device time of the merge op (S = 3 sources of 480p class -> 1080p, P = 4) against the chain it replaces: 3 x (RESIZE + quantise) +
    integer sum + argmax + lut.  Both timed with events around `iters` runs, the legs alternating; the op also through cutie_time_ops."""
    srcs, (H, W), P = [(480, 854), (600, 1067), (720, 1280)], (1080, 1920), 4
    probs = [_smooth_probs(P, h, w, seed=k).to(dev) for k, (h, w) in enumerate(srcs)]
    lut = torch.arange(P, dtype=torch.int32, device=dev)
    ids = torch.empty((H, W), dtype=torch.uint8, device=dev)
    full = [torch.empty((P, H, W), dtype=torch.float32, device=dev) for _ in srcs]
    fused = O.OpList()
    fused.prob_to_id_merged(probs, lut, ids, out_hw=(H, W))
    fused.finalize()
    rs = O.OpList()
    for p, f in zip(probs, full):
        rs.resize(p, f, C=P, H=p.shape[1], W=p.shape[2], OH=H, OW=W, plane=p.stride(0), ldrow=p.stride(1))
    rs.finalize()

    def chain():
        rs.run()
        total = (full[0] * 255).to(torch.uint8).to(torch.int32)
        for f in full[1:]:
            total += (f * 255).to(torch.uint8).to(torch.int32)
        return lut[total.argmax(0)].to(torch.uint8)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    for fn in (fused.run, chain):                                            # warm-up
        timed(fn)
    legs = {'merge_op_ms': [], 'chain_ms': []}
    for _ in range(repeats):
        legs['merge_op_ms'].append(timed(fused.run))
        legs['chain_ms'].append(timed(chain))
    out = {k: [round(v, 4) for v in vs] for k, vs in legs.items()}
    out.update({k + '_median': round(statistics.median(vs), 4) for k, vs in legs.items()})
    out['merge_op_time_ops_ms'] = round(statistics.median(_lib.get_executor().time_ops(fused.arr, 50) for _ in range(7)), 4)
    out['resize_x3_time_ops_ms'] = round(statistics.median(_lib.get_executor().time_ops(rs.arr, 50) for _ in range(7)), 4)
    out['equal_ids'] = bool(torch.equal(ids, chain()))
    out['geometry'] = {'sources': srcs, 'output': [H, W], 'planes': P}
    return out


def _tree_bytes(root):
    n = b = 0
    for dp, _, fs in os.walk(root):
        for f in fs:
            n, b = n + 1, b + os.path.getsize(os.path.join(dp, f))
    return n, b


def multiscale_protocol(dev, repeats, videos=2, frames=16):
    """The whole protocol on `videos` copies of the bike example cycled to `frames` frames each (854 x 480, sizes 240 / 320 / 400,
    random-init weights, egress='device'): the file route -- S runs with save_scores, then merge_multi_scale -- against ONE multi-scale
    run; wall clock, masks per second and bytes written, the legs alternating after a warm-up of each.  Also the members' `seconds`
    (time around step) in both routes and the stepping thread's time inside process_merged."""
    import shutil
    from cutie_amd import eval_vos as E
    from cutie_amd.config import default_config
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from cutie_amd.merge_multi_scale import merge
    from cutie_amd.model.cutie import CUTIE
    cfg = default_config()
    net = CUTIE(cfg).to(dev).eval()
    src = os.path.join(ROOT, 'tests', 'golden', 'bike')
    jpgs = sorted(f for f in os.listdir(src) if f.endswith('.jpg'))
    inside = [0.0]
    plain = ResultSaver.process_merged

    def counted(self, *a, **k):
        t = time.perf_counter()
        r = plain(self, *a, **k)
        inside[0] += time.perf_counter() - t
        return r
    ResultSaver.process_merged = counted
    legs = {'file_route': [], 'one_pass': []}
    try:
        with tempfile.TemporaryDirectory() as data:
            for v in range(videos):
                img, msk = os.path.join(data, 'JPEGImages', f'v{v}'), os.path.join(data, 'Annotations', f'v{v}')
                os.makedirs(img)
                os.makedirs(msk)
                for t in range(frames):
                    shutil.copy(os.path.join(src, jpgs[t % len(jpgs)]), os.path.join(img, f'{t:05d}.jpg'))
                shutil.copy(os.path.join(src, '00000.png'), msk)
            scales = [list(VOSTestDataset(os.path.join(data, 'JPEGImages'), os.path.join(data, 'Annotations'), use_all_masks=False,
                                          size=s).get_datasets()) for s in MS_SIZES]

            def file_route(out):
                t0, secs = time.perf_counter(), 0.0
                runs = []
                for s, sc in zip(MS_SIZES, scales):
                    run = os.path.join(out, f'run{s}')
                    for rd in sc:
                        secs += E.process_video(net, cfg, rd, os.path.join(run, 'Annotations'), save_scores=True,
                                                score_output_root=os.path.join(run, 'Scores'), egress='device')['seconds']
                    runs.append(run)
                t1 = time.perf_counter()
                n = merge(runs, os.path.join(out, 'merged'), 'D', num_proc=4)
                t2 = time.perf_counter()
                files, nbytes = _tree_bytes(out)
                return {'wall_s': t2 - t0, 'runs_s': t1 - t0, 'merge_s': t2 - t1, 'masks': n, 'masks_per_s': n / (t2 - t0), 'step_seconds': secs,
                        'files_written': files, 'bytes_written': nbytes}

            def one_pass(out):
                inside[0] = 0.0
                t0, secs, n = time.perf_counter(), 0.0, 0
                for c in range(videos):
                    r = E.process_video_multiscale(net, cfg, [sc[c] for sc in scales], os.path.join(out, 'Annotations'), egress='device')
                    secs, n = secs + r['seconds'], n + r['frames']
                wall = time.perf_counter() - t0
                files, nbytes = _tree_bytes(out)
                return {'wall_s': wall, 'masks': n, 'masks_per_s': n / wall, 'step_seconds': secs, 'process_merged_ms_per_frame': 1e3 * inside[0] / n,
                        'files_written': files, 'bytes_written': nbytes}
            for leg in (file_route, one_pass):                               # warm-up: plans, code objects, pinned buffers
                with tempfile.TemporaryDirectory() as tmp:
                    leg(tmp)
            for _ in range(repeats):
                for name, leg in (('file_route', file_route), ('one_pass', one_pass)):
                    with tempfile.TemporaryDirectory() as tmp:
                        legs[name].append(leg(tmp))
    finally:
        ResultSaver.process_merged = plain
    out = {'videos': videos, 'frames_per_video': frames, 'sizes': list(MS_SIZES), 'frame': [480, 854]}
    for name, runs in legs.items():
        out[name] = {k: [round(r[k], 4) if isinstance(r[k], float) else r[k] for r in runs] for k in runs[0]}
        out[name]['wall_s_median'] = round(statistics.median(r['wall_s'] for r in runs), 4)
        out[name]['step_seconds_median'] = round(statistics.median(r['step_seconds'] for r in runs), 4)
    out['one_pass_faster'] = out['one_pass']['wall_s_median'] < out['file_route']['wall_s_median']
    return out


def multiscale_main(args, dev):
    result = {'repeats': args.repeats, 'cpus': len(os.sched_getaffinity(0))}
    with torch.inference_mode():
        result['merge_op'] = merge_op_times(dev, args.repeats)
        result['protocol'] = multiscale_protocol(dev, args.repeats)
    out = args.out if args.out != os.path.join(ROOT, 'profiles', 'egress.json') else os.path.join(ROOT, 'profiles', 'multiscale.json')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def _smooth_probs(P, h, w, seed):
    """Seeded object-like softmax planes [P, h, w] (low-frequency logits, sharpened)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, h, w, generator=g) * 0.3
    x = x + F.interpolate(torch.randn(1, P, max(h // 16, 2), max(w // 16, 2), generator=g), size=(h, w), mode='bicubic', align_corners=False)[0] * 4
    return torch.softmax(x, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'egress.json'))
    ap.add_argument('--multiscale', action='store_true', help='the multi-scale leg instead: merge op against its chain, one-pass run against the '
                                                              'file route (profiles/multiscale.json)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'egress_bench needs the MI355X'
    dev = torch.device('cuda:0')
    if args.multiscale:
        return multiscale_main(args, dev)
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
