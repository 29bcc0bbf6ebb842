"""Device ingest probe (profiles/ingest_probe.md, profiles/jpeg_decode.md): what the host pays per frame in each ingest mode, and what
the GPU pays.

    python tools/ingest_probe.py cpu [--frames 24]            # host ms/frame of VideoReader[i] per mode, inline and ReadAhead(4)
    python tools/ingest_probe.py gpu [--frames 40]            # RESIZE flags 4 / 6 and the JPEG decode us per frame (events), the decode's
                                                              # sync rounds / serial segments, eval_vos wall-clock frames/s per mode
    python tools/ingest_probe.py decode [--frames 40]         # only the JPEG decodes at 480p / 720p / 1080p, for
                                                              # rocprofv3 --kernel-trace --stats (per-stage kernel times)
        [--batch 1 4 8 16]                                    # ... the same frames N per call: 1 = the one-frame forms (jpeg_to_device),
                                                              # N > 1 = the batch forms (jpegs_to_device, RESIZE flags 256)
    python tools/ingest_probe.py gpu --decode-batch 4 8 16    # ... the eval_vos legs also with 'device-decode' and --decode-batch N
    [--out FILE.md]                                           # also append the markdown table to FILE

Synthetic JPEG folders (smooth random content, quality 90) are generated in a temporary directory.  The eval_vos numbers are
WALL-CLOCK around process_video / process_videos_lockstep (synchronised), not the driver's own step time, which excludes ingest."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SIZES = {'480p': (480, 854, -1), '720p': (720, 1280, 480), '1080p': (1080, 1920, 480)}
MODES = ('host', 'device', 'device-decode')


def make_video(root, name, n, h, w, seed, ids=(1, 2)):
    from cutie_amd.inference.utils.results_utils import davis_palette
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'JPEGImages', name)); os.makedirs(os.path.join(root, 'Annotations', name))
    base = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
    for t in range(n):
        small = np.roll(base, t, axis=1)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(os.path.join(root, 'JPEGImages', name, f'{t:05d}.jpg'), quality=90)
    m = np.zeros((h, w), dtype=np.uint8)
    for k, oid in enumerate(ids):
        m[h // 4 * k + h // 8: h // 4 * k + h // 4, w // 4: w // 2 + k * w // 8] = oid
    png = Image.fromarray(m)
    png.putpalette(davis_palette)
    png.save(os.path.join(root, 'Annotations', name, '00000.png'))


def cpu_part(frames):
    from cutie_amd.inference.data.prefetch import ReadAhead
    from cutie_amd.inference.data.video_reader import VideoReader
    rows = ['| source | size | mode | inline ms/frame | ReadAhead(4) ms/frame |', '|---|---|---|---|---|']
    ratios = {}
    with tempfile.TemporaryDirectory() as root:
        for tag, (h, w, size) in SIZES.items():
            make_video(root, tag, frames, h, w, seed=1)
            res = {}
            for mode in MODES:
                rd = VideoReader(tag, os.path.join(root, 'JPEGImages', tag), os.path.join(root, 'Annotations', tag), size=size, ingest=mode)
                rd[0]
                t0 = time.perf_counter()
                for i in range(len(rd)):
                    rd[i]
                inline = (time.perf_counter() - t0) / len(rd) * 1e3
                t0 = time.perf_counter()
                for _ in ReadAhead(rd, workers=4):
                    pass
                ahead = (time.perf_counter() - t0) / len(rd) * 1e3
                res[mode] = (inline, ahead)
                rows.append(f'| {w}x{h} | {size} | {mode} | {inline:.2f} | {ahead:.2f} |')
            ratios[tag] = {m: (res[m][0] / res['host'][0], res[m][1] / res['host'][1]) for m in MODES[1:]}
    rows.append('')
    for m in MODES[1:]:
        rows.append(f'{m} / host: ' + ', '.join(f'{k} {r[m][0]:.2f} inline, {r[m][1]:.2f} read-ahead' for k, r in ratios.items()))
    return rows


def decode_part(frames, rows=None, batches=(1,)):
    """The GPU JPEG decode of one synthetic frame per size, `frames` times after a warm-up: us per frame (events, packet upload
    included), and the sync statistics of the last decode.  batches: frames per call -- 1 is jpeg_to_device (the one-frame forms),
    N > 1 is jpegs_to_device over N copies of the frame (the batch forms), frames // N calls."""
    from cutie_amd.inference.data import device_ingest as D
    from cutie_amd.inference.data import jpeg as J
    rows = rows if rows is not None else []
    rows += ['| JPEG decode (device_ingest.jpeg_to_device / jpegs_to_device, native size) | frames per call | bytes | chunks | us per frame (events) | sync rounds | serial segments |',
             '|---|---|---|---|---|---|---|']
    with tempfile.TemporaryDirectory() as root:
        for tag, (h, w, _) in SIZES.items():
            make_video(root, tag, 1, h, w, seed=3)
            pkt, why = J.parse_file(os.path.join(root, 'JPEGImages', tag, '00000.jpg'))
            assert pkt is not None, why
            for B in batches:
                staging = D.PngStaging()

                def call():
                    if B == 1:
                        D.jpeg_to_device(pkt, 'cuda', stream=torch.cuda.current_stream())
                    else:
                        D.jpegs_to_device([pkt] * B, 'cuda', stream=torch.cuda.current_stream(), staging=staging)
                calls = max(1, frames // B)
                for _ in range(5):
                    call()
                torch.cuda.synchronize()
                stats0 = dict(D.decode_stats)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                serial = D.decode_stats['serial_segments'] - stats0['serial_segments']
                rows.append(f'| {w}x{h} | {B} | {pkt.buf.nbytes} | {int(pkt.hdr[J.HDR_NCHUNK])} | {e0.elapsed_time(e1) / (calls * B) * 1e3:.1f} | '
                            f'{D.decode_stats["max_sync_rounds"]} | {serial} |')
    return rows


def gpu_part(frames, decode_batches=()):
    from cutie_amd import ops as O
    from cutie_amd.config import default_config
    from cutie_amd.eval_vos import process_video, process_videos_lockstep
    from cutie_amd.inference.data.vos_test_dataset import VOSTestDataset
    from cutie_amd.model.cutie import CUTIE
    from oracle.weights import make_state_dict
    rows = ['| kernel | geometry | us per frame (events, 200 launches) |', '|---|---|---|']
    for (H, W, OH, OW) in ((1080, 1920, 480, 853), (720, 1280, 480, 853), (480, 854, 480, 854)):
        src = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device='cuda')
        dst = torch.empty((3, OH, OW), device='cuda')
        ol = O.OpList(prio=False)
        if (H, W) == (OH, OW):
            ol.resize(src, dst, C=3, H=H, W=W, OH=OH, OW=OW, plane=0, ldrow=W * 3, src_u8=True)
        else:
            ol.resize(src, dst, C=3, H=H, W=W, OH=OH, OW=OW, plane=0, ldrow=W * 3, src_u8=True, antialias=True,
                      taps=torch.from_numpy(O.resize_aa_table(H, W, OH, OW)).cuda(), scratch=torch.empty((3, H, OW), device='cuda'))
        ol.finalize()
        for _ in range(20):
            ol.run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            ol.run()
        e1.record()
        torch.cuda.synchronize()
        rows.append(f'| RESIZE flags {int(ol.arr["flags"][0])} | {W}x{H} -> {OW}x{OH} | {e0.elapsed_time(e1) / 200 * 1e3:.1f} |')
    rows.append('')
    decode_part(frames, rows)
    rows += ['', '| eval_vos (1280x720, --size 480, 4 videos) | ingest | decode batch | frames | wall s | wall frames/s | step-only frames/s |',
             '|---|---|---|---|---|---|---|']
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    cfg = default_config()
    with tempfile.TemporaryDirectory() as root:
        for v in range(4):
            make_video(root, f'v{v}', frames, 720, 1280, seed=10 + v)
        for lockstep in (1, 4):
            legs = [(m, 1) for m in MODES] + [('device-decode', B) for B in decode_batches if B > 1]
            for mode, B in legs + legs:                                    # each leg twice: the first pass warms plans and allocator
                ds = VOSTestDataset(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'), use_all_masks=False, size=480, ingest=mode)
                rds = list(ds.get_datasets())
                out = os.path.join(root, f'out_{mode}_{B}_{lockstep}')
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.inference_mode():
                    if lockstep == 1:
                        st = [process_video(net, cfg, rd, out, decode_batch=B) for rd in rds]
                    else:
                        st = list(process_videos_lockstep(net, cfg, rds, out, decode_batch=B).values())
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                n = sum(s['frames'] for s in st)
                step = sum(s['seconds'] for s in st)
                rows.append(f'| --lockstep {lockstep} | {mode} | {B} | {n} | {wall:.2f} | {n / wall:.0f} | {n / max(step, 1e-9):.0f} |')
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('part', choices=['cpu', 'gpu', 'decode'])
    ap.add_argument('--frames', type=int, default=None)
    ap.add_argument('--out')
    ap.add_argument('--batch', type=int, nargs='+', default=[1], help='decode: frames per call (1: the one-frame forms)')
    ap.add_argument('--decode-batch', type=int, nargs='+', default=[], help="gpu: eval_vos legs with 'device-decode' and this decode_batch")
    a = ap.parse_args()
    if min(a.batch + a.decode_batch) < 1:
        ap.error('--batch / --decode-batch are at least 1')
    frames = a.frames or (24 if a.part == 'cpu' else 40)
    if a.part == 'cpu':
        rows = cpu_part(frames)
    elif a.part == 'gpu':
        rows = gpu_part(frames, tuple(a.decode_batch))
    else:
        rows = decode_part(frames, batches=tuple(a.batch))
    text = '\n'.join(rows) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
