"""Times the polygon trace (PROB_TO_ID flags == 8192, csrc/polygons.hip) on one MI355X and writes profiles/polygons.md:

(1) the stage with cutie_time_ops at 854x480 and 1920x1080 on the three-blob mask (3 objects) of profiles/region_filter.md, with the one-
    workgroup path where the plane's edges allow it (i6 = 0) and on the general chain (i6 = 1), at the saver's edge capacity and at the
    plane's worst case, next to the track statistics and the plain PROB_TO_ID kernel on planes of the same size; and the general chain on
    0.5-density noise, where every round has work;
(2) the experiment of DESIGN.md section 15: eval_vos.run_dataset over four copies of a 96-frame 854x480 clip with --egress device
    --lockstep 4, wall-clock frames/s of the second pass, without the switch and with --polygons; every sample in a fresh process, the
    legs interleaved, their order rotating from round to round.

    python tools/polygon_probe.py [--frames 96] [--rounds 3] [--out profiles/polygons.md]

Needs the GPU (no fall-back)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from tools.region_probe import planes        # noqa: E402  (the same planes as profiles/region_filter.md)
from tools.track_probe import clips          # noqa: E402  (the same clips as profiles/track_report.md)


def stage_rows(iters=50):
    from cutie_amd import _lib, ops as O
    from cutie_amd.inference.utils.results_utils import POLY_EDGES
    rows = []
    ex = _lib.get_executor()

    def timed(ol):
        arr = ol.finalize()
        us = [ex.time_ops(arr, iters) * 1e3 for _ in range(5)]
        return f'{statistics.median(us):.1f} | {min(us):.1f} - {max(us):.1f}'

    def rounds(cap):
        return max(cap - 1, 0).bit_length()
    for H, W in ((480, 854), (1080, 1920)):
        named = dict((n, p) for n, p in planes(H, W))
        blobs = torch.from_numpy(named['three blobs']).cuda()
        table = torch.empty((3, 12), dtype=torch.int32, device='cuda')
        ol = O.OpList()
        ol.track_stats(blobs, [1, 2, 3], table)
        rows.append(f'| {W}x{H} | three blobs | track statistics, id plane only (3 launches) | {timed(ol)} |')
        prob = torch.rand((4, H, W), device='cuda').softmax(0).contiguous()
        lut = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device='cuda')
        ol = O.OpList()
        ol.prob_to_id(prob, lut, torch.empty((H, W), dtype=torch.uint8, device='cuda'), P=4, H=H, W=W, plane=prob.stride(0), ldrow=prob.stride(1))
        rows.append(f'| {W}x{H} | 4 planes | plain PROB_TO_ID (1 launch) | {timed(ol)} |')
        stream_bytes, worst = O.OpList.polygon_capacity(H, W)
        for name, caps in (('three blobs', (POLY_EDGES, worst)), ('0.5-density noise', (worst,))):
            src = torch.from_numpy(named[name]).cuda()
            for cap in caps:
                scratch = torch.empty(O.OpList.polygon_scratch_words(H, W, 3, cap), dtype=torch.int32, device='cuda')
                stream = torch.empty(stream_bytes // 4, dtype=torch.int32, device='cuda')
                tab, status = torch.empty(12, dtype=torch.int32, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
                for path in (0, 1):
                    ol = O.OpList()
                    ol.polygon_trace(src, [1, 2, 3], stream, tab, status, scratch, connectivity=8, edge_capacity=cap, path=path)
                    t = timed(ol)
                    st = status.cpu().tolist()
                    small = path == 0 and st[3] <= O.OpList.POLY_SMALL_EDGES
                    what = 'one workgroup; the chain behind it returns at once' if small else 'general chain'
                    rows.append(f'| {W}x{H} | {name}: E = {st[3]}, R = {st[2]}, {st[0]} bytes | polygon trace, i6 = {path}, E_cap = {cap} '
                                f'({8 + rounds(cap) + (1 - path)} launches, {rounds(cap)} of them rounds; {what}) | {t} |')
    return rows


# one sample -- run_dataset twice, the second pass timed -- in a process of its own
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
reports = [json.load(open(os.path.join(out, 'polygons', v, 'polygons.json'))) for v in (os.listdir(os.path.join(out, 'polygons')) if os.path.isdir(os.path.join(out, 'polygons')) else [])]
print('LEG ' + json.dumps({'fps': fps, 'reported': sum(len(r['frames']) for r in reports)}))
'''


def leg(root, frames, extra):
    p = subprocess.run([sys.executable, '-c', LEG, root, str(frames)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f'leg {extra} failed ({p.returncode}): {p.stderr[-2000:]}')
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith('LEG ')][-1][4:])
    assert r['reported'] == (4 * frames if extra else 0), r
    return r['fps']


def run_rows(frames, rounds):
    legs = [('no switch', []), ('--polygons', ['--polygons'])]
    fps = {name: [] for name, _ in legs}
    root = tempfile.mkdtemp(prefix='polygon_probe_')
    try:
        clips(root, frames)
        for k in range(rounds):                  # (the order rotates: every leg runs first, second in turn)
            for name, extra in legs[k % len(legs):] + legs[:k % len(legs)]:
                fps[name].append(leg(root, frames, extra))
                print(f'{name}: {fps[name][-1]:.1f} frames/s', flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return [f'| {name} | ' + ' / '.join(f'{v:.1f}' for v in vs) + f' | {statistics.median(vs):.1f} |' for name, vs in fps.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'polygons.md'))
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--notes', help='a file whose text is appended (what the figures mean)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'polygon_probe needs the MI355X'
    lines = ['# Polygon trace: tools/polygon_probe.py', '', f'device: {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} CPUs', '',
             'Stage time: cutie_time_ops, 50 back-to-back replays (warm caches), median of 5 (min - max), microseconds per replay of the whole chain; '
             '3 listed objects, connectivity 8, the stream at the plane\'s worst case.', '',
             '| size | plane | launches | us | min - max |', '|---|---|---|---|---|'] + stage_rows()
    lines += ['', f'eval_vos.run_dataset over 4 clips of {args.frames} frames of 854x480 (--egress device --lockstep 4), wall-clock frames/s of the second pass; '
              f'every sample in a fresh process, the legs interleaved and their order rotating, {args.rounds} rounds:', '', '| run | frames/s per round | median |', '|---|---|---|']
    lines += run_rows(args.frames, args.rounds)
    lines += ['', 'The parent commit was not measured in this run: without the switch this tree issues the parent\'s launches.']
    if args.notes:
        lines += ['', open(args.notes).read().rstrip('\n')]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
