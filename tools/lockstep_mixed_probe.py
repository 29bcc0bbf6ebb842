"""What does lock step buy clips that differ in their object count?  (LockstepCores(mixed_objects=True), profiles/lockstep_mixed.md)

Synthetic 854 x 480 clips, long-term memory on, four clips of (1, 3, 3, 5) objects -- 12 objects, the total of bench.py's 4 x 3 -- through
three legs on ONE box, each the median of five timed regions of --steps lock-step frames (bench.py's protocol: pre-roll to a steady bank,
warm-up, then regions between device synchronisations):

  one_by_one   the clips one after another on their own InferenceCore with look-ahead hints: what eval_vos does with them without the switch
  mixed        the four clips as ONE group with mixed_objects=True
  uniform      four clips of 3 objects as one group: the ceiling (the multi_clip leg of bench.py)

    python tools/lockstep_mixed_probe.py [--legs one_by_one,mixed,uniform] [--counts 1,3,3,5] [--steps 200] [--out result.json]

Prints one JSON line (frames/s = clip frames per second over all clips); legs that the checkout does not have (a parent commit without
mixed_objects) are reported as null.  Every leg runs in a fresh child process: a group that starts behind the one-clip leg in the same
process runs slower, on this tree and on its parent alike (profiles/lockstep_mixed.md, last section), so legs that share a process cannot
be compared."""
import argparse
import inspect
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def regions_fps(step, steps, regions, frames_per_step):
    vals = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        vals.append(frames_per_step * steps / (time.perf_counter() - t0))
    return vals


def clip_views(cl, NF, dev, depth):
    fr = torch.stack([cl.frame(t) for t in range(NF)]).to(dev)
    v = [fr[i] for i in range(NF)]
    return v + v[:depth + 1]


def leg_group(net, cfg, counts, args, dev, mixed):
    from cutie_amd.inference.lockstep import LockstepCores
    from cutie_amd.utils.synth import SyntheticClip
    NF, depth = 48, 16
    clips = [SyntheticClip(args.height, args.width, k, NF, seed=101 + c) for c, k in enumerate(counts)]
    views = [clip_views(cl, NF, dev, depth) for cl in clips]
    kw = dict(mixed_objects=True) if mixed else {}
    ls = LockstepCores(net, cfg, len(counts), **kw)
    hint = lambda t: {'next_images': [v[(t + 1) % NF:(t + 1) % NF + depth] for v in views]}
    t = [1]

    def step():
        ls.step([v[t[0] % NF] for v in views], **hint(t[0]))
        t[0] += 1
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        ls.step([v[0] for v in views], [cl.first_mask().to(dev) for cl in clips], [cl.objects for cl in clips])
        for _ in range(args.preroll + args.warmup):
            step()
        before = ls.batched_steps
        vals = regions_fps(step, args.steps, args.regions, len(counts))
        assert ls.batched_steps - before == args.steps * args.regions, 'every timed frame of a group must run as one plan per stage'
    return vals


def leg_one_by_one(net, cfg, counts, args, dev):
    """Clip after clip; a region's time is the sum over the clips, so its frames/s is comparable with a group's."""
    from cutie_amd.inference import inference_core as IC
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.utils.synth import SyntheticClip
    NF = 48
    depth = IC.WINDOW + IC.WINDOW_LEAD + 2
    secs = [0.0] * args.regions
    st = torch.cuda.Stream(device=dev)
    for c, k in enumerate(counts):
        cl = SyntheticClip(args.height, args.width, k, NF, seed=101 + c)
        v = clip_views(cl, NF, dev, depth)
        proc = InferenceCore(net, cfg=cfg)
        hint = lambda t: {'next_images': v[(t + 1) % NF:(t + 1) % NF + depth]}
        t = [1]

        def step():
            proc.step(v[t[0] % NF], **hint(t[0]))
            t[0] += 1
        with torch.cuda.stream(st):
            proc.step(v[0], cl.first_mask().to(dev), objects=cl.objects, **hint(0))
            for _ in range(args.preroll + args.warmup):
                step()
            for r, fps in enumerate(regions_fps(step, args.steps, args.regions, 1)):
                secs[r] += args.steps / fps
    return [len(counts) * args.steps / s for s in secs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='one_by_one,mixed,uniform')
    ap.add_argument('--counts', default='1,3,3,5')
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=854)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--preroll', type=int, default=300)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    counts = tuple(int(v) for v in args.counts.split(','))
    legs = args.legs.split(',')
    if len(legs) > 1:                                        # one fresh process per leg (this one never opens the GPU)
        out = None
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), '--legs', leg, '--counts', args.counts, '--height', str(args.height), '--width', str(args.width),
                   '--steps', str(args.steps), '--warmup', str(args.warmup), '--preroll', str(args.preroll), '--regions', str(args.regions)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                raise SystemExit(f'leg {leg} failed with exit status {r.returncode}')
            one = json.loads(r.stdout.strip().split('\n')[-1])
            if out is None:
                out = one
            else:
                out['legs'].update(one['legs'])
        finish(out, args)
        return
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    from cutie_amd.config import default_config
    from cutie_amd.inference.lockstep import LockstepCores
    from cutie_amd.model.cutie import CUTIE
    from cutie_amd.utils.synth_weights import make_state_dict
    cfg = default_config(use_long_term=True)
    torch.manual_seed(0)
    net = CUTIE(cfg).to(dev).eval()
    net.load_weights(make_state_dict(seed=0))
    has_mixed = 'mixed_objects' in inspect.signature(LockstepCores.__init__).parameters
    out = {'counts': list(counts), 'size': [args.height, args.width], 'steps': args.steps, 'regions': args.regions,
           'device': torch.cuda.get_device_name(dev), 'has_mixed_objects': has_mixed, 'legs': {}}
    with torch.inference_mode():
        for leg in args.legs.split(','):
            if leg == 'one_by_one':
                vals = leg_one_by_one(net, cfg, counts, args, dev)
            elif leg == 'mixed':
                vals = leg_group(net, cfg, counts, args, dev, True) if has_mixed else None
            elif leg == 'uniform':
                vals = leg_group(net, cfg, (3,) * len(counts), args, dev, False)
            else:
                raise SystemExit(f'unknown leg {leg}')
            out['legs'][leg] = None if vals is None else {'fps_median': round(sorted(vals)[len(vals) // 2], 1), 'fps_regions': [round(v, 1) for v in vals]}
    finish(out, args)


def finish(out, args):
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
