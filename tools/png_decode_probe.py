"""Times the PNG decode stages (RESIZE flags 64 / 128, csrc/png_dec.hip) on one MI355X and writes profiles/png_decode.md: kernel time from
cutie_time_ops for palette masks at 854x480 and 1920x1080, one image and a batch of 64, the all-Paeth worst case, PIL's decode of the same
files on the same box, score_masks wall clock over a folder in both decode modes, and the experiment of DESIGN.md section 15 again:
eval_vos.run_dataset over four copies of a 96-frame 854x480 clip, second pass, without --score, with --score (host decode) and with --score
--gt-decode device, one clip at a time and with --lockstep 4, three interleaved rounds each (the spread is given, not one number).

    python tools/png_decode_probe.py [--out profiles/png_decode.md] [--parent ROWS.md ...]
    python tools/png_decode_probe.py --baseline --out ROWS.md     (in a checkout of the parent commit, with this file copied in: the runs it
                                                                   can make -- no --score, --score -- as raw rows; --parent joins them)
"""
import argparse
import io
import os
import sys
import tempfile
import time
import zlib

import numpy as np
import torch
from PIL import Image

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))



def _png_modules():
    """(not at import time: --baseline runs in a checkout that has none of them)"""
    from cutie_amd import _lib, ops as O
    from cutie_amd.inference.data import png_packet as P
    import png_corpus as C
    return _lib, O, P, C


def mask(H, W, seed):
    yy, xx = np.mgrid[:H, :W]
    rng = np.random.default_rng(seed)
    ids = np.zeros((H, W), dtype=np.uint8)
    for k in range(1, 5):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(H // 8, H // 3)
        ids[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k
    return ids


def pil_file(ids):
    im = Image.fromarray(ids)
    im.putpalette(bytes(range(48)) * 16)
    f = io.BytesIO()
    im.save(f, format='PNG')
    return f.getvalue()


def paeth_file(ids):
    C = _png_modules()[3]
    H, W = ids.shape
    return C.png_file(W, H, 8, 3, zlib.compress(C.filter_rows(ids, 1, [4]), 6))


def kernel_ms(packets, iters=20):
    _lib, O, P, C = _png_modules()
    table, pb, ib, ob = O.OpList.png_layout(packets)
    blob = np.zeros(pb, dtype=np.uint8)
    for k, pk in enumerate(packets):
        blob[table[k, 0]:table[k, 0] + pk.buf.nbytes] = pk.buf
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    pk_dev, tab = dev(blob), dev(table)
    infl, out = torch.empty(ib, dtype=torch.uint8, device='cuda'), torch.empty(ob, dtype=torch.uint8, device='cuda')
    status = torch.empty((len(packets), 4), dtype=torch.int32, device='cuda')
    res = []
    for stage in ('png_inflate', 'png_unfilter'):
        ol = O.OpList()
        if stage == 'png_inflate':
            ol.png_inflate(pk_dev, tab, infl, status, n=len(packets))
        else:
            ol.png_unfilter(pk_dev, tab, infl, out, status, n=len(packets))
        res.append(_lib.get_executor().time_ops(ol.finalize(), iters))
    assert not status.cpu().numpy()[:, 0].any()
    return res, status.cpu().numpy()[:, 3].mean()


def pil_ms(data, iters=20):
    t = time.perf_counter()
    for _ in range(iters):
        np.array(Image.open(io.BytesIO(data)))
    return (time.perf_counter() - t) / iters * 1e3


def clips(root, frames, copies=4):
    """`copies` videos of `frames` frames: the tests/golden/bike frames back and forth, ground truth = shifted copies of the first mask."""
    import shutil
    src = os.path.join(ROOT, 'tests', 'golden', 'bike')
    first = Image.open(os.path.join(src, '00000.png'))
    ids = np.array(first)
    for c in range(copies):
        img, msk, gt = (os.path.join(root, d, f'bike{c}') for d in ('JPEGImages', 'Annotations', 'GT'))
        for d in (img, msk, gt):
            os.makedirs(d)
        shutil.copy(os.path.join(src, '00000.png'), msk)
        for t in range(frames):
            k = t % 4 if (t // 4) % 2 == 0 else 3 - t % 4
            shutil.copy(os.path.join(src, f'0000{k}.jpg'), os.path.join(img, f'{t:05d}.jpg'))
            im = Image.fromarray(np.roll(ids, (2 * k, 5 * k), (0, 1)))
            im.putpalette(first.getpalette())
            im.save(os.path.join(gt, f'{t:05d}.png'))


def run_rows(frames, baseline, rounds=3):
    """frames/s of eval_vos.run_dataset (device egress), second pass, `rounds` interleaved rounds per configuration."""
    import shutil
    from cutie_amd import eval_vos as E
    from cutie_amd.config import default_config
    from cutie_amd.model.cutie import CUTIE
    from oracle import scenarios as S
    cfg = default_config()
    net = CUTIE(cfg).cuda().eval()
    net.load_weights(S.decisive_state_dict())
    root = tempfile.mkdtemp(prefix='png_probe_')
    who = 'parent commit' if baseline else 'this tree'
    modes = ('none', 'host') if baseline else ('none', 'host', 'device')
    fps = {}
    try:
        clips(root, frames)
        for rnd in range(rounds):
            for lock in (1, 4):
                for mode in modes:
                    argv = ['--images', os.path.join(root, 'JPEGImages'), '--masks', os.path.join(root, 'Annotations'), '--output',
                            os.path.join(root, f'out_{mode}_{lock}'), '--dataset', 'd17-val', '--egress', 'device']
                    if mode != 'none':
                        argv += ['--score', '--gt', os.path.join(root, 'GT')]
                    if mode == 'device':
                        argv += ['--gt-decode', 'device']
                    if lock > 1:
                        argv += ['--lockstep', str(lock)]
                    ap = E.arg_parser()
                    args = ap.parse_args(argv)
                    E.check_args(ap, args)
                    for _ in range(2):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        E.run_dataset(net, cfg, args)
                        torch.cuda.synchronize()
                        last = 4 * frames / (time.perf_counter() - t0)
                    fps.setdefault((lock, mode), []).append(last)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    name = {'none': 'no --score', 'host': '--score (host decode)', 'device': '--score --gt-decode device'}
    return [f"| {who}, {'one clip at a time' if lock == 1 else '--lockstep 4'}: {name[mode]} | " + ' / '.join(f'{v:.1f}' for v in vs) + ' |'
            for (lock, mode), vs in sorted(fps.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_decode.md'))
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--baseline', action='store_true', help='only the eval_vos runs a checkout of the parent commit can make, as raw table rows')
    ap.add_argument('--parent', nargs='*', default=[], help='row files of --baseline runs of the parent commit on the same box')
    args = ap.parse_args()
    if args.baseline:
        text = '\n'.join(run_rows(args.frames, True)) + '\n'
        print(text)
        with open(args.out, 'w') as f:
            f.write(text)
        return
    _lib, O, P, C = _png_modules()
    lines = ['# PNG decode on the device: tools/png_decode_probe.py', '', f'device: {torch.cuda.get_device_name(0)}', '',
             '| case | images | inflate ms | unfilter ms | per image ms | tokens / image | PIL ms / image |', '|---|---|---|---|---|---|---|']
    for label, (H, W) in (('480p', (480, 854)), ('1080p', (1080, 1920))):
        for kind, make in (('PIL writer', pil_file), ('all Paeth', paeth_file)):
            files = [make(mask(H, W, s)) for s in range(8)] * 8          # (eight distinct masks: the hand-written Paeth encoder is slow)
            packets = [P.parse(f)[0] for f in files]
            host = float(np.mean([pil_ms(f, 5) for f in files[:8]]))
            for n in (1, 64):
                (a, b), tok = kernel_ms(packets[:n])
                lines.append(f'| {label} {kind} | {n} | {a:.3f} | {b:.3f} | {(a + b) / n:.3f} | {tok:.0f} | {host:.3f} |')
    from cutie_amd.score_masks import score_folders
    with tempfile.TemporaryDirectory() as root:
        for d in ('gt', 'pred'):
            os.makedirs(os.path.join(root, d, 'v'))
        for t in range(300):
            for d, s in (('gt', t), ('pred', t + 1000)):
                with open(os.path.join(root, d, 'v', f'{t:05d}.png'), 'wb') as f:
                    f.write(pil_file(mask(480, 854, s)))
        walls = {'host': [], 'device': []}
        for _ in range(3):
            for mode in ('host', 'device'):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                score_folders(os.path.join(root, 'pred'), os.path.join(root, 'gt'), output=os.path.join(root, 'out_' + mode), decode=mode)
                walls[mode].append(time.perf_counter() - t0)
    lines += ['', 'score_masks over 300 frames of 854x480, wall clock in seconds, three interleaved rounds:', '']
    lines += [f'- decode={m}: ' + ', '.join(f'{w:.3f}' for w in ws) for m, ws in walls.items()]
    lines += ['', f'eval_vos.run_dataset over 4 clips of {args.frames} frames of 854x480 (device egress), wall-clock frames/s of the second pass, '
              'three interleaved rounds:', '', '| run | frames/s, rounds 1 / 2 / 3 |', '|---|---|'] + run_rows(args.frames, False)
    for k, f in enumerate(args.parent):
        lines += [r.replace('parent commit,', f'parent commit (run {k + 1}),') for r in open(f).read().rstrip('\n').split('\n')]
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
