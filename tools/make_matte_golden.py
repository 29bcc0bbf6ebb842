"""Writes tests/golden/matte/*.npz: inputs and the bytes that the UNMODIFIED reference's gui/interactive_utils.py writes for them (its
torch functions, run on the CPU) -- what tests/matte_ref.py, and through it csrc/matte.hip, must reproduce exactly.

    python tools/make_matte_golden.py --reference PATH_TO_REFERENCE_CHECKOUT

Needs the reference checkout (imported, never copied) and runs on the build machine only; the tests read the files.
Per file: frame uint8 [H, W, 3]; planes float16 [P, H, W] (the tests and this tool widen them to float32, exactly); layer uint8
[H, W, 4]; table uint8 [256, 4] (the reference's colour map); and one array per case -- `davis`, `light`, `fade` (the hard modes on the
argmax of the planes) and `popup|layer|rgba` + `_` + the target list joined by `_` (`none` for the empty list)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'matte')
SIZES = [(1, 1), (3, 5), (33, 47), (97, 131)]


def planes_of(P, H, W, rs):
    logits = rs.randn(P, H, W).astype(np.float32) * 2
    if H > 8:                                      # object-like: low-frequency blobs under the noise
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        for q in range(P):
            logits[q] += 4 * np.sin(yy / H * (q + 2)) * np.cos(xx / W * (q + 3))
    e = np.exp(logits - logits.max(0))
    return (e / e.sum(0)).astype(np.float16)


def smooth_inputs(P, H, W, rs):
    """A frame and a layer of flat tiles, planes in steps of 1/32 from low-frequency logits: tens of KB once deflated."""
    yy, xx = np.mgrid[0:H, 0:W]
    ty, tx = yy // 12, xx // 12                     # flat tiles of 12 x 12, a few colours: what deflate handles
    frame = rs.randint(0, 256, (ty.max() + 1, tx.max() + 1, 3)).astype(np.uint8)[ty, tx]
    frame[:, :, 1] = (frame[:, :, 1].astype(np.int32) + yy // 4) % 256          # ... with a slow vertical ramp in one channel
    layer = rs.randint(0, 256, (ty.max() + 1, tx.max() + 1, 4)).astype(np.uint8)[ty, tx]
    layer[(ty + tx) % 3 == 0, 3] = 255
    layer[(ty + tx) % 3 == 1, 3] = 0
    logits = np.stack([3 * np.sin(yy / H * (q + 2) + q) * np.cos(xx / W * (q + 3)) for q in range(P)]).astype(np.float32)
    e = np.exp(logits - logits.max(0))
    return frame, layer, (np.round(e / e.sum(0) * 32) / 32).astype(np.float16)


def target_lists(P):
    return [[], [1], [1, 3], list(range(1, P))] if P > 3 else [[], [1], list(range(1, P))]


def key(mode, targets):
    return mode + '_' + ('_'.join(str(t) for t in targets) if targets else 'none')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='a checkout of the reference (hkchengrex/Cutie)')
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    torch.cuda.is_available = lambda: False        # the module picks its device on import: the CPU
    from gui import interactive_utils as IU
    assert IU.device.type == 'cpu'
    os.makedirs(OUT, exist_ok=True)
    table = np.zeros((256, 4), np.uint8)
    table[:, :3] = IU.color_map_np

    def run(frame, planes16, layer, cases, hard_modes):
        img = lambda: IU.image_to_torch(frame, 'cpu')          # (the hard modes change the image in place: a fresh one per call)
        prob = torch.from_numpy(planes16.astype(np.float32))
        lay = torch.from_numpy(layer).float() / 255
        out = {}
        for mode in hard_modes:
            out[mode] = IU.get_visualization_torch(mode, img(), prob, lay, [])
        for mode, targets in cases:
            out[key(mode, targets)] = IU.get_visualization_torch(mode, img(), prob, lay, list(targets))
        return out

    for H, W in SIZES:
        for P in (2, 4):
            rs = np.random.RandomState(1000 * H + 10 * W + P)
            frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
            layer = rs.randint(0, 256, (H, W, 4)).astype(np.uint8)
            layer[rs.rand(H, W) < 0.2, 3] = 255
            layer[rs.rand(H, W) < 0.2, 3] = 0
            planes = planes_of(P, H, W, rs)
            lists = target_lists(P)
            if (H, W) == (97, 131):                # the large size: inputs that compress (the smaller sizes carry the noise) and two or three cases
                frame, layer, planes = smooth_inputs(P, H, W, rs)
                cases = [('popup', lists[-1]), ('layer', lists[2])] if P == 4 else [('rgba', lists[1])]
                hard = ('davis',) if P == 4 else ('light', 'fade')
            else:
                cases = [(m, t) for m in ('popup', 'layer', 'rgba') for t in lists]
                hard = ('davis', 'light', 'fade')
            np.savez_compressed(os.path.join(OUT, f'm_{H}x{W}_p{P}.npz'), frame=frame, planes=planes, layer=layer, table=table,
                                **run(frame, planes, layer, cases, hard))
    # the clamps: hand-built planes whose target sum passes 1 (and stays below, and is exactly 0 and 1) -- layer and rgba clip; popup
    # does not and its bytes are undefined above 1, so it is left out
    H, W, P = 9, 14, 4
    rs = np.random.RandomState(77)
    frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    layer = rs.randint(0, 256, (H, W, 4)).astype(np.uint8)
    planes = np.zeros((P, H, W), np.float16)
    planes[1] = rs.choice(np.array([0, 0.25, 0.5, 0.75, 0.8125, 1.0], np.float16), (H, W))
    planes[2] = rs.choice(np.array([0, 0.125, 0.5, 0.9375, 1.0], np.float16), (H, W))
    planes[3] = rs.rand(H, W).astype(np.float16)
    planes[0] = np.maximum(0, 1 - planes[1:].astype(np.float32).sum(0)).astype(np.float16)
    assert (planes[1:].astype(np.float32).sum(0) > 1).any()
    cases = [(m, t) for m in ('layer', 'rgba') for t in ([1, 2], [1, 2, 3], [3, 1])]
    np.savez_compressed(os.path.join(OUT, 'm_clamp_9x14_p4.npz'), frame=frame, planes=planes, layer=layer, table=table,
                        **run(frame, planes, layer, cases, ()))
    for n in sorted(os.listdir(OUT)):
        print(n, os.path.getsize(os.path.join(OUT, n)))


if __name__ == '__main__':
    main()
