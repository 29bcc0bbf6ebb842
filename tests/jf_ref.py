"""The model of the DAVIS J&F counts (PROB_TO_ID flags == 64, csrc/score.hip): numpy + scipy, written from the published code of
davis2017-evaluation (utils.py seg2bmap at equal size, metrics.py db_eval_boundary: the boundary maps dilated by disk(bound_pix) with
nothing outside the image).  TEST INFRASTRUCTURE ONLY.  The package itself (and cv2 / skimage, which it needs) is not available to these
tests: the agreement with it is by construction from its source, not by running it."""
import numpy as np
from scipy import ndimage


def seg2bmap(seg):
    """Binary mask -> boundary map: b = (s ^ e) | (s ^ so) | (s ^ se) with the east, south and south-east neighbours; the last row uses
    s ^ e only, the last column s ^ so only, the bottom-right pixel is 0."""
    seg = np.asarray(seg).astype(bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def dilate(b, r):
    return ndimage.binary_dilation(b, structure=disk(r))


def matched(a, b, r):
    """a, b bool [N, H, W] -> int [N]: per plane the pixels of a within r of a pixel of b, |a & dilate(b, r)|.  ONE call of scipy's
    dilation over the stack with the structure disk(r)[None] (setting up a large structure costs more than applying it), computed at
    the pixels of ``mask`` only -- elsewhere scipy's output is its input -- which gives the same sums at a fraction of the cost."""
    if not a.any() or not b.any():
        return np.zeros(len(a), dtype=np.int64)
    return (a & ndimage.binary_dilation(b, structure=disk(r)[None], mask=a)).sum(axis=(1, 2))


def counts_batch(pairs, objects, r):
    """pairs = [(pred, gt), ...] of one shape -> int64 [len(pairs), n, 8]: per pair and id of ``objects`` |p & g|, |p | g|, boundary pixels
    of p, of g, p boundary within r of g boundary, g boundary within r of p boundary, |p|, |g| for p = (pred == id), g = (gt == id)."""
    n = len(objects)
    out = np.zeros((len(pairs), n, 8), dtype=np.int64)
    bp, bg = [], []
    for q, (pred, gt) in enumerate(pairs):
        for k, oid in enumerate(objects):
            p, g = np.asarray(pred) == oid, np.asarray(gt) == oid
            bp.append(seg2bmap(p))
            bg.append(seg2bmap(g))
            out[q, k, [0, 1, 2, 3, 6, 7]] = [(p & g).sum(), (p | g).sum(), bp[-1].sum(), bg[-1].sum(), p.sum(), g.sum()]
    bp, bg = np.stack(bp), np.stack(bg)
    m = matched(np.concatenate([bp, bg]), np.concatenate([bg, bp]), r)
    out[:, :, 4] = m[:len(bp)].reshape(len(pairs), n)
    out[:, :, 5] = m[len(bp):].reshape(len(pairs), n)
    return out


def counts(pred, gt, objects, r):
    """One pair -> int64 [n, 8] (see counts_batch)."""
    return counts_batch([(pred, gt)], objects, r)[0]


class ScoreExecutor:
    """Wraps another executor (tests/mock_exec.py MockExecutor on host memory) and runs PROB_TO_ID flags == 64 through the model."""
    is_mock = True

    def __init__(self, inner):
        self.inner = inner
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def stream(self):
        return 0

    def run(self, arr):
        from mock_exec import view, U8, I32
        for rec in arr:
            if int(rec['kind']) == 36 and int(rec['flags']) == 64:
                i, p = [int(v) for v in rec['i']], [int(v) for v in rec['p']]
                H, W, r, n = i[1], i[2], i[5], i[9]
                pred, gt = view(p[2], U8, (H, W)).numpy(), view(p[3], U8, (H, W)).numpy()
                objs = view(p[6], I32, (n,)).tolist()
                import torch
                view(p[7], I32, (n, 8)).copy_(torch.from_numpy(counts(pred, gt, objs, r).astype(np.int32)))
                self.calls += 1
            else:
                self.inner.run_one(rec)
