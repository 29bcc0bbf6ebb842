"""The numpy model of the track statistics (PROB_TO_ID flags == 1024, include/cutie_hip.h; kernels: cutie_amd/csrc/tracks.hip): a plain
function of (id plane, object list, prob, lut) -> int32 [n, 12].  Per object: 0 area | 1 xmin 2 ymin 3 xmax 4 ymax | 5,6 sum of x | 7,8 sum
of y | 9 confidence samples | 10,11 confidence sum; the pairs are 64-bit values, low word first.  Written object by object with np.where,
sums in Python integers -- nothing of the kernels' decomposition (chunks, waves, blocks, carries) appears here."""
import numpy as np

WORDS = 12
f32 = np.float32


def q16(v):
    """float32 array -> int64 array: 0 if !(v > 0) (a NaN too), 65535 if v >= 1, else (int)(v * 65535.f + 0.5f), each operation rounded
    to float32 on its own."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(invalid='ignore', over='ignore'):
        mid = (v * f32(65535.0) + f32(0.5)).astype(f32)
        mid = np.where((v > 0) & (v < 1), mid, f32(0)).astype(np.int64)          # truncation of a value in [0.5, 65535.5)
    return np.where(v >= 1, 65535, np.where(v > 0, mid, 0)).astype(np.int64)


def winners(prob):
    """[P, h, w] -> (arg [h, w], best [h, w]): the first plane with the largest value by PROB_TO_ID's rule -- plane 0, then every plane whose
    value is > the best so far (a NaN is never larger, and nothing is larger than a NaN in plane 0)."""
    prob = np.asarray(prob, dtype=f32)
    best = prob[0].copy()
    arg = np.zeros(best.shape, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for q in range(1, prob.shape[0]):
            m = prob[q] > best
            best = np.where(m, prob[q], best)
            arg = np.where(m, q, arg)
    return arg, best


def _isum(a):
    """the exact sum as a Python integer (fewer than 2^31 terms below 2^31 each: an int64 sum cannot wrap)"""
    return int(np.sum(a, dtype=np.int64))


def _pair(v):
    return [v & 0xffffffff, (v >> 32) & 0xffffffff]


def table(ids, objs, prob=None, lut=None):
    """ids uint8 [H, W]; objs: n ints; prob f32 [P, h, w] (any view) with lut: P ints, or None -> int32 [n, 12]."""
    ids = np.asarray(ids)
    assert ids.dtype == np.uint8 and ids.ndim == 2
    H, W = ids.shape
    objs = [int(v) for v in objs]
    if prob is not None:
        arg, best = winners(prob)
        lut = [int(v) for v in lut]
        assert len(lut) == np.asarray(prob).shape[0]
    rows, first = [], {}
    for k, oid in enumerate(objs):
        if not 1 <= oid <= 255:                                    # an absent object
            rows.append([0, W, H, -1, -1] + [0] * 7)
            continue
        if oid in first:                                           # an entry equal to an earlier one: its row again
            rows.append(list(rows[first[oid]]))
            continue
        first[oid] = k
        ys, xs = np.where(ids == oid)
        area = int(len(xs))
        if area:
            row = [area, int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] + _pair(_isum(xs)) + _pair(_isum(ys))
        else:
            row = [0, W, H, -1, -1, 0, 0, 0, 0]
        count, total = 0, 0
        if prob is not None:
            for q, v in enumerate(lut):
                if v == oid:
                    won = arg == q
                    count += int(won.sum())
                    total += _isum(q16(best[won]))
        rows.append(row + [count] + _pair(total))
    out = np.array(rows, dtype=np.int64).reshape(len(objs), WORDS)
    return (out & 0xffffffff).astype(np.uint32).view(np.int32)
