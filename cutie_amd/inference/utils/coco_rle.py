"""COCO compressed RLE of a binary mask, numpy only -- the format of pycocotools' ``rleEncode`` / ``rleToString`` / ``rleFrString`` (the
BURST json carries its first-frame masks and its predictions as such strings; cutie/inference/data/burst_video_reader.py:78 and
cutie/inference/utils/results_utils.py:169-170 of the reference call pycocotools for them).  Also the model the device encoder
(csrc/rle.hip, PROB_TO_ID flags == 32) matches byte for byte.

Counts: the mask flattened COLUMN-major (index p = x * H + y) as run lengths, starting with a run of zeros (``counts[0] == 0`` when
pixel 0 is set); the last run is always there; an all-zero mask is the single count H * W.
String: count i > 2 is coded as the signed difference ``counts[i] - counts[i - 2]``; every value as 5-bit groups, least significant
first, bit 0x20 of a character = another group follows, the last group's bit 0x10 = the sign; characters are ``chr(group + 48)``."""
from typing import List, Sequence

import numpy as np


def counts_of(mask) -> List[int]:
    """Run lengths of ``mask`` ([H, W], anything non-zero is set) in column-major order, zeros first."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f'coco_rle: a mask is [H, W], not {m.shape}')
    flat = (m != 0).ravel(order='F')
    n = flat.size
    if n == 0:
        return [0]
    bounds = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [n]))
    counts = np.diff(bounds)
    if flat[0]:
        counts = np.concatenate(([0], counts))
    return [int(c) for c in counts]


def to_string(counts: Sequence[int]) -> str:
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    x = c.copy()
    x[3:] -= c[1:-2]                                          # i > 2: the difference to the count two places back
    out = np.zeros((x.size, 13), dtype=np.uint8)              # 13 groups of 5 bits hold any int64
    live = np.ones(x.size, dtype=bool)
    used = np.zeros((x.size, 13), dtype=bool)
    for r in range(13):
        if not live.any():
            break
        g = x & 0x1f
        x = x >> 5                                            # arithmetic
        more = np.where((g & 0x10) != 0, x != -1, x != 0)
        out[:, r] = np.where(live, g | (more.astype(np.int64) << 5), 0) + 48
        used[:, r] = live
        live = live & more
    return out[used].tobytes().decode('ascii')                # row-major selection: count by count, group by group


def from_string(s: str) -> List[int]:
    v = np.frombuffer(s.encode('ascii'), dtype=np.uint8).astype(np.int64) - 48
    if v.size == 0:
        return []
    if ((v < 0) | (v > 63)).any() or (v[-1] & 0x20):
        raise ValueError('coco_rle: not a compressed RLE string')
    last = (v & 0x20) == 0                                    # the last group of every value
    first = np.concatenate(([True], last[:-1]))
    start = np.flatnonzero(first)
    k = np.arange(v.size) - np.repeat(start, np.diff(np.concatenate((start, [v.size]))))       # group index inside its value
    if (k > 11).any():
        raise ValueError('coco_rle: a value of more than 12 groups')
    x = np.add.reduceat((v & 0x1f) << (5 * k), start)
    nk = k[last] + 1
    x = np.where((v[last] & 0x10) != 0, x | (np.int64(-1) << (5 * nk)), x)
    c = x.copy()                                              # undo the differences: one chain over the odd places, one over the even
    c[1::2] = np.cumsum(x[1::2])                              # from place 2 on (place 0 stands alone)
    c[2::2] = np.cumsum(x[2::2])
    return [int(t) for t in c]


def encode(mask) -> str:
    return to_string(counts_of(mask))


def decode(counts: str, h: int, w: int) -> np.ndarray:
    """-> uint8 [h, w] of 0 / 1."""
    if isinstance(counts, bytes):
        counts = counts.decode('ascii')
    c = np.asarray(from_string(counts) if isinstance(counts, str) else counts, dtype=np.int64)
    if (c < 0).any() or int(c.sum()) != h * w:
        raise ValueError(f'coco_rle: the counts cover {int(c.sum())} pixels, the mask has {h} x {w}')
    vals = (np.arange(c.size) & 1).astype(np.uint8)
    return np.repeat(vals, c).reshape((h, w), order='F')
