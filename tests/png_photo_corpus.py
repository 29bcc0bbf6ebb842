"""name -> (first source uint8 [H, W] | [H, W, 3], last-channel plane uint8 [H, W] | None): the images both the model
(tests/png_photo_ref.py) and the device encoder (csrc/png_photo.hip) are checked on.  All small; built once per process."""
import functools
import os

import numpy as np

import png_photo_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
R = P.R
FIB_SEED = 20250611            # the shuffle of the Fibonacci plane
CL_SEED = None                 # a seeded plane whose code-length code passes 7 bits before limiting: none found (see cl_candidate)


def soft_alpha(H, W):
    """A smooth matte: 255 inside an ellipse, a soft edge, 0 outside."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.hypot((yy - H / 2) / (H / 3), (xx - W / 2) / (W / 3))
    return np.clip(255 * (1.6 - 1.2 * d), 0, 255).astype(np.uint8)


def bike_crop():
    from PIL import Image
    im = np.array(Image.open(os.path.join(HERE, 'golden', 'bike', '00000.jpg')).convert('RGB'))
    return np.ascontiguousarray(im[200:264, 300:396])          # 64 x 96


def fib_plane():
    """Counts in Fibonacci proportion over 19 values inside ONE block (32 rows) -- 1, 2, 3, 5 ..: the end-of-block symbol is the other
    1 --, shuffled so that nothing matches: the unlimited Huffman code would be 19 bits deep."""
    fib = [1, 2]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    # the value of rank k (0 = the most frequent): 0, -1, 1, -2, 2 .. as bytes -- small magnitudes, large differences: filter 0 wins every row
    vals = np.concatenate([np.full(c, (18 - k) // 2 if (18 - k) % 2 == 0 else 256 - (19 - k) // 2, np.uint8) for k, c in enumerate(fib)])
    rng = np.random.default_rng(FIB_SEED)
    rng.shuffle(vals)
    W = -(-len(vals) // 32)
    out = np.zeros(32 * W, np.uint8)
    out[1::2] = 255                                            # the padding alternates the two most frequent values: no run
    out[:len(vals)] = vals
    return out.reshape(32, W)


def cl_candidate(seed, H=64, W=256):
    """The planes searched for a code-length code deeper than 7 bits: value k of 40 takes a share ~ phi^-k, so the code lengths of the
    literal code spread over many values with Fibonacci-like counts of their own."""
    rng = np.random.default_rng(seed)
    p = 0.618 ** np.arange(40)
    return rng.choice(40, size=(H, W), p=p / p.sum()).astype(np.uint8)


def ramps():
    """One plane per filter that should win on it (the CPU test asserts that each of the five does win somewhere)."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:24, 0:70]
    out = {}
    out['ramp_none'] = ((yy + xx) & 1).astype(np.uint8)                                                 # left and above always differ
    out['ramp_sub'] = (((np.arange(24)[:, None] * 37) % 46 + 3 * xx) & 255).astype(np.uint8)                 # rows start anywhere, step 3 inside
    out['ramp_up'] = (((np.arange(70)[None, :] * 37) % 130 + 5 * yy) & 255).astype(np.uint8)                  # columns start anywhere, step 5 down
    avg = np.zeros((24, 70), np.int64)
    avg[0] = rng.integers(0, 256, 70)
    avg[:, 0] = rng.integers(0, 256, 24)
    for y in range(1, 24):
        for x in range(1, 70):
            avg[y, x] = (((avg[y, x - 1] + avg[y - 1, x]) >> 1) + (40 if (x + y) & 1 else -40)) & 255
    out['ramp_avg'] = avg.astype(np.uint8)
    out['ramp_paeth'] = ((3 * yy * yy + 2 * xx * xx + rng.integers(0, 2, (24, 70))) & 255).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(20250610)
    out = {}
    out['1x1'] = (np.array([[7]], np.uint8), None)
    out['1x2'] = (np.array([[7, 200]], np.uint8), None)
    out['2x1'] = (np.array([[7], [9]], np.uint8), None)
    out['1x1_rgba'] = (np.array([[[1, 2, 3]]], np.uint8), np.array([[4]], np.uint8))
    out['1xW'] = ((np.arange(300) // 50).astype(np.uint8).reshape(1, 300), None)                        # every match at distance 1
    out['Hx1'] = ((np.arange(70) % 3).astype(np.uint8).reshape(70, 1), None)
    for W in (62, 63, 64, 127, 128):                                                                    # L = 63, 64, 65, 128, 129
        out[f'L{W + 1}_b1'] = (rng.integers(0, 4, (5, W), dtype=np.uint8), None)
    for W in (15, 16, 31, 32):                                                                          # L = 61, 65, 125, 129 (L = 4 W + 1)
        out[f'L{4 * W + 1}_b4'] = (rng.integers(0, 3, (5, W, 3), dtype=np.uint8) * 80, rng.integers(0, 2, (5, W), dtype=np.uint8) * 255)
    yy, xx = np.mgrid[0:2 * R + 1, 0:45]
    smooth = ((np.sin(yy / 9.0) + np.cos(xx / 7.0)) * 60 + 128).astype(np.uint8)
    for H in (R - 1, R, R + 1, 2 * R + 1):
        out[f'H{H}'] = (smooth[:H].copy(), None)
    out['limit_b1'] = ((np.arange(16383) * 7 // 64).astype(np.uint8).reshape(1, 16383), None)           # L = 16384, one row
    out['limit_b4'] = (rng.integers(0, 256, (2, 4095, 3), dtype=np.uint8), np.full((2, 4095), 255, np.uint8))
    out['zeros'] = (np.zeros((40, 70), np.uint8), None)
    out['ones255'] = (np.full((40, 70), 255, np.uint8), None)
    out['ones255_rgba'] = (np.full((33, 20, 3), 255, np.uint8), np.full((33, 20), 255, np.uint8))
    out['noise'] = (rng.integers(0, 256, (33, 67), dtype=np.uint8), None)                               # no match at all
    out['noise_rgba'] = (rng.integers(0, 256, (33, 67, 3), dtype=np.uint8), rng.integers(0, 256, (33, 67), dtype=np.uint8))
    for k, v in ramps().items():
        out[k] = (v, None)
    for n in (257, 258, 259, 260, 261, 262, 263, 264, 265, 516, 517, 518, 519, 520, 521, 522):         # the take rule: runs around 258 and 516
        out[f'run{n}'] = (np.full((3, n), 5, np.uint8), None)
        m = np.full((2, n + 2), 9, np.uint8)
        m[:, 0], m[1, 0] = 4, 3
        out[f'run{n}_edge'] = (m, None)
    blk = rng.integers(0, 4, (9, 13), dtype=np.uint8)
    out['blocks'] = (np.kron(blk, np.ones((7, 23), np.uint8))[:, :290], None)                           # mask-like: matches up and left
    out['blocks_la'] = (np.kron(blk, np.ones((7, 23), np.uint8))[:, :290] * 60, np.kron(blk > 1, np.ones((7, 23), np.uint8))[:, :290].astype(np.uint8) * 255)
    out['fib'] = (fib_plane(), None)
    # every channel climbs at its own rate from a start of its own per row: the residuals repeat with the pixel, not with the byte -- distance B
    xs = np.arange(40)[None, :, None]
    ramp = (rng.integers(0, 60, (5, 1, 4)) + np.array([1, 2, 3, 4])[None, None, :] * xs).astype(np.uint8)
    out['period_rgba'] = (np.ascontiguousarray(ramp[:, :, :3]), np.ascontiguousarray(ramp[:, :, 3]))
    out['period_rgb'] = (np.ascontiguousarray(ramp[:, :, 1:]), None)
    out['period_la'] = (np.ascontiguousarray(ramp[:, :, 0]), np.ascontiguousarray(ramp[:, :, 2]))
    crop = bike_crop()
    alpha = soft_alpha(*crop.shape[:2])
    grey = (crop.astype(np.int64) @ np.array([77, 150, 29]) >> 8).astype(np.uint8)
    out['bike_l'] = (grey, None)
    out['bike_la'] = (grey, alpha)
    out['bike_rgb'] = (crop, None)
    out['bike_rgba'] = (crop, alpha)
    out['alpha'] = (soft_alpha(96, 128), None)
    return out


PHOTO = ('bike_l', 'bike_la', 'bike_rgb', 'bike_rgba')
SMOOTH = ('alpha', 'H65')


@functools.lru_cache(maxsize=None)
def encoded(name):
    """The model's result for a corpus item, computed once and shared."""
    s0, s1 = corpus()[name]
    return P.encode(s0, s1)
