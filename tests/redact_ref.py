"""The model of PROB_TO_ID flags == 65536 (include/cutie_hip.h; csrc/redact.hip), the frame with an effect blended over it under a weight
plane, in numpy: the oracle of the CPU and GPU tests.  Integers only; f is the frame's byte, every channel on its own, "//" the floor
division of non-negative integers.

BLUR      exactly three passes.  One pass maps a uint8 image a to a': with w(y, x) = the rows max(0, y - r) .. min(H - 1, y + r) and the
          columns max(0, x - r) .. min(W - 1, x + r) (nothing exists outside the frame), N its pixel count and S the sum of a over it,
          a'(y, x) = (2 S + N) // (2 N) -- one 2-D window mean rounded once.  e = the third pass's output.  1 <= r <= 64.
PIXELATE  cell (Y, X) holds the rows Y c .. min(H, (Y + 1) c) - 1 and the columns X c .. min(W, (X + 1) c) - 1; with n its pixel count
          and S its sum, e = (2 S + n) // (2 n) for every pixel of the cell.  2 <= c <= 256.
FILL      e = the colour's byte.
BLEND     w' = w, or 255 - w with the invert bit; out = (w' e + (255 - w') f + 127) // 255.

``brute_*`` restate the same with plain loops over windows and cells and Python integers; tests/test_redact_cpu.py pins the vectorised
model to them."""
import numpy as np

MAX_RADIUS, MAX_CELL = 64, 256
MODES = {'blur': 0, 'pixelate': 1, 'fill': 2}


def box_pass(a, r):
    """One pass: uint8 [H, W, C] -> uint8 [H, W, C], through an integral image in int64."""
    H, W = a.shape[:2]
    I = np.zeros((H + 1, W + 1) + a.shape[2:], dtype=np.int64)
    I[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
    x0, x1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
    S = I[y1][:, x1] - I[y0][:, x1] - I[y1][:, x0] + I[y0][:, x0]
    N = ((y1 - y0)[:, None] * (x1 - x0)[None, :]).reshape((H, W) + (1,) * (a.ndim - 2))
    return ((2 * S + N) // (2 * N)).astype(np.uint8)


def blur(frame, r):
    assert 1 <= r <= MAX_RADIUS
    return box_pass(box_pass(box_pass(frame, r), r), r)


def pixelate(frame, c):
    assert 2 <= c <= MAX_CELL
    H, W = frame.shape[:2]
    S = np.add.reduceat(np.add.reduceat(frame.astype(np.int64), np.arange(0, H, c), axis=0), np.arange(0, W, c), axis=1)
    ny = np.minimum(np.arange(0, H, c) + c, H) - np.arange(0, H, c)
    nx = np.minimum(np.arange(0, W, c) + c, W) - np.arange(0, W, c)
    n = (ny[:, None] * nx[None, :])[..., None]
    cells = ((2 * S + n) // (2 * n)).astype(np.uint8)
    return cells[np.arange(H) // c][:, np.arange(W) // c]


def effect(frame, mode, strength=0, color=(0, 0, 0)):
    """-> e uint8 [H, W, 3]"""
    code = MODES.get(mode, mode)
    if code == 0:
        return blur(frame, int(strength))
    if code == 1:
        return pixelate(frame, int(strength))
    assert code == 2
    return np.broadcast_to(np.array(color, dtype=np.uint8), frame.shape).copy()


def blend(frame, e, w, invert=False):
    w = w.astype(np.int64)
    if invert:
        w = 255 - w
    w = w[..., None]
    return ((w * e.astype(np.int64) + (255 - w) * frame.astype(np.int64) + 127) // 255).astype(np.uint8)


def model(frame, weight, mode, strength=0, color=(0, 0, 0), invert=False):
    """frame uint8 [H, W, 3], weight uint8 [H, W] -> out uint8 [H, W, 3]"""
    frame, weight = np.asarray(frame), np.asarray(weight)
    assert frame.dtype == np.uint8 and weight.dtype == np.uint8 and frame.shape == weight.shape + (3,)
    return blend(frame, effect(frame, mode, strength, color), weight, invert)


# ---- the same with loops and Python integers ------------------------------------------------------------------------------------------
def brute_box_pass(a, r):
    H, W, C = a.shape
    out = np.zeros_like(a)
    for y in range(H):
        for x in range(W):
            rows = range(max(0, y - r), min(H - 1, y + r) + 1)
            cols = range(max(0, x - r), min(W - 1, x + r) + 1)
            N = len(rows) * len(cols)
            for ch in range(C):
                S = 0
                for yy in rows:
                    for xx in cols:
                        S += int(a[yy, xx, ch])
                out[y, x, ch] = (2 * S + N) // (2 * N)
    return out


def brute_pixelate(a, c):
    H, W, C = a.shape
    out = np.zeros_like(a)
    for Y in range((H + c - 1) // c):
        for X in range((W + c - 1) // c):
            rows = range(Y * c, min(H, (Y + 1) * c))
            cols = range(X * c, min(W, (X + 1) * c))
            n = len(rows) * len(cols)
            for ch in range(C):
                S = 0
                for yy in rows:
                    for xx in cols:
                        S += int(a[yy, xx, ch])
                for yy in rows:
                    for xx in cols:
                        out[yy, xx, ch] = (2 * S + n) // (2 * n)
    return out


def brute_model(frame, weight, mode, strength=0, color=(0, 0, 0), invert=False):
    code = MODES.get(mode, mode)
    H, W, _ = frame.shape
    if code == 0:
        e = frame
        for _ in range(3):
            e = brute_box_pass(e, strength)
    elif code == 1:
        e = brute_pixelate(frame, strength)
    else:
        e = None
    out = np.zeros_like(frame)
    for y in range(H):
        for x in range(W):
            w = int(weight[y, x])
            if invert:
                w = 255 - w
            for ch in range(3):
                ee = int(color[ch]) if e is None else int(e[y, x, ch])
                out[y, x, ch] = (w * ee + (255 - w) * int(frame[y, x, ch]) + 127) // 255
    return out
