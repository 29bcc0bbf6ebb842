"""Inputs of the redaction tests, shared by the CPU tests (model against brute force) and the GPU tests (kernels against the model): a frame
uint8 [H, W, 3] and a weight plane uint8 [H, W] per named content; the case list of tests/test_gpu_redact.py."""
import numpy as np

WEIGHTS = ('zero', 'full', 'noise', 'blob')
# one pixel, a single row, a single column, and sizes that straddle the wave (64) and the blur tile widths in each direction; the last one
# is wider than a blur tile of every radius (256 - 2 r columns)
SIZES = [(1, 1), (1, 70), (70, 1), (2, 3), (7, 17), (63, 65), (64, 64), (65, 129), (131, 200), (33, 300)]
RADII = [1, 2, 7, 31, 64]
CELLS = [2, 3, 16, 17, 256]


def frame(H, W, seed=0):
    """noise over a gradient: neighbouring windows and cells differ, and so do the channels"""
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * xx + yy) % 256, (2 * yy + 5 * xx + 40) % 256, (xx * yy + 90) % 256], axis=-1)
    return ((base + rng.integers(0, 96, (H, W, 3))) % 256).astype(np.uint8)


def weight(kind, H, W, seed=0):
    rng = np.random.default_rng([seed, H, W, WEIGHTS.index(kind)])
    if kind == 'zero':
        return np.zeros((H, W), np.uint8)
    if kind == 'full':
        return np.full((H, W), 255, np.uint8)
    if kind == 'noise':
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]                                # a 0 | 255 ellipse off the centre, cut by the frame's edge
    return (255 * ((((yy - 0.4 * H) / max(0.35 * H, 1)) ** 2 + ((xx - 0.7 * W) / max(0.4 * W, 1)) ** 2) <= 1.0)).astype(np.uint8)


def make(kind, H, W, seed=0):
    return frame(H, W, seed), weight(kind, H, W, seed)
