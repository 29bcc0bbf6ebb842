"""Inputs of the guided-filter tests, shared by the CPU tests (model against the textbook filter) and the GPU tests (kernels against the
model): a guide uint8 [H, W, 3] and planes uint8 [S, H, W] per named content."""
import numpy as np

CONTENTS = ('noise', 'all255', 'zero', 'constant_plane', 'grey_guide', 'constant_channel', 'checkerboard', 'edge')


def blurred_step(H, W, at, width):
    """A plane that rises from 0 to 255 around column ``at`` over about ``width`` pixels (a resampled low-resolution edge)."""
    x = np.arange(W, dtype=np.float64)
    ramp = np.clip((x - at) / width + 0.5, 0.0, 1.0)
    return np.broadcast_to(np.rint(255.0 * ramp).astype(np.uint8), (H, W)).copy()


def make(kind, H, W, S, seed=0):
    """-> (guide, planes) of the named content.  'edge' is the use case: the guide steps at column W // 2, the planes are blurred steps
    displaced by a few pixels."""
    rng = np.random.default_rng([seed, H, W, S, CONTENTS.index(kind)])
    guide = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    planes = rng.integers(0, 256, (S, H, W), dtype=np.uint8)
    if kind == 'all255':                     # the largest sums
        guide[:], planes[:] = 255, 255
    elif kind == 'zero':
        guide[:], planes[:] = 0, 0
    elif kind == 'constant_plane':           # comes back exactly
        for s in range(S):
            planes[s] = (37 * s + 200) % 256
    elif kind == 'grey_guide':               # R = G = B: the covariance has rank 1
        guide[..., 1] = guide[..., 0]
        guide[..., 2] = guide[..., 0]
    elif kind == 'constant_channel':
        guide[..., 1] = 91
    elif kind == 'checkerboard':
        yy, xx = np.mgrid[0:H, 0:W]
        board = (((yy + xx) & 1) * 255).astype(np.uint8)
        guide[:] = board[..., None]
        planes[:] = 255 - board
        if S > 1:
            planes[1] = board
    elif kind == 'edge':
        guide[:, :W // 2] = (40, 60, 50)
        guide[:, W // 2:] = (210, 190, 220)
        guide[:] = np.clip(guide.astype(np.int64) + rng.integers(-3, 4, guide.shape), 0, 255).astype(np.uint8)
        for s in range(S):
            planes[s] = blurred_step(H, W, W // 2 + 3 - (s % 3), 9.0)
    return guide, planes


def edge_slopes(guide, plane, out):
    """Mean absolute rise across the guide's step (columns W // 2 - 1 -> W // 2) of the input plane and of the refined one."""
    W = plane.shape[1]
    c = W // 2
    rise = lambda z: float(np.abs(z[:, c].astype(np.float64) - z[:, c - 1].astype(np.float64)).mean())
    return rise(plane), rise(out)
