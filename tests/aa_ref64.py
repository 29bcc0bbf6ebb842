"""Float64 reference of torch's antialiased bilinear resize (F.interpolate(mode='bilinear', align_corners=False, antialias=True)),
with a per-element error bound for an fp32 evaluation.  TEST INFRASTRUCTURE ONLY (style of tests/ref64.py).

The filter is torch's: the separable triangle of _upsample_bilinear2d_aa with the tap ranges and the fp32 weights rounded as torch's CPU
kernel rounds them (written out here independently of cutie_amd/ops.py aa_taps, which the tests compare against it).  The two passes
(horizontal, then vertical) are evaluated exactly in float64 on the fp32 input values.

Bound: an fp32 pass over n taps with normalised weights w >= 0 is a dot product, |fl(sum w x) - sum w x| <= gamma_n sum w |x|
(gamma_n = n u / (1 - n u), u = 2^-24; with or without fused multiply-adds).  The horizontal pass gives e1 = gamma_nx sum w |x|
(+ u |T| for storing the intermediate); the vertical pass over the inexact intermediate adds sum v e1 + gamma_ny sum v (|T| + e1).
For inputs in [0, 1] this stays below 2^-19."""
import numpy as np

U = 2.0 ** -24
CEILING = 2.0 ** -19


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1 - n * U)


def taps(n_in, n_out):
    """-> (first [n_out], count [n_out], fp32 weights [n_out, K]) of one axis, as torch computes them for float input."""
    f32, f64 = np.float32, np.float64
    if n_in == n_out:                                   # torch skips an axis whose size does not change
        return np.arange(n_out), np.ones(n_out, dtype=np.int64), np.ones((n_out, 1), dtype=f32)
    scale = f32(f32(n_in) / f32(n_out))
    support = scale if scale >= 1.0 else f32(1.0)
    inv = f32(f64(1.0) / f64(scale)) if scale >= 1.0 else f32(1.0)
    kmax = int(np.ceil(f64(support))) * 2 + 1
    firsts, counts = np.zeros(n_out, dtype=np.int64), np.zeros(n_out, dtype=np.int64)
    W = np.zeros((n_out, kmax), dtype=f32)
    for i in range(n_out):
        center = f32(f64(scale) * (i + 0.5))
        lo = max(int(f64(f32(center - support)) + 0.5), 0)
        n = min(int(f64(f32(center + support)) + 0.5), n_in) - lo
        n = min(max(n, 0), kmax)
        tot = f32(0.0)
        for j in range(n):
            a = f32((f64(f32(f32(j + lo) - center)) + 0.5) * f64(inv))
            a = abs(a)
            w = f32(f32(1.0) - a) if a < 1.0 else f32(0.0)
            W[i, j] = w
            tot = f32(tot + w)
        if tot != 0:
            W[i, :n] = (W[i, :n] / tot).astype(f32)
        firsts[i], counts[i] = lo, n
    return firsts, counts, W


def matrix(n_in, n_out):
    """Dense float64 [n_out, n_in] of the fp32 weights, and the tap counts."""
    first, count, w = taps(n_in, n_out)
    A = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        A[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
    return A, count


def resize_aa64(x, OH, OW):
    """x: float [C, H, W] (numpy / CPU tensor, the fp32 values) -> (float64 [C, OH, OW], bound [C, OH, OW])."""
    x = np.asarray(x, dtype=np.float64)
    C, H, W = x.shape
    Ax, nx = matrix(W, OW)
    Ay, ny = matrix(H, OH)
    T = x @ Ax.T                                        # [C, H, OW]
    e1 = gamma(nx)[None, None, :] * (np.abs(x) @ Ax.T) + U * np.abs(T)
    out = np.einsum('yh,chw->cyw', Ay, T)
    bound = np.einsum('yh,chw->cyw', Ay, e1) + gamma(ny)[None, :, None] * np.einsum('yh,chw->cyw', Ay, np.abs(T) + e1)
    return out, bound
