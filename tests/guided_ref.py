"""The colour guided filter of PROB_TO_ID flags == 32768 (include/cutie_hip.h; csrc/guided.hip) in numpy, operation by operation: ``model``
gives the bytes the kernels must give.  ``textbook`` is the filter as He, Sun and Tang state it -- float64 on [0, 1] images, box means,
``np.linalg.solve`` per pixel, no fixed point --, written independently: what the contract is measured against."""
import numpy as np

MAX_RADIUS, MAX_PLANES = 64, 16
EPS_MIN, EPS_MAX = 1e-6, 1.0


def _edges(n, r):
    k = np.arange(n)
    return np.maximum(k - r, 0), np.minimum(k + r, n - 1) + 1


def window_sums(x, r):
    """x [..., H, W] (int64 or float64) -> the sums over the rows max(0, y - r) .. min(H - 1, y + r) and the columns likewise, by an
    integral image: exact for integers."""
    H, W = x.shape[-2:]
    c = np.zeros(x.shape[:-2] + (H + 1, W + 1), dtype=x.dtype)
    c[..., 1:, 1:] = x.cumsum(-2).cumsum(-1)
    y0, y1 = _edges(H, r)
    x0, x1 = _edges(W, r)
    y0, y1 = y0[:, None], y1[:, None]
    return c[..., y1, x1] - c[..., y0, x1] - c[..., y1, x0] + c[..., y0, x0]


def window_count(H, W, r):
    y0, y1 = _edges(H, r)
    x0, x1 = _edges(W, r)
    return ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(np.int64)


def _sat_rint(x):
    assert np.isfinite(x).all()
    return np.clip(np.rint(x), -2147483648.0, 2147483647.0).astype(np.int64)


def coefficients(guide, planes, r, eps):
    """Stages 1 and 2 -> (A int64 [S, 3, H, W], B int64 [S, H, W]), the fixed-point coefficients of every window."""
    guide, planes = np.asarray(guide), np.asarray(planes)
    assert guide.dtype == np.uint8 and guide.ndim == 3 and guide.shape[2] == 3 and planes.dtype == np.uint8 and planes.ndim == 3
    H, W = guide.shape[:2]
    assert planes.shape[1:] == (H, W) and 1 <= planes.shape[0] <= MAX_PLANES and 1 <= r <= MAX_RADIUS
    eps = np.float64(np.float32(eps))                                  # the descriptor carries eps as a float
    assert np.float32(EPS_MIN) <= np.float32(eps) <= np.float32(EPS_MAX)
    I = guide.astype(np.int64).transpose(2, 0, 1)                       # [3, H, W]
    N = window_count(H, W, r)
    S = window_sums(I, r)                                               # S_c
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    C = {cd: N * window_sums(I[cd[0]] * I[cd[1]], r) - S[cd[0]] * S[cd[1]] for cd in pairs}
    Nd = N.astype(np.float64)
    e = ((eps * 65025.0) * Nd) * Nd
    m00, m01, m02 = C[0, 0].astype(np.float64) + e, C[0, 1].astype(np.float64), C[0, 2].astype(np.float64)
    m11, m12, m22 = C[1, 1].astype(np.float64) + e, C[1, 2].astype(np.float64), C[2, 2].astype(np.float64) + e
    a00 = m11 * m22 - m12 * m12
    a01 = m02 * m12 - m01 * m22
    a02 = m01 * m12 - m02 * m11
    a11 = m00 * m22 - m02 * m02
    a12 = m01 * m02 - m00 * m12
    a22 = m00 * m11 - m01 * m01
    det = (m00 * a00 + m01 * a01) + m02 * a02
    Sd = S.astype(np.float64)
    A = np.empty((planes.shape[0], 3, H, W), dtype=np.int64)
    B = np.empty((planes.shape[0], H, W), dtype=np.int64)
    for s, plane in enumerate(planes.astype(np.int64)):
        T = window_sums(plane, r)
        g = [(N * window_sums(I[c] * plane, r) - S[c] * T).astype(np.float64) for c in range(3)]
        c0 = ((a00 * g[0] + a01 * g[1]) + a02 * g[2]) / det
        c1 = ((a01 * g[0] + a11 * g[1]) + a12 * g[2]) / det
        c2 = ((a02 * g[0] + a12 * g[1]) + a22 * g[2]) / det
        b = (T.astype(np.float64) - ((c0 * Sd[0] + c1 * Sd[1]) + c2 * Sd[2])) / Nd
        A[s, 0], A[s, 1], A[s, 2] = _sat_rint(c0 * 1048576.0), _sat_rint(c1 * 1048576.0), _sat_rint(c2 * 1048576.0)
        B[s] = _sat_rint(b * 4096.0)
    return A, B


def model(guide, planes, r, eps, full=False):
    """guide uint8 [H, W, 3], planes uint8 [S, H, W] -> the refined planes uint8 [S, H, W]; ``full``: (bytes, q float64 before rounding)."""
    guide, planes = np.asarray(guide), np.asarray(planes)
    A, B = coefficients(guide, planes, r, eps)
    H, W = guide.shape[:2]
    Nd = window_count(H, W, r).astype(np.float64)
    I = guide.astype(np.float64).transpose(2, 0, 1)
    sA, sB = window_sums(A, r).astype(np.float64), window_sums(B, r).astype(np.float64)
    q = (((sA[:, 0] * I[0] + sA[:, 1] * I[1]) + sA[:, 2] * I[2]) * (1.0 / 1048576.0) + sB * (1.0 / 4096.0)) / Nd
    out = np.minimum(np.maximum(np.rint(q), 0.0), 255.0).astype(np.uint8)
    return (out, q) if full else out


def textbook(guide, plane, r, eps):
    """The colour guided filter of the paper (its equations 19 - 21): guide float64 [H, W, 3] and plane float64 [H, W] on [0, 1] -> q
    float64 [H, W], unclipped.  Windows are clipped at the frame, as the paper's box filter normalised by the pixel count."""
    I = np.asarray(guide, dtype=np.float64)
    p = np.asarray(plane, dtype=np.float64)
    H, W = p.shape
    n = window_count(H, W, r).astype(np.float64)
    mean = lambda x: window_sums(np.ascontiguousarray(x), r) / n
    mI = np.stack([mean(I[..., c]) for c in range(3)], -1)              # [H, W, 3]
    mp = mean(p)
    cov_Ip = np.stack([mean(I[..., c] * p) for c in range(3)], -1) - mI * mp[..., None]
    sigma = np.empty((H, W, 3, 3))
    for c in range(3):
        for d in range(3):
            sigma[..., c, d] = mean(I[..., c] * I[..., d]) - mI[..., c] * mI[..., d]
    a = np.linalg.solve(sigma + eps * np.eye(3), cov_Ip[..., None])[..., 0]
    b = mp - (a * mI).sum(-1)
    ma = np.stack([mean(a[..., c]) for c in range(3)], -1)
    return (ma * I).sum(-1) + mean(b)
