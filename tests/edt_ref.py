"""The numpy model of PROB_TO_ID flags == 4096 (include/cutie_hip.h, csrc/edt.hip): the exact squared Euclidean distance of every pixel of
an id plane to the nearest pixel of the other class, per set of ids, capped at ``limit``, and the band byte that is a compare of it.

Written from the definition, not from the kernel's column and row passes: for a pixel p of class c, d2(p) is the minimum of dx^2 + dy^2
over the pixels of the other class inside the frame.  Two exhaustive searches of exactly that minimum, chosen by cost alone:
  * offsets: every offset (dy, dx) in the order of dy^2 + dx^2; a pixel is settled by the first offset at which a pixel of the other class
    lies (pixels next to an edge settle after a few offsets);
  * pairs: what is still open after NEAR offsets is compared with every candidate pixel of the other class.  A candidate is a pixel of
    the other class with a 4-neighbour of class c: the nearest pixel q of the other class always is one, because the pixel one step
    from q towards p along an axis in which they differ is strictly nearer to p and therefore of class c.
Nothing exists outside the frame; where the frame holds no pixel of the other class, D = limit."""
import numpy as np

NEAR = 24          # offsets with dy^2 + dx^2 < NEAR^2 are searched by shifting, the rest by pairs


def _offsets(bound, H, W):
    """(d2, dy, dx) of every offset with 0 < d2 < bound inside a frame of H x W, by d2"""
    r = int(np.ceil(np.sqrt(bound)))
    dy, dx = np.mgrid[-min(r, H - 1):min(r, H - 1) + 1, -min(r, W - 1):min(r, W - 1) + 1]
    d2 = dy * dy + dx * dx
    keep = (d2 > 0) & (d2 < bound)
    order = np.argsort(d2[keep], kind='stable')
    return np.stack([d2[keep][order], dy[keep][order], dx[keep][order]], axis=1)


def _to_other(ask, tgt, limit, D):
    """D[p] = min(limit, squared distance from p to the nearest pixel of ``tgt``) for the pixels p of ``ask``"""
    H, W = ask.shape
    if not ask.any() or not tgt.any():
        return
    open_ = ask.copy()
    for n, (d2, dy, dx) in enumerate(_offsets(min(limit, NEAR * NEAR), H, W).tolist()):
        if n % 16 == 0 and not open_.any():
            return
        # p = (y, x) and q = (y + dy, x + dx), both inside the frame
        py, px = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
        qy, qx = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
        hit = open_[py, px] & tgt[qy, qx]
        D[py, px][hit] = d2
        open_[py, px] &= ~hit
    if limit <= NEAR * NEAR or not open_.any():
        return                                   # (what is still open is at least `limit` away)
    near_ask = np.zeros_like(ask)
    near_ask[1:] |= ask[:-1]
    near_ask[:-1] |= ask[1:]
    near_ask[:, 1:] |= ask[:, :-1]
    near_ask[:, :-1] |= ask[:, 1:]
    cy, cx = np.nonzero(tgt & near_ask)
    oy, ox = np.nonzero(open_)
    step = max(1, (1 << 22) // max(1, cy.size))
    for k in range(0, oy.size, step):
        y, x = oy[k:k + step, None].astype(np.int64), ox[k:k + step, None].astype(np.int64)
        d2 = ((y - cy[None]) ** 2 + (x - cx[None]) ** 2).min(axis=1)
        D[oy[k:k + step], ox[k:k + step]] = np.minimum(d2, limit)


def dist2_of(F, limit):
    """F bool [H, W] -> int32 [H, W]: D(p) = min(limit, d2(p))"""
    F = np.asarray(F, dtype=bool)
    D = np.full(F.shape, limit, dtype=np.int64)
    _to_other(F, ~F, limit, D)
    _to_other(~F, F, limit, D)
    return D.astype(np.int32)


def band_of(F, D, inner, outer, mid):
    """the band byte: in F 255 where D > inner else mid; outside F mid where D <= outer else 0"""
    return np.where(F, np.where(D > inner, 255, mid), np.where(D <= outer, mid, 0)).astype(np.uint8)


def edt_band(plane, sets, inner, outer, mid, limit):
    """plane uint8 [H, W], sets uint8 [S, 256] -> (dist2 int32 [S, H, W], band uint8 [S, H, W])"""
    plane, sets = np.asarray(plane, dtype=np.uint8), np.asarray(sets, dtype=np.uint8).reshape(-1, 256)
    assert plane.ndim == 2 and inner >= 0 and outer >= 0 and max(inner, outer) < limit <= 65536 and 0 <= mid <= 255
    S = sets.shape[0]
    dist2 = np.zeros((S,) + plane.shape, dtype=np.int32)
    band = np.zeros((S,) + plane.shape, dtype=np.uint8)
    for s in range(S):
        F = sets[s][plane] != 0
        dist2[s] = dist2_of(F, limit)
        band[s] = band_of(F, dist2[s], inner, outer, mid)
    return dist2, band


def sets_of(*groups):
    """uint8 [S, 256] with set s = the ids of groups[s]"""
    sets = np.zeros((len(groups), 256), dtype=np.uint8)
    for s, ids in enumerate(groups):
        sets[s, list(ids)] = 1
    return sets
