"""The numpy model of the region filter (PROB_TO_ID flags == 2048, include/cutie_hip.h; kernels: cutie_amd/csrc/regions.hip): connected
components of a uint8 id plane by a union-find of its own (no scipy in here: tests/test_region_filter_cpu.py compares this model WITH
scipy.ndimage.label), then the two stages of the contract.

Union-find over arrays: the edges are the pairs of neighbouring pixels of the stage's kind with equal ids.  A round hooks, for every edge
whose ends have different roots, the larger root under the smaller (np.minimum.at: the smallest candidate stays), then compresses every path.
A root that is not its component's smallest index either hooks or is hooked onto in every round, so the number of trees at least halves: a
few rounds, whatever the shape of the component.  Parents only ever decrease: the root of a component is its smallest linear index, its
first pixel in raster order."""
import numpy as np


def _edges(key, connectivity):
    """key: int [H, W], -1 = not of the stage's kind.  -> (a, b) linear indices of the connected neighbour pairs"""
    H, W = key.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pairs = [(slice(None), slice(1, None), slice(None), slice(None, -1)),               # left
             (slice(1, None), slice(None), slice(None, -1), slice(None))]               # up
    if connectivity == 8:
        pairs += [(slice(1, None), slice(1, None), slice(None, -1), slice(None, -1)),   # up-left
                  (slice(1, None), slice(None, -1), slice(None, -1), slice(1, None))]   # up-right
    a, b = [], []
    for ya, xa, yb, xb in pairs:
        ka, kb = key[ya, xa], key[yb, xb]
        m = (ka >= 0) & (ka == kb)
        a.append(idx[ya, xa][m])
        b.append(idx[yb, xb][m])
    return np.concatenate(a), np.concatenate(b)


def roots(key, connectivity):
    """-> int64 [H, W]: the smallest linear index of every pixel's component (-1 where key is -1)"""
    if connectivity not in (4, 8):
        raise ValueError(f'connectivity {connectivity}')
    H, W = key.shape
    parent = np.arange(H * W, dtype=np.int64)
    a, b = _edges(key, connectivity)
    while a.size:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        a, b, ra, rb = a[differ], b[differ], ra[differ], rb[differ]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    out = parent.reshape(H, W)
    out[key < 0] = -1
    return out


def islands(ids, min_region, connectivity=8):
    """Stage A -> (plane, components removed, pixels cleared)"""
    ids = np.asarray(ids, dtype=np.uint8)
    if min_region < 2:
        return ids.copy(), 0, 0
    key = np.where(ids != 0, ids.astype(np.int64), -1)
    r = roots(key, connectivity)
    area = np.bincount(r[r >= 0], minlength=ids.size)
    small = (r >= 0) & (area[np.maximum(r, 0)] < min_region)
    out = ids.copy()
    out[small] = 0
    return out, int(np.unique(r[small]).size), int(small.sum())


def holes(ids, fill_holes, connectivity=8):
    """Stage B -> (plane, components filled, pixels filled)"""
    ids = np.asarray(ids, dtype=np.uint8)
    if fill_holes < 2:
        return ids.copy(), 0, 0
    H, W = ids.shape
    key = np.where(ids == 0, 0, -1).astype(np.int64)
    r = roots(key, connectivity)
    area = np.bincount(r[r >= 0], minlength=ids.size)
    frame = np.zeros((H, W), dtype=bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    open_ = np.zeros(ids.size, dtype=bool)
    open_[r[frame & (r >= 0)]] = True
    rr = np.maximum(r, 0)
    fill = (r >= 0) & ~open_[rr] & (area[rr] < fill_holes)
    out = ids.copy()
    if fill.any():
        first = r[fill]
        assert (first % W > 0).all()                          # the pixel left of the first pixel exists ...
        source = ids.reshape(-1)[first - 1]
        assert (source != 0).all()                            # ... and is an object's
        out[fill] = source
    return out, int(np.unique(r[fill]).size), int(fill.sum())


def region_filter(ids, min_region=0, fill_holes=0, connectivity=8):
    """-> (plane uint8 [H, W], counts int32 [4]: islands removed | pixels cleared | holes filled | pixels filled)"""
    if min_region < 0 or fill_holes < 0:
        raise ValueError('negative threshold')
    a, n_islands, cleared = islands(ids, min_region, connectivity)
    b, n_holes, filled = holes(a, fill_holes, connectivity)
    return b, np.array([n_islands, cleared, n_holes, filled], dtype=np.int32)
