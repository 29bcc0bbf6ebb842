"""The model of the polygon trace (PROB_TO_ID flags == 8192; the contract: include/cutie_hip.h): a direct walk
over a set of directed boundary edges, written for clarity.  It shares no code with cutie_amd.inference.utils.polygons.trace_rings.

x runs right, y down.  Pixel (x, y) is the unit square [x, x + 1] x [y, y + 1]; an edge is (x, y, d) = tail vertex and direction, with
the object on the right of the direction of travel; outside the frame nothing belongs to the object."""
import numpy as np

STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))          # d = 0 E, 1 S, 2 W, 3 N


def object_rows(obj_ids):
    """-> {id: row} of the entries that name an object: inside 1 .. 255 and not named by an earlier entry."""
    rows = {}
    for k, v in enumerate(obj_ids):
        v = int(v)
        if 1 <= v <= 255 and v not in rows:
            rows[v] = k
    return rows


def boundary_edges(mask):
    """The directed boundary edges of a boolean mask [H, W] as a set of (x, y, d)."""
    H, W = mask.shape
    inside = lambda x, y: 0 <= x < W and 0 <= y < H and bool(mask[y, x])
    edges = set()
    for y in range(H):
        for x in range(W):
            if not mask[y, x]:
                continue
            if not inside(x, y - 1):
                edges.add((x, y, 0))                 # top, east
            if not inside(x + 1, y):
                edges.add((x + 1, y, 1))             # right, south
            if not inside(x, y + 1):
                edges.add((x + 1, y + 1, 2))         # bottom, west
            if not inside(x - 1, y):
                edges.add((x, y + 1, 3))             # left, north
    return edges


def successor(edges, edge, connectivity):
    x, y, d = edge
    hx, hy = x + STEP[d][0], y + STEP[d][1]
    turns = (3, 0, 1) if connectivity == 8 else (1, 0, 3)       # left, straight, right | right, straight, left
    for t in turns:
        nxt = (hx, hy, (d + t) & 3)
        if nxt in edges:
            return nxt
    raise AssertionError(f'no edge leaves the head of {edge}')


def rings_of_mask(mask, connectivity):
    """-> [(points [(x, y) ...], L, first edge (x, y, d))] in the order of the first edge's (y, x, d)."""
    assert connectivity in (4, 8)
    edges = boundary_edges(mask)
    seen, rings = set(), []
    for first in sorted(edges, key=lambda e: (e[1], e[0], e[2])):
        if first in seen:
            continue
        walk, e = [], first
        while e not in seen:
            seen.add(e)
            walk.append(e)
            e = successor(edges, e, connectivity)
        assert e == first, 'the successor is not a permutation'
        points = [(w[0], w[1]) for k, w in enumerate(walk) if walk[k - 1][2] != w[2]]
        rings.append((points, len(walk), first))
    return rings


def shoelace2(points):
    """Twice the signed area: positive for an outer ring, negative for a hole (y down, object on the right)."""
    s = 0
    for k, (x0, y0) in enumerate(points):
        x1, y1 = points[(k + 1) % len(points)]
        s += x0 * y1 - x1 * y0
    return s


def trace(plane, obj_ids, connectivity):
    """-> rings int32 [R, 4] (object row | first vertex | vertices | edges), vertices uint32 [V] (x | y << 16), table int32 [n, 4]
    (first ring | rings | first vertex | vertices), E."""
    plane = np.asarray(plane)
    rows = object_rows(obj_ids)
    by_row = {k: v for v, k in rows.items()}
    ring_rows, verts, table, E = [], [], [], 0
    for k in range(len(obj_ids)):
        r0, v0 = len(ring_rows), len(verts)
        if k in by_row:
            for points, L, _ in rings_of_mask(plane == by_row[k], connectivity):
                ring_rows.append((k, len(verts), len(points), L))
                verts.extend(x | y << 16 for x, y in points)
                E += L
        table.append((r0, len(ring_rows) - r0, v0, len(verts) - v0))
    return (np.array(ring_rows, dtype=np.int32).reshape(-1, 4), np.array(verts, dtype=np.uint32),
            np.array(table, dtype=np.int32).reshape(-1, 4), E)


def stage(plane, obj_ids, connectivity, edge_capacity, stream_bytes):
    """What the stage leaves: (stream words uint32 [4 R + V] or None when nothing is written, table int32 [n, 4], status int32 [4])."""
    rings, verts, table, E = trace(plane, obj_ids, connectivity)
    n = len(obj_ids)
    if n == 0:
        return None, table, np.zeros(4, dtype=np.int32)
    if E > edge_capacity:
        return None, np.zeros((n, 4), dtype=np.int32), np.array([0, 2, 0, E], dtype=np.int32)
    nbytes = 16 * len(rings) + 4 * len(verts)
    if nbytes > stream_bytes:
        table = table.copy()
        table[:, 0] = 0
        table[:, 2] = 0
        return None, table, np.array([nbytes, 1, len(rings), E], dtype=np.int32)
    words = np.concatenate([rings.reshape(-1).view(np.uint32), verts])
    return words, table, np.array([nbytes, 0, len(rings), E], dtype=np.int32)


def fill(rings, verts, H, W):
    """Crack-parity fill of ring rows and packed vertices -> {object row: bool [H, W]}.  A vertical edge at column x toggles every pixel
    to its right on its rows; the xor along x is the mask."""
    out = {}
    for k, v0, nv, _ in np.asarray(rings).reshape(-1, 4).tolist():
        acc = out.setdefault(k, np.zeros((H, W + 1), dtype=bool))
        pts = [(int(p) & 0xffff, int(p) >> 16) for p in verts[v0:v0 + nv]]
        for q, (x0, y0) in enumerate(pts):
            x1, y1 = pts[(q + 1) % nv]
            if x0 == x1:
                acc[min(y0, y1):max(y0, y1), x0] ^= True
    return {k: np.logical_xor.accumulate(a, axis=1)[:, :W] for k, a in out.items()}
