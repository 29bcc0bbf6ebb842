"""Polygons of the result masks: the host tracer behind the GPU stage and the writer of polygons.json.

The stage (PROB_TO_ID flags == 8192, OpList.polygon_trace; the contract: include/cutie_hip.h) traces every listed
object of an id plane into rings of lattice corners on the device.  ``trace_rings`` computes the same rows and packed vertices on the host;
it is the fall-back for a frame that overflows a capacity of the stage, as the host codecs are behind the PNG and RLE slabs, and serves
nothing else: the product has no CPU path.

Coordinates are LATTICE CORNERS: pixel (x, y) is the square [x, x + 1] x [y, y + 1], so a one-pixel object at (3, 2) is the ring
(3, 2) (4, 2) (4, 3) (3, 3).  A consumer that wants pixel-centre coordinates subtracts 0.5 from every coordinate.  Rings marked ``hole``
are to be SUBTRACTED from their object (even-odd fill gives the mask back exactly); COCO-style consumers that cannot express holes must
decide for themselves what to do with them."""
import json
import os

import numpy as np


def _rows(obj_ids):
    lut = np.full(257, -1, dtype=np.int64)
    for k, v in enumerate(obj_ids):
        v = int(v)
        if 1 <= v <= 255 and lut[v] < 0:
            lut[v] = k
    return lut


# per direction: the pixel of the object (on the right of travel) and the pixel across, in the quad (NW, NE, SW, SE) of the tail vertex
_IN = (3, 2, 0, 1)
_ACROSS = (1, 3, 2, 0)
_DX = np.array([1, 0, -1, 0])
_DY = np.array([0, 1, 0, -1])


def trace_rings(plane, obj_ids, connectivity=8):
    """plane: uint8 [H, W] (numpy, or anything np.asarray takes); obj_ids: the list of the stage (an entry outside 1 .. 255 or equal to an
    earlier one is an absent object).  -> rings int32 [R, 4] (object row | first vertex | vertices | unit edges), vertices uint32 [V]
    (x | y << 16), table int32 [n, 4] (first ring | rings | first vertex | vertices): word for word what the stage writes."""
    if connectivity not in (4, 8):
        raise ValueError(f'trace_rings: connectivity {connectivity}, 4 or 8')
    plane = np.asarray(plane)
    if plane.ndim != 2 or plane.dtype != np.uint8 or plane.shape[0] < 1 or plane.shape[1] < 1:
        raise ValueError('trace_rings: plane is uint8 [H, W] with H, W >= 1')
    obj_ids = [int(v) for v in obj_ids]
    n = len(obj_ids)
    H, W = plane.shape
    lut = _rows(obj_ids)
    P = np.full((H + 2, W + 2), 256, dtype=np.int64)
    P[1:-1, 1:-1] = plane
    quad = (P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:])            # NW NE SW SE of every vertex, [H + 1, W + 1]
    exists = [(lut[quad[_IN[d]]] >= 0) & (quad[_IN[d]] != quad[_ACROSS[d]]) for d in range(4)]
    eid = np.sort(np.concatenate([np.flatnonzero(exists[d]) * 4 + d for d in range(4)]))      # slot -> edge index, ascending
    E = int(eid.size)
    rings, verts = [], []
    if E:
        d = eid & 3
        vy, vx = np.divmod(eid >> 2, W + 1)
        val = np.choose(d, [quad[_IN[k]][vy, vx] for k in range(4)])
        hx, hy = vx + _DX[d], vy + _DY[d]
        nd = np.full(E, -1, dtype=np.int64)
        for turn in ((3, 0, 1) if connectivity == 8 else (1, 0, 3)):
            c = (d + turn) & 3
            ok = (np.choose(c, [quad[_IN[k]][hy, hx] for k in range(4)]) == val) & (np.choose(c, [quad[_ACROSS[k]][hy, hx] for k in range(4)]) != val)
            nd = np.where((nd < 0) & ok, c, nd)
        succ = np.searchsorted(eid, (hy * (W + 1) + hx) * 4 + nd)
        succ_l, d_l, row_l = succ.tolist(), d.tolist(), lut[val].tolist()
        vx_l, vy_l = vx.tolist(), vy.tolist()
        seen = np.zeros(E, dtype=bool)
        found = []
        for first in range(E):                                             # slots ascend with the edge index: `first` is its ring's first edge
            if seen[first]:
                continue
            pts, L, i, prev_d = [], 0, first, None
            while not seen[i]:
                seen[i] = True
                L += 1
                pts.append((i, d_l[i]))
                i = succ_l[i]
            last_d = pts[-1][1]
            corners = []
            for i, di in pts:
                if di != last_d:
                    corners.append(vx_l[i] | vy_l[i] << 16)
                last_d = di
            found.append((row_l[first], first, corners, L))
        found.sort(key=lambda r: (r[0], r[1]))
        for row, _, corners, L in found:
            rings.append((row, len(verts), len(corners), L))
            verts.extend(corners)
    rings = np.array(rings, dtype=np.int32).reshape(-1, 4)
    table = np.zeros((n, 4), dtype=np.int32)
    r = v = 0
    for k in range(n):
        mine = rings[rings[:, 0] == k]
        table[k] = (r, len(mine), v, int(mine[:, 2].sum()))
        r += len(mine)
        v += int(mine[:, 2].sum())
    return rings, np.array(verts, dtype=np.uint32), table


def ring_area2(points):
    """Twice the signed shoelace area of [(x, y) ...] in int64: positive for an outer ring, negative for a hole."""
    p = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    return int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


class PolygonReport:
    """Collects the traced frames of one video and writes polygons.json (see the module docstring for the coordinate conventions):

    {"video", "height", "width", "connectivity", "objects": [ids],
     "frames": [{"frame", "index", "objects": {"<id>": {"area": A, "rings": [{"hole", "area", "perimeter", "points": [x0, y0, ...]}]}}}]}

    ``area`` of a ring is its absolute shoelace area, of an object the signed sum = its pixel count; an object without a pixel keeps its
    entry with area 0 and no rings; frames stay in the order reported."""

    def __init__(self, video=None, connectivity=8):
        self.video, self.connectivity = video, int(connectivity)
        self.height = self.width = None
        self.objects = []
        self.frames = []

    def add(self, frame_name, frame_index, rings, vertices, table, obj_ids, H, W):
        rings = np.asarray(rings, dtype=np.int32).reshape(-1, 4)
        vertices = np.asarray(vertices, dtype=np.uint32)
        table = np.asarray(table, dtype=np.int32).reshape(-1, 4)
        if self.height is None:
            self.height, self.width = int(H), int(W)
        elif (self.height, self.width) != (int(H), int(W)):
            raise ValueError(f'PolygonReport: a frame of {H} x {W} in a report of {self.height} x {self.width}')
        # the whole frame at once (this runs on the saver's writer thread, next to the thread that issues the launches): the shoelace
        # terms of every vertex against its successor inside its ring, summed per ring; then plain list slices
        x, y = (vertices & 0xffff).astype(np.int64), (vertices >> 16).astype(np.int64)
        nxt = np.arange(1, len(vertices) + 1)
        if len(rings):
            nxt[rings[:, 1] + rings[:, 2] - 1] = rings[:, 1]
            area2 = np.add.reduceat(x * y[nxt] - x[nxt] * y, rings[:, 1]).tolist()
        flat, rows = np.stack([x, y], axis=1).reshape(-1).tolist(), rings.tolist()
        objects, named = {}, set()
        for k, oid in enumerate(int(v) for v in obj_ids):
            if not 1 <= oid <= 255 or oid in named:
                continue
            named.add(oid)
            if oid not in self.objects:
                self.objects.append(oid)
            r0, nr = int(table[k, 0]), int(table[k, 1])
            out = [{'hole': area2[r] < 0, 'area': abs(area2[r]) // 2, 'perimeter': rows[r][3], 'points': flat[2 * rows[r][1]:2 * (rows[r][1] + rows[r][2])]}
                   for r in range(r0, r0 + nr)]
            objects[str(oid)] = {'area': sum(area2[r0:r0 + nr]) // 2 if nr else 0, 'rings': out}
        self.frames.append({'frame': str(frame_name), 'index': int(frame_index), 'objects': objects})

    def as_dict(self):
        return {'video': self.video, 'height': self.height, 'width': self.width, 'connectivity': self.connectivity,
                'objects': list(self.objects), 'frames': self.frames}

    def write(self, directory):
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, 'polygons.json')
        with open(path, 'w') as f:
            f.write(json.dumps(self.as_dict()))      # (dumps, not dump: one pass of the C encoder; dump walks the points in Python)
        return path
