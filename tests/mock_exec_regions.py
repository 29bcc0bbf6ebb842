"""The descriptor interpreter of tests/mock_exec_tracks.py with the region filter (PROB_TO_ID flags == 2048) through the numpy model
(tests/region_ref.py), so that every path of a ResultSaver with min_region / fill_holes runs on the CPU -- and, for BURST under
egress='device', the RLE stage (flags == 32) through the host codec (cutie_amd/inference/utils/coco_rle.py)."""
import numpy as np
import torch

from cutie_amd.inference.utils import coco_rle

import region_ref
from mock_exec import I32, U8, view
from mock_exec_tracks import TracksMockExecutor


class RegionsMockExecutor(TracksMockExecutor):
    def __init__(self):
        super().__init__()
        self.region_calls = []               # (H, W, min_region, fill_holes, connectivity) of every region-filter op

    def _op_36(self, flags, i, f, p):
        if flags == 32:
            return self._rle(i, p)
        if flags != 2048:
            return super()._op_36(flags, i, f, p)
        H, W, min_region, fill_holes, conn = i[1], i[2], i[3], i[4], i[5]
        assert H >= 1 and W >= 1 and min_region >= 0 and fill_holes >= 0 and conn in (4, 8)
        assert p[2] and p[5] and p[7] and p[5] % 4 == 0 and p[7] % 4 == 0 and i[8] + (i[9] << 31) >= 2 * H * W
        self.region_calls.append((H, W, min_region, fill_holes, conn))
        plane = view(p[2], U8, (H, W))
        out, counts = region_ref.region_filter(plane.numpy().copy(), min_region, fill_holes, conn)
        plane.copy_(torch.from_numpy(out))
        view(p[7], I32, (4,)).copy_(torch.from_numpy(counts))

    def _rle(self, i, p):
        H, W, n = i[1], i[2], i[9]
        ids = view(p[2], U8, (H, W)).numpy()
        objs = view(p[6], I32, (n,)).tolist() if n else []
        rows, blob = [], b''
        for oid in objs:
            seg = ids == oid
            s = coco_rle.encode(seg).encode('ascii') if seg.any() else b''
            rows.append([len(blob), len(s), 0, int(seg.sum())])
            blob += s
        assert len(blob) <= i[7]
        if blob:
            view(p[3], U8, (len(blob),)).copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        if n:
            view(p[7], I32, (n, 4)).copy_(torch.from_numpy(np.array(rows, dtype=np.int32)))
        view(p[4], I32, (4,)).copy_(torch.tensor([len(blob), 0, 0, 0], dtype=torch.int32))
