"""The descriptor interpreter of tests/mock_exec_regions.py with the distance stage (PROB_TO_ID flags == 4096) through the numpy model
(tests/edt_ref.py), so that every path of a ResultSaver with trimap / trimap_objects / dilate_mask runs on the CPU."""
import numpy as np
import torch

import edt_ref
from mock_exec import I32, U8, view
from mock_exec_regions import RegionsMockExecutor


class EdtMockExecutor(RegionsMockExecutor):
    def __init__(self):
        super().__init__()
        self.edt_calls = []                  # (H, W, S, inner, outer, limit, mid) of every distance op

    def _op_36(self, flags, i, f, p):
        if flags != 4096:
            return super()._op_36(flags, i, f, p)
        H, W, inner, outer, limit, mid, S = i[1], i[2], i[3], i[4], i[5], i[6], i[9]
        assert H >= 1 and W >= 1 and 1 <= S <= 16 and inner >= 0 and outer >= 0 and max(inner, outer) < limit <= 65536 and 0 <= mid <= 255
        assert p[2] and p[6] and p[5] and (p[3] or p[7]) and p[5] % 4 == 0 and p[7] % 4 == 0
        assert i[8] + (i[7] << 31) >= (S * H * W + 1) // 2
        self.edt_calls.append((H, W, S, inner, outer, limit, mid))
        plane = view(p[2], U8, (H, W)).numpy().copy()
        sets = view(p[6], U8, (S, 256)).numpy().copy()
        dist2, band = edt_ref.edt_band(plane, sets, inner, outer, mid, limit)
        if p[7]:
            view(p[7], I32, (S, H, W)).copy_(torch.from_numpy(dist2))
        if p[3]:
            view(p[3], U8, (S, H, W)).copy_(torch.from_numpy(band))
