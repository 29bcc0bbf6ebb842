"""The descriptor interpreter of tests/mock_exec_edt.py with the polygon trace (PROB_TO_ID flags == 8192) through the model
(tests/polygon_ref.py), so that every path of a ResultSaver with polygons= runs on the CPU.  The stream's capacity and the edge capacity are
honoured: the error bits can be raised."""
import numpy as np
import torch

import polygon_ref
from mock_exec import I32, U8, view
from mock_exec_edt import EdtMockExecutor
from cutie_amd import ops as O


class PolygonMockExecutor(EdtMockExecutor):
    def __init__(self):
        super().__init__()
        self.polygon_calls = []              # (H, W, n, connectivity, path, status words) of every polygon op

    def _op_36(self, flags, i, f, p):
        if flags != 8192:
            return super()._op_36(flags, i, f, p)
        H, W, C, cap, conn, path, n = i[1], i[2], i[3], i[4], i[5], i[6], i[9]
        assert 1 <= H <= 65535 and 1 <= W <= 65535 and (H + 1) * (W + 1) < 1 << 29 and 0 <= n <= 255 and conn in (4, 8) and path in (0, 1)
        assert C >= 1 and cap >= 0 and cap % 4 == 0
        assert p[2] and p[4] and p[5] and (p[3] or cap == 0) and p[3] % 16 == 0 and p[5] % 16 == 0 and p[7] % 16 == 0
        assert n == 0 or (p[6] and p[7])
        assert i[8] + (i[7] << 31) >= O.OpList.polygon_scratch_words(H, W, n, C)
        plane = view(p[2], U8, (H, W)).numpy().copy()
        objs = view(p[6], I32, (n,)).numpy().tolist() if n else []
        words, table, status = polygon_ref.stage(plane, objs, conn, C, cap)
        self.polygon_calls.append((H, W, n, conn, path, status.tolist()))
        view(p[4], I32, (4,)).copy_(torch.from_numpy(status))
        if n:
            view(p[7], I32, (n, 4)).copy_(torch.from_numpy(np.ascontiguousarray(table)))
        if words is not None and len(words):
            view(p[3], I32, (len(words),)).copy_(torch.from_numpy(words.view(np.int32).copy()))
