"""The descriptor interpreter of tests/mock_exec_polygons.py with the filtered, dynamic-Huffman PNG stage (PROB_TO_ID flags == 16384)
through the model (tests/png_photo_ref.py), so that every path of a ResultSaver with cutout= / png_codes='dynamic' runs on the CPU.  The
stream's capacity is honoured: the error bit can be raised."""
import numpy as np
import torch

import png_photo_ref
from mock_exec import I32, U8, view
from mock_exec_polygons import PolygonMockExecutor
from cutie_amd import ops as O


class PngPhotoMockExecutor(PolygonMockExecutor):
    def __init__(self):
        super().__init__()
        self.png_photo_calls = []            # (H, W, B, status words) of every op

    def _op_36(self, flags, i, f, p):
        if flags != 16384:
            return super()._op_36(flags, i, f, p)
        H, W, c0, ld0, ld1, cap = i[1], i[2], i[3], i[4], i[5], i[7]
        B = c0 + (1 if p[6] else 0)
        assert H >= 1 and W >= 1 and c0 in (1, 3) and W * B + 1 <= O.OpList.PNG_PHOTO_ROW_LIMIT and ld0 >= W * c0 and (not p[6] or ld1 >= W)
        assert cap >= 0 and p[2] and p[4] and p[5] and (p[3] or cap < 4) and p[3] % 4 == 0 and p[4] % 4 == 0 and p[5] % 16 == 0
        assert i[8] >= O.OpList.png_photo_scratch_words(H, W, B)
        src = view(p[2], U8, (H, W, c0), (ld0, c0, 1)).numpy().copy()
        last = view(p[6], U8, (H, W), (ld1, 1)).numpy().copy() if p[6] else None
        stream, status = png_photo_ref.stage(src[:, :, 0] if c0 == 1 else src, last, cap)
        self.png_photo_calls.append((H, W, B, status.tolist()))
        view(p[4], I32, (4,)).copy_(torch.from_numpy(status))
        if stream is not None:
            view(p[3], U8, (len(stream),)).copy_(torch.frombuffer(bytearray(stream), dtype=torch.uint8))
