"""The descriptor interpreter of tests/mock_exec_guided.py with the redaction stage (PROB_TO_ID flags == 65536) through the model
(tests/redact_ref.py), so that every path of a ResultSaver with redact= runs on the CPU.  The descriptor's invariants are asserted as
the launcher checks them."""
import numpy as np
import torch

import redact_ref
from mock_exec import U8, view
from mock_exec_guided import GuidedMockExecutor
from cutie_amd import ops as O


def _overlap(a, na, b, nb):
    return a < b + nb and b < a + na


class RedactMockExecutor(GuidedMockExecutor):
    def __init__(self):
        super().__init__()
        self.redact_calls = []               # (H, W, mode, strength, colour, invert) of every op
        self.redact_log = []                 # (frame, weight, out) of every op, copies

    def _op_36(self, flags, i, f, p):
        if flags != 65536:
            return super()._op_36(flags, i, f, p)
        H, W, strength, ldf, ldw, mode, inv, color = i[1], i[2], i[3], i[4], i[5], i[6], i[9], i[10]
        assert H >= 1 and W >= 1 and H * W < 1 << 31 and mode in (0, 1, 2) and inv in (0, 1) and 0 <= color < 1 << 24
        assert mode != 0 or 1 <= strength <= O.OpList.REDACT_MAX_RADIUS
        assert mode != 1 or 2 <= strength <= O.OpList.REDACT_MAX_CELL
        assert p[2] and p[6] and p[3] and p[5] and p[5] % 4 == 0 and ldf >= 3 * W and ldw >= W
        need = O.OpList.redact_scratch_words(mode, H, W, strength)
        assert i[7] >= 0 and i[8] >= 0 and i[8] + (i[7] << 31) >= need
        for at, n in ((p[2], (H - 1) * ldf + 3 * W), (p[6], (H - 1) * ldw + W)):        # neither the output nor the scratch touches an input
            assert not _overlap(p[3], 3 * H * W, at, n) and not _overlap(p[5], 4 * need, at, n)
        assert not _overlap(p[3], 3 * H * W, p[5], 4 * need)
        frame = view(p[2], U8, (H, W, 3), (ldf, 3, 1)).numpy().copy()
        weight = view(p[6], U8, (H, W), (ldw, 1)).numpy().copy()
        rgb = (color & 255, color >> 8 & 255, color >> 16 & 255)
        out = redact_ref.model(frame, weight, mode, strength, rgb, bool(inv))
        self.redact_calls.append((H, W, mode, strength, rgb, inv))
        self.redact_log.append((frame, weight, out))
        view(p[3], U8, (H, W, 3)).copy_(torch.from_numpy(out))
