"""The descriptor interpreter of tests/mock_exec_png_photo.py with the colour guided filter (PROB_TO_ID flags == 32768) through the model
(tests/guided_ref.py), so that every path of a ResultSaver with matte_refine= runs on the CPU.  The descriptor's invariants are asserted as
the launcher checks them."""
import numpy as np
import torch

import guided_ref
from mock_exec import U8, view
from mock_exec_png_photo import PngPhotoMockExecutor
from cutie_amd import ops as O


def _overlap(a, na, b, nb):
    return a < b + nb and b < a + na


class GuidedMockExecutor(PngPhotoMockExecutor):
    def __init__(self):
        super().__init__()
        self.guided_calls = []               # (H, W, S, radius, eps) of every op

    def _op_36(self, flags, i, f, p):
        if flags != 32768:
            return super()._op_36(flags, i, f, p)
        H, W, r, ldg, ldp, ps, S0, ldl = i[1], i[2], i[3], i[4], i[5], i[6], i[9], i[10]
        eps = float(np.float32(f[0]))
        S = S0 + (1 if p[7] else 0)
        assert H >= 1 and W >= 1 and H * W < 1 << 31 and 1 <= r <= O.OpList.GUIDED_MAX_RADIUS and 1 <= S <= O.OpList.GUIDED_MAX_PLANES and S0 >= 0
        assert np.float32(O.OpList.GUIDED_EPS_MIN) <= np.float32(eps) <= np.float32(O.OpList.GUIDED_EPS_MAX)
        assert p[2] and p[3] and p[5] and (p[6] or S0 == 0) and p[5] % 4 == 0 and ldg >= 3 * W
        assert (S0 == 0 or (ldp >= W and (S0 == 1 or ps >= (H - 1) * ldp + W))) and (not p[7] or ldl >= W)
        need = O.OpList.guided_scratch_words(S, H, W)
        assert i[7] >= 0 and i[8] >= 0 and i[8] + (i[7] << 31) >= need
        spans = [(p[2], (H - 1) * ldg + 3 * W)] + ([(p[6], (S0 - 1) * ps + (H - 1) * ldp + W)] if S0 else []) + ([(p[7], (H - 1) * ldl + W)] if p[7] else [])
        for at, n in spans:                                                          # neither the output nor the scratch touches an input
            assert not _overlap(p[3], S * H * W, at, n) and not _overlap(p[5], 4 * need, at, n)
        assert not _overlap(p[3], S * H * W, p[5], 4 * need)
        guide = view(p[2], U8, (H, W, 3), (ldg, 3, 1)).numpy().copy()
        planes = [view(p[6], U8, (S0, H, W), (ps, ldp, 1)).numpy().copy()] if S0 else []
        if p[7]:
            planes.append(view(p[7], U8, (1, H, W), (0, ldl, 1)).numpy().copy())
        out = guided_ref.model(guide, np.concatenate(planes), r, eps)
        self.guided_calls.append((H, W, S, r, eps))
        view(p[3], U8, (S, H, W)).copy_(torch.from_numpy(out))
