"""The descriptor interpreter (tests/mock_exec.py, with the mixed lock-step forms of tests/mock_exec_mixed.py) with the forms of PROB_TO_ID
that a ResultSaver with ``tracks`` issues on every path: the track statistics (flags == 1024) through the numpy model (tests/track_ref.py),
and -- so that egress='device' and ``process_merged`` run on the CPU as well -- the resampled ids (flags&4), the merge of S sources
(flags&16) and the PNG stage (flags&8) through their own models (tests/merge_ref.py, tests/png_ref.py)."""
import numpy as np
import torch

import merge_ref
import png_ref
import track_ref
from mock_exec import F32, I32, U8, U64, view
from mock_exec_mixed import MixedMockExecutor


class TracksMockExecutor(MixedMockExecutor):
    def __init__(self):
        super().__init__()
        self.track_calls = []                # (H, W, n, with probabilities) of every track-statistics op

    def _op_36(self, flags, i, f, p):
        if flags == 1024:
            return self._track_stats(i, p)
        if not flags & (4 | 8 | 16):
            return super()._op_36(flags, i, f, p)
        assert not flags & ~31 and (flags & 3) == 0, flags
        if flags & 16:                                                       # S sources merged at (i5, i6)
            S, OH, OW, P = i[9], i[5], i[6], i[0]
            ptrs = view(p[0], U64, (S,)).tolist()
            geom = view(p[6], I32, (S, 4)).tolist()
            probs = [view(ptr, F32, (P, h, w), (plane, ldrow, 1)).numpy() for ptr, (h, w, plane, ldrow) in zip(ptrs, geom)]
            ids = merge_ref.merge(probs, view(p[1], I32, (P,)).tolist(), OH, OW).astype(np.uint8)
            view(p[2], U8, (OH, OW)).copy_(torch.from_numpy(ids))
        elif p[0]:
            P, H, W, plane, ldrow = i[:5]
            OH, OW = (i[5], i[6]) if flags & 4 else (H, W)
            prob = view(p[0], F32, (P, H, W), (plane, ldrow, 1)).numpy()
            if (OH, OW) != (H, W):
                prob = merge_ref.resize(prob, OH, OW)
            arg, _ = track_ref.winners(prob)
            ids = np.asarray(view(p[1], I32, (P,)).tolist(), dtype=np.uint8)[arg]
            view(p[2], U8, (OH, OW)).copy_(torch.from_numpy(ids))
        else:                                                                # the PNG stage on its own, on an existing plane
            OH, OW = i[1], i[2]
            ids = view(p[2], U8, (OH, OW)).numpy().copy()
        if flags & 8:
            stream, adler = png_ref.encode(ids)
            assert len(stream) <= i[7]
            view(p[3], U8, (len(stream),)).copy_(torch.frombuffer(bytearray(stream), dtype=torch.uint8))
            view(p[4], I32, (4,)).copy_(torch.from_numpy(np.array([len(stream), adler, 0, 0], dtype=np.uint32).view(np.int32)))

    def _track_stats(self, i, p):
        H, W, n = i[1], i[2], i[9]
        assert H >= 1 and W >= 1 and 0 <= n <= 255 and p[2]
        prob = lut = None
        if p[0]:
            P, h, w = i[0], i[5], i[6]
            assert 1 <= P <= 256 and p[1] and i[4] >= w
            prob = view(p[0], F32, (P, h, w), (i[3], i[4], 1)).numpy()
            lut = view(p[1], I32, (P,)).tolist()
        self.track_calls.append((H, W, n, prob is not None))
        if n == 0:
            return
        assert p[6] and p[7] and p[7] % 16 == 0
        objs = view(p[6], I32, (n,)).tolist()
        want = track_ref.table(view(p[2], U8, (H, W)).numpy(), objs, prob, lut)
        view(p[7], I32, (n, track_ref.WORDS)).copy_(torch.from_numpy(want.copy()))
