"""The descriptor interpreter (tests/mock_exec.py) with the MIXED forms of the lock-step ops (include/cutie_hip.h: clips in lock step with
different object counts -- UPSAMPLE2X_ADD i6, UP4_SOFTMAX i5, ATTN_Q2P i10, STEM i10, COPY2D i4).  Every mixed form is run as what it stands
for: clip by clip the uniform (one-clip) form of the base interpreter, with the pointers advanced by the prefix sums of the counts."""
import torch

from cutie_amd import ops as O
from mock_exec import U8, MockExecutor, view


def unpack_counts(word):
    """The 3-bit fields of a counts word up to the first zero (ops.pack_counts)."""
    counts = []
    while word & 7:
        counts.append(word & 7)
        word >>= 3
    assert word == 0 and 1 <= len(counts) <= 8, counts
    return counts


class MixedMockExecutor(MockExecutor):
    # ---- UPSAMPLE2X_ADD: object b adds the skip map of its clip ----------------------------------------------------------
    def _op_4(self, flags, i, f, p):
        if not i[6]:
            return super()._op_4(flags, i, f, p)
        B, h, w, C = i[:4]
        counts = unpack_counts(i[6])
        assert sum(counts) == B and i[4] == 0
        st = O.clip_starts(counts)
        for c, k in enumerate(counts):                                   # the one-clip launch: B = K_c objects, one skip map
            pc = list(p)
            pc[0] = p[0] + 2 * st[c] * h * w * C
            pc[1] = p[1] + 2 * c * i[5] * C
            pc[2] = p[2] + 2 * st[c] * 4 * h * w * C
            super()._op_4(flags, [k, h, w, C] + [0] * 20, f, pc)

    # ---- UP4_SOFTMAX: clip c has K_c logit planes in, K_c + 1 planes out, behind those of the clips in front --------------------
    def _op_11(self, flags, i, f, p):
        if not i[5]:
            return super()._op_11(flags, i, f, p)
        h, w = i[1], i[2]
        counts = unpack_counts(i[5])
        assert len(counts) == i[4] and (flags & 1) and not (flags & 8)
        st = O.clip_starts(counts)
        ncell = (h // 4) * (w // 4)
        for c, k in enumerate(counts):
            pc = list(p)
            pc[0] = p[0] + 4 * st[c] * h * w
            pc[1] = p[1] + 4 * (st[c] + c) * 16 * h * w
            pc[2] = p[2] + 4 * (st[c] + c) * 16 * h * w if p[2] else 0
            if flags & 4:
                pc[3], pc[4] = p[3] + 4 * st[c] * ncell, p[4] + 2 * st[c] * ncell * i[3]
            super()._op_11(flags, [k + 1, h, w, i[3], 1] + [0] * 19, f, pc)

    # ---- ATTN_Q2P (chain form): the foreground mask is decided among the objects of the object's own clip ------------------------
    def _op_18(self, flags, i, f, p):
        if not i[10]:
            return super()._op_18(flags, i, f, p)
        K, Q, HW, C = i[:4]
        counts = unpack_counts(i[10])
        assert sum(counts) == K and i[9] == 0 and (flags & 8)
        st = O.clip_starts(counts)
        rows = Q * 256 * 4                                               # bytes of an object's f32 rows [Q, 256]
        for c, k in enumerate(counts):                                   # the one-clip launch over the clip's objects: every per-object pointer advanced
            pc = list(p)
            o = st[c]
            pc[0] = p[0] + o * (Q * (i[7] or 256) * 4 if not (flags & 16) else rows)
            pc[1] = p[1] + 2 * o * HW * i[5]
            pc[2] = p[2] + 4 * o * HW
            if p[3]:
                pc[3] = p[3] + o * rows
            if p[4]:
                pc[4] = p[4] + o * rows
            if not (flags & 16) and p[7]:
                pc[7] = p[7] + o * rows
            if (flags & 4) and p[10]:
                pc[10] = p[10] + 2 * o * rows                            # int64 accumulators
            if p[13]:
                pc[13] = p[13] + 2 * o * rows
            ic = list(i)
            ic[0], ic[9], ic[10] = k, 0, 0
            super()._op_18(flags, ic, f, pc)

    # ---- STEM: the frames are clips with their own object counts; the masks are dense planes -----------------------------------------
    def _op_41(self, flags, i, f, p):
        if not i[10]:
            return super()._op_41(flags, i, f, p)
        H, W = i[2], i[3]
        counts = unpack_counts(i[10])
        assert len(counts) == i[8] and p[1] and i[6] == max(counts)
        st = O.clip_starts(counts)
        for c, k in enumerate(counts):
            pf = list(p[:5]) + [0] * 11
            pf[0] = p[0] if c == 0 else p[4 + c]
            pf[1] = p[1] + 4 * (st[c] + c) * H * W
            pf[4] = p[4] + 2 * st[c] * (H // 4) * (W // 4) * 64
            super()._op_41(flags, i[:6] + [k, i[7]] + [0] * 16, f, pf)

    # ---- COPY2D: destination row r (an object) = the source row of its clip -------------------------------------------------------
    def _op_28(self, flags, i, f, p):
        if not i[4]:
            return super()._op_28(flags, i, f, p)
        rows, rb, ss, ds = i[:4]
        counts = unpack_counts(i[4])
        assert sum(counts) == rows and rb % 16 == 0
        src = view(p[0], U8, (len(counts), rb), (ss, 1)).clone()
        idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
        view(p[1], U8, (rows, rb), (ds, 1)).copy_(src[idx])
