"""The batch forms of the GPU JPEG decode (RESIZE flags 8 / 16 / 32 with 256; include/cutie_hip.h, ABI 11, forms added) on the CPU: the
table / header check of cutie_amd/csrc/jpeg.hip load_img in Python, and an interpreter that runs the forms image by image through the
integer reference (tests/jpeg_ref.py); it also runs the multi-scale merge (PROB_TO_ID flags & 16) by its numpy model
(tests/merge_ref.py), which the --sizes driver needs.  TEST INFRASTRUCTURE ONLY."""
from collections import Counter

import numpy as np
import torch

from cutie_amd.inference.data import jpeg as J

import jpeg_ref
import merge_ref
from mock_exec import F32, I32, U8, view
from test_jpeg_cpu import JpegMock, _host

ERR_TABLE = 4
R_PKT, R_WORK, R_COEF, R_PLANES, R_RGB, R_PKT_BYTES, R_LD = range(7)
# descriptor ints
I_N, I_PKT, I_WORK, I_COEF, I_PLANES, I_RGB, I_ROUNDS, I_MAX_CHUNK, I_MAX_SEG, I_MAX_BLOCK, I_MAX_PIX = range(11)


def check_row(tab, k, pkts, i):
    """Row k of the table and its packet header against the descriptor ints, as every kernel checks them -> the header, or None."""
    r = [int(v) for v in tab[k]]
    po, pb = r[R_PKT], r[R_PKT_BYTES]
    if po < 0 or po % 16 or pb < 4 * J.HDR_WORDS or pb % 4 or po + pb > i[I_PKT]:
        return None
    h = [int(v) for v in pkts[po:po + 4 * J.HDR_WORDS].view(np.int32)]
    if h[J.HDR_MAGIC] != J.MAGIC or h[J.HDR_BYTES] != pb:
        return None
    words = pb // 4
    nchunk, nseg, nblock, ncomp, H, W = (h[x] for x in (J.HDR_NCHUNK, J.HDR_NSEG, J.HDR_NBLOCK, J.HDR_NCOMP, J.HDR_H, J.HDR_W))
    if not (1 <= nchunk <= i[I_MAX_CHUNK] and 1 <= nseg <= i[I_MAX_SEG] and 1 <= nblock <= i[I_MAX_BLOCK]):
        return None
    if H < 1 or W < 1 or H * W > i[I_MAX_PIX] or ncomp not in (1, 3) or h[J.HDR_CHUNK_BITS] < 64:
        return None
    if not (1 <= h[J.HDR_BPM] <= J.MAX_BPM and 1 <= h[J.HDR_NTAB] <= 6 and h[J.HDR_MCUS_X] >= 1 and h[J.HDR_NMCU] >= 1 and h[J.HDR_RI] >= 1
            and h[J.HDR_HMAX] in (1, 2) and h[J.HDR_VMAX] in (1, 2)):
        return None
    for off, n in ((J.HDR_OFF_SEG, 4 * nseg), (J.HDR_OFF_C2S, nchunk), (J.HDR_OFF_COMP, 3 * J.COMP_WORDS), (J.HDR_OFF_MB, 4 * J.MAX_BPM),
                   (J.HDR_OFF_Q, 64 * ncomp), (J.HDR_OFF_HUFF, h[J.HDR_NTAB] * J.TABW)):
        if h[off] < J.HDR_WORDS or h[off] + n > words:
            return None
    if not 4 * J.HDR_WORDS <= h[J.HDR_OFF_DATA] <= pb:
        return None
    wo = r[R_WORK]
    wend = int(tab[k + 1][R_WORK]) if k + 1 < i[I_N] else i[I_WORK]
    if wo < 0 or wo % 2 or wend < wo or wend > i[I_WORK] or 10 * nchunk + (i[I_ROUNDS] + 1) * nseg > wend - wo:
        return None
    if r[R_COEF] < 0 or r[R_COEF] % 8 or r[R_COEF] + 64 * nblock > i[I_COEF]:
        return None
    if r[R_PLANES] < 0 or r[R_PLANES] % 8 or h[J.HDR_PLANE_BYTES] < 64 * nblock or r[R_PLANES] + h[J.HDR_PLANE_BYTES] > i[I_PLANES]:
        return None
    if r[R_RGB] < 0 or r[R_RGB] % 16 or r[R_LD] < 3 * W or r[R_RGB] + (H - 1) * r[R_LD] + 3 * W > i[I_RGB]:
        return None
    return h


class JpegBatchMock(JpegMock):
    """JpegMock with the batch forms: every image of the table through the reference, after the table / header check; an image that
    fails it gets error bit 4 and is skipped.  ``batch_ops`` counts the batch descriptors by stage flag, ``one_frame`` the one-frame ones."""
    batch_ops = Counter()
    one_frame = 0

    @classmethod
    def reset(cls):
        cls.batch_ops, cls.one_frame = Counter(), 0

    def _op_36(self, flags, i, f, p):
        """PROB_TO_ID flags & 16, the merge of the --sizes driver (host egress), by its numpy model (tests/merge_ref.py)."""
        if not flags & 16:
            return super()._op_36(flags, i, f, p)
        assert not flags & 8
        P, OH, OW, S = i[0], i[5], i[6], i[9]
        ptrs, geom = _host(p[0], np.uint64, S), _host(p[6], np.int32, 4 * S).reshape(S, 4)
        probs = [view(int(ptrs[s]), F32, (P, int(h), int(w)), (int(ps), int(rs), 1)).numpy() for s, (h, w, ps, rs) in enumerate(geom)]
        ids = merge_ref.merge(probs, view(p[1], I32, (P,)).numpy(), OH, OW)
        view(p[2], {0: U8, 1: I32}[flags & 3], (OH, OW)).copy_(torch.from_numpy(ids))

    def _op_37(self, flags, i, f, p):
        if not flags & 256:
            if flags & 56:
                JpegBatchMock.one_frame += 1
            return super()._op_37(flags, i, f, p)
        assert flags & 56 and not flags & ~(256 | 56), flags
        n = i[I_N]
        assert 1 <= n <= 65535 and p[0] % 16 == 0 and p[1] % 16 == 0 and p[6] % 16 == 0
        pkts, tab = _host(p[0], np.uint8, i[I_PKT]), _host(p[1], np.int32, 8 * n).reshape(n, 8)
        status = _host(p[6], np.int32, 4 * n).reshape(n, 4)
        for stage in (8, 16, 32):
            if flags & stage:
                JpegBatchMock.batch_ops[stage] += 1
        if flags & 8:
            assert p[2] % 8 == 0 and p[3] % 16 == 0
            status[:] = 0
        for k in range(n):
            h = check_row(tab, k, pkts, i)
            if h is None:
                status[k, 0] |= ERR_TABLE
                continue
            r = [int(v) for v in tab[k]]
            buf = pkts[r[R_PKT]:r[R_PKT] + r[R_PKT_BYTES]].copy()
            nblock, H, W, plane_bytes = h[J.HDR_NBLOCK], h[J.HDR_H], h[J.HDR_W], h[J.HDR_PLANE_BYTES]
            if flags & 8:
                coef, err = jpeg_ref.huff(buf)
                _host(p[3], np.int16, i[I_COEF])[r[R_COEF]:r[R_COEF] + nblock * 64] = coef.reshape(-1)
                status[k, :3] = (err, 1, 0)
            if flags & 16:
                coef = _host(p[3], np.int16, i[I_COEF])[r[R_COEF]:r[R_COEF] + nblock * 64].reshape(nblock, 64)
                _host(p[4], np.uint8, i[I_PLANES])[r[R_PLANES]:r[R_PLANES] + plane_bytes] = jpeg_ref.idct(buf, coef)
            if flags & 32:
                rgb = jpeg_ref.color(buf, _host(p[4], np.uint8, i[I_PLANES])[r[R_PLANES]:r[R_PLANES] + plane_bytes])
                out = _host(p[5], np.uint8, i[I_RGB])
                for y in range(H):
                    o = r[R_RGB] + y * r[R_LD]
                    out[o:o + 3 * W] = rgb[y].reshape(-1)
