"""Numpy model of PROB_TO_ID flags == 128 (include/cutie_hip.h ABI 11, csrc/jpeg_enc.hip): overlay blend + libjpeg-turbo's baseline
encoder path (4:2:0, ISLOW FDCT, standard Huffman tables) -> the entropy-coded segment.  TEST INFRASTRUCTURE ONLY.

    encode(frame, ids, ctab, qt) -> bytes        # byte-stuffed, padded with 1-bits; header and EOI: utils/jpeg_writer.py

Every intermediate of the FDCT is computed in int64 and asserted to fit int32 (the kernels use 32-bit integers).
``EncodeExecutor`` wraps tests/mock_exec.py's interpreter and serves the stage from this model (host memory)."""
import numpy as np

from cutie_amd.inference.utils import jpeg_writer as JW

_I32 = 1 << 31


def blend(frame, ids, ctab):
    """uint8 [H, W, 3]: where id == 0 the frame, elsewhere (frame + colour[id]) >> 1.  ids None: the frame."""
    frame = np.asarray(frame, dtype=np.uint8)
    if ids is None:
        return frame.copy()
    ids = np.asarray(ids, dtype=np.uint8)
    mix = ((frame.astype(np.int32) + np.asarray(ctab, dtype=np.uint8)[ids][..., :3].astype(np.int32)) >> 1).astype(np.uint8)
    return np.where((ids != 0)[..., None], mix, frame)


def ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def geometry(H, W):
    cw, ch = -(-W // 2), -(-H // 2)
    return dict(bw_y=-(-W // 8), bh_y=-(-H // 8), cw=cw, ch=ch, bw_c=-(-cw // 8), bh_c=-(-ch // 8), mw=-(-W // 16), mh=-(-H // 16))


def _pad(plane, rows, cols):
    """Replicate the last column out to `cols`, then the last row out to `rows`."""
    h, w = plane.shape
    return np.pad(plane, ((0, rows - h), (0, cols - w)), mode='edge')


def planes(rgb):
    """-> Y [8 bh_y, 8 bw_y], Cb, Cr [8 bh_c, 8 bw_c] as the encoder's DCT sees them (before the level shift)."""
    H, W = rgb.shape[:2]
    g = geometry(H, W)
    y, cb, cr = ycc(rgb)
    out = [_pad(y, 8 * g['bh_y'], 8 * g['bw_y'])]
    bias = np.tile(np.array([1, 2], dtype=np.int64), 4 * g['bw_c'])[None, :]
    for c in (cb, cr):
        c = _pad(c, 2 * g['ch'], 16 * g['bw_c'])             # the input's last column out to 16 x blocks, its last row once if H is odd
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(d, 8 * g['bh_c'], 8 * g['bw_c']))     # the last DOWNSAMPLED row out to whole blocks
    return out


def _chk(*xs):
    for x in xs:
        assert np.abs(x).max(initial=0) < _I32, 'an FDCT intermediate leaves int32'
    return xs[0] if len(xs) == 1 else xs


def _descale(x, n):
    _chk(x + (1 << (n - 1)))
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """jfdctint.c, one pass over the last axis of d [..., 8] (int64)."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = _chk((t12 + t13) * 4433)
    out[..., 2] = _descale(_chk(z1 + t13 * 6270), n)
    out[..., 6] = _descale(_chk(z1 + t12 * -15137), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = _chk((z3 + z4) * 9633)
    t4, t5, t6, t7 = _chk(t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299)
    z1, z2, z3, z4 = _chk(z1 * -7373, z2 * -20995, z3 * -16069, z4 * -3196)
    z3, z4 = _chk(z3 + z5, z4 + z5)
    out[..., 7] = _descale(_chk(t4 + z1 + z3), n)
    out[..., 5] = _descale(_chk(t5 + z2 + z4), n)
    out[..., 3] = _descale(_chk(t6 + z2 + z3), n)
    out[..., 1] = _descale(_chk(t7 + z1 + z4), n)
    return out


def fdct_quant(blocks, q):
    """blocks int [n, 8, 8] samples, q [64] natural order -> int [n, 64] quantised coefficients in ZIGZAG order."""
    d = blocks.astype(np.int64) - 128
    d = _fdct_pass(d, True)                                        # rows
    d = _fdct_pass(d.transpose(0, 2, 1), False).transpose(0, 2, 1)  # columns
    c = d.reshape(-1, 64)
    div = (np.asarray(q, dtype=np.int64) << 3)[None, :]
    qc = np.sign(c) * ((np.abs(c) + (div >> 1)) // div)
    return qc[:, JW.ZIGZAG]


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)     # [bh, bw, 8, 8]


def coded_blocks(rgb, qt):
    """-> list over the coded blocks, MCU by MCU (Y00 Y01 Y10 Y11 Cb Cr): (component, zigzag coefficients [64] or None for a dummy block)."""
    H, W = rgb.shape[:2]
    g = geometry(H, W)
    py, pcb, pcr = planes(rgb)
    cy = fdct_quant(_blocks(py).reshape(-1, 8, 8), qt[0]).reshape(g['bh_y'], g['bw_y'], 64)
    ccb = fdct_quant(_blocks(pcb).reshape(-1, 8, 8), qt[1]).reshape(g['bh_c'], g['bw_c'], 64)
    ccr = fdct_quant(_blocks(pcr).reshape(-1, 8, 8), qt[1]).reshape(g['bh_c'], g['bw_c'], 64)
    out = []
    for my in range(g['mh']):
        for mx in range(g['mw']):
            for k in range(4):
                by, bx = 2 * my + (k >> 1), 2 * mx + (k & 1)
                out.append((0, cy[by, bx] if (by < g['bh_y'] and bx < g['bw_y']) else None))
            out.append((1, ccb[my, mx]))
            out.append((2, ccr[my, mx]))
    return out


_CODES = None


def _codes():
    global _CODES
    if _CODES is None:
        _CODES = [JW.huff_codes(s) for s in JW.HUFF_SPECS]        # DC lum, AC lum, DC chr, AC chr
    return _CODES


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, size):
        self.acc = (self.acc << size) | code
        self.n += size

    def finish(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, 'big') if self.n else b''
        return raw.replace(b'\xff', b'\xff\x00')


def _magnitude(v):
    a = abs(int(v))
    cat = a.bit_length()
    return cat, (int(v) if v >= 0 else int(v) - 1) & ((1 << cat) - 1)


def entropy(blocks):
    """The segment of coded_blocks' list.  A dummy block: AC all zero, DC = the DC of the block coded just before it (difference 0)."""
    codes = _codes()
    out, last = _Bits(), [0, 0, 0]
    for comp, zz in blocks:
        dc, ac = codes[0 if comp == 0 else 2], codes[1 if comp == 0 else 3]
        if zz is None:
            out.put(*dc[0])
            out.put(*ac[0x00])
            continue
        cat, bits = _magnitude(int(zz[0]) - last[comp])
        last[comp] = int(zz[0])
        out.put(*dc[cat])
        out.put(bits, cat)
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.put(*ac[0xF0])
                run -= 16
            cat, bits = _magnitude(v)
            out.put(*ac[run << 4 | cat])
            out.put(bits, cat)
            run = 0
        if run > 0:
            out.put(*ac[0x00])
    return out.finish()


def encode(frame, ids=None, ctab=None, qt=None) -> bytes:
    qt = JW.quant_tables() if qt is None else np.asarray(qt)
    return entropy(coded_blocks(blend(frame, ids, ctab), qt))


def has_zrl(rgb, qt) -> bool:
    """Does any block hold a zero run above 15 in front of a nonzero coefficient?"""
    for _, zz in coded_blocks(np.asarray(rgb), np.asarray(qt)):
        if zz is None:
            continue
        nz = np.flatnonzero(zz[1:])
        if len(nz) and (np.diff(np.concatenate(([-1], nz))) > 16).any():
            return True
    return False


class EncodeExecutor:
    """Wraps another executor (tests/mock_exec.py's interpreter on host memory) and runs PROB_TO_ID flags == 128 through the model:
    the slots of include/cutie_hip.h ABI 11."""
    is_mock = True

    def __init__(self, inner):
        self.inner = inner
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def stream(self):
        return 0

    def run(self, arr):
        from mock_exec import view, U8, I32
        import torch
        for rec in arr:
            if int(rec['kind']) == 36 and int(rec['flags']) == 128:
                i, p = [int(v) for v in rec['i']], [int(v) for v in rec['p']]
                H, W, ld, cap = i[1], i[2], i[4], i[7]
                frame = view(p[0], U8, (H, W, 3), (ld, 3, 1)).numpy()
                ids = view(p[2], U8, (H, W)).numpy() if p[2] else None
                ctab = view(p[6], U8, (256, 4)).numpy() if p[6] else None
                qt = view(p[7], U8, (256,)).numpy().view(np.uint16).reshape(2, 64)
                data = encode(frame, ids, ctab, qt)
                status = view(p[4], I32, (4,))
                fits = len(data) <= cap
                status.copy_(torch.tensor([len(data), 0, 0 if fits else 1, 0], dtype=torch.int32))
                if fits and data:
                    view(p[3], U8, (len(data),)).copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
                self.calls += 1
            else:
                self.inner.run_one(rec)
