"""Integer numpy reference of the GPU JPEG decode (cutie_amd/csrc/jpeg.hip), stage by stage, read from the same packet the kernels
read (cutie_amd/inference/data/jpeg.py).  Each stage is libjpeg's: the sequential Huffman decoder (jdhuff.c), the ISLOW IDCT
(jidctint.c) with its range-limit table (jdmaster.c), fancy upsampling (jdsample.c) and the fixed-point YCbCr -> RGB tables
(jdcolor.c).  TEST INFRASTRUCTURE ONLY.

  huff(buf)          -> (int16 [nblock, 64] coefficients, natural order, quantised, absolute DC; error bits)
  idct(buf, coef)    -> uint8 [plane bytes]: every component's plane, blocks_w * 8 wide, whole blocks
  color(buf, planes) -> uint8 [H, W, 3]
  decode(buf)        -> color(idct(huff)))"""
import numpy as np

from cutie_amd.inference.data import jpeg as J

ERR_CODE, ERR_TRUNC = 1, 2


def _hdr(buf):
    return buf[:J.HDR_WORDS * 4].view(np.int32)


def _words(buf, off, n):
    return buf[off * 4:(off + n) * 4].view(np.int32)


def _comps(buf):
    h = _hdr(buf)
    return _words(buf, int(h[J.HDR_OFF_COMP]), 3 * J.COMP_WORDS).reshape(3, J.COMP_WORDS)[:int(h[J.HDR_NCOMP])]


def lookup16(t):
    """Device table -> (length, symbol) lists indexed by the next 16 bits, as jpeg_huff_decode walks maxcode; length 0: no code."""
    w = np.arange(1 << 16, dtype=np.int64)
    ln = np.zeros(1 << 16, dtype=np.int64)
    sym = np.zeros(1 << 16, dtype=np.int64)
    maxcode, valoff = t[J.TAB_MAXCODE:J.TAB_MAXCODE + 18].astype(np.int64), t[J.TAB_VALOFF:J.TAB_VALOFF + 18].astype(np.int64)
    for length in range(1, 17):
        code = w >> (16 - length)
        hit = (ln == 0) & (code <= maxcode[length])
        ln[hit] = length
        sym[hit] = t[J.TAB_VAL + np.clip(code[hit] + valoff[length], 0, 255)]
    return ln.tolist(), sym.tolist()


def huff(buf):
    h = _hdr(buf)
    nseg, bpm, mcus_x, nmcu, ri = (int(h[k]) for k in (J.HDR_NSEG, J.HDR_BPM, J.HDR_MCUS_X, J.HDR_NMCU, J.HDR_RI))
    segs = _words(buf, int(h[J.HDR_OFF_SEG]), 4 * nseg).reshape(nseg, 4)
    comps = _comps(buf)
    mb = _words(buf, int(h[J.HDR_OFF_MB]), 4 * J.MAX_BPM).reshape(J.MAX_BPM, 4)
    tabs = _words(buf, int(h[J.HDR_OFF_HUFF]), J.TABW * int(h[J.HDR_NTAB])).reshape(-1, J.TABW)
    look = [lookup16(t) for t in tabs]
    coef = np.zeros((int(h[J.HDR_NBLOCK]), 64), dtype=np.int64)
    blocks = [tuple(int(x) for x in mb[b, :3]) for b in range(bpm)]
    zz = J.ZIGZAG.tolist()

    def out(err):
        return ((coef + 32768) % 65536 - 32768).astype(np.int16), err

    for s in range(nseg):
        off, nbytes = int(segs[s, 0]), int(segs[s, 1])
        win = np.frombuffer(bytes(buf[off:off + nbytes]) + b'\xff' * 8, dtype=np.uint8).astype(np.int64)
        win32 = ((win[:-3] << 24) | (win[1:-2] << 16) | (win[2:-1] << 8) | win[3:]).tolist()
        nbits = 8 * nbytes
        p = 0
        last = [0, 0, 0]
        for m in range(s * ri, min((s + 1) * ri, nmcu)):
            my, mx = divmod(m, mcus_x)
            for c, bh, bv in blocks:
                cw = comps[c]
                blk = coef[int(cw[J.COMP_BLK_OFF]) + (my * int(cw[J.COMP_V]) + bv) * int(cw[J.COMP_BW]) + mx * int(cw[J.COMP_H]) + bh]
                ln, sym = look[int(cw[J.COMP_DC])]
                w = (win32[p >> 3] << (p & 7)) >> 16 & 0xFFFF
                if ln[w] == 0:
                    return out(ERR_CODE)
                t = sym[w]
                p += ln[w]
                d = 0
                if t:
                    r = ((win32[p >> 3] << (p & 7)) >> (32 - t)) & ((1 << t) - 1)
                    p += t
                    d = r if r >= (1 << (t - 1)) else r - (1 << t) + 1
                last[c] += d
                blk[0] = last[c]
                ln, sym = look[int(cw[J.COMP_AC])]
                k = 1
                while k < 64:
                    w = (win32[p >> 3] << (p & 7)) >> 16 & 0xFFFF
                    if ln[w] == 0:
                        return out(ERR_CODE)
                    rs = sym[w]
                    p += ln[w]
                    r, t = rs >> 4, rs & 15
                    if t:
                        k += r
                        v = ((win32[p >> 3] << (p & 7)) >> (32 - t)) & ((1 << t) - 1)
                        p += t
                        blk[zz[min(k, 63)]] = v if v >= (1 << (t - 1)) else v - (1 << t) + 1     # (jpeg_natural_order[64..79] = 63)
                    elif r != 15:
                        break
                    else:
                        k += 15
                    k += 1
                if p > nbits:
                    return out(ERR_TRUNC)
    return out(0)


# ---- IDCT: jidctint.c jpeg_idct_islow ------------------------------------------------------------------------------------------
CONST_BITS, PASS1_BITS = 13, 2
(FIX_0_298631336, FIX_0_390180644, FIX_0_541196100, FIX_0_765366865, FIX_0_899976223, FIX_1_175875602, FIX_1_501321110,
 FIX_1_847759065, FIX_1_961570560, FIX_2_053119869, FIX_2_562915447, FIX_3_072711026) = (
    2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(x0, x1, x2, x3, x4, x5, x6, x7):
    """One ISLOW pass on int64 arrays -> its 8 outputs before descaling (scaled by 2^CONST_BITS)."""
    z1 = (x2 + x6) * FIX_0_541196100
    tmp2 = z1 + x6 * -FIX_1_847759065
    tmp3 = z1 + x2 * FIX_0_765366865
    tmp0 = (x0 + x4) << CONST_BITS
    tmp1 = (x0 - x4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * FIX_1_175875602
    t0, t1, t2, t3 = t0 * FIX_0_298631336, t1 * FIX_2_053119869, t2 * FIX_3_072711026, t3 * FIX_1_501321110
    z1, z2 = z1 * -FIX_0_899976223, z2 * -FIX_2_562915447
    z3, z4 = z3 * -FIX_1_961570560 + z5, z4 * -FIX_0_390180644 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]


def range_limit(x):
    """libjpeg's IDCT output table: entry x & 1023 of sample_range_limit + CENTERJSAMPLE (the 10-bit wrap included)."""
    u = (x + 128) & 1023
    return np.where(u < 256, u, np.where(u < 640, 255, 0)).astype(np.uint8)


def idct_blocks(coef, quant):
    """int16 [n, 64] natural order, quant [64] natural order -> uint8 [n, 8, 8]; DEQUANTIZE in int as libjpeg does."""
    d = coef.astype(np.int64).reshape(-1, 8, 8) * quant.astype(np.int64).reshape(1, 8, 8)
    cols = _idct_1d(*(d[:, k, :] for k in range(8)))              # pass 1: columns -> workspace rows
    ws = np.stack([_descale(v, CONST_BITS - PASS1_BITS) for v in cols], axis=1)
    ws = (ws + 2 ** 31) % 2 ** 32 - 2 ** 31                       # (int workspace)
    rows = _idct_1d(*(ws[:, :, k] for k in range(8)))             # pass 2: rows
    return np.stack([range_limit(_descale(v, CONST_BITS + PASS1_BITS + 3)) for v in rows], axis=2)


def idct(buf, coef):
    h = _hdr(buf)
    comps = _comps(buf)
    nf = int(h[J.HDR_NCOMP])
    quant = _words(buf, int(h[J.HDR_OFF_Q]), 64 * nf).reshape(nf, 64)
    planes = np.zeros(int(h[J.HDR_PLANE_BYTES]), dtype=np.uint8)
    for c in range(nf):
        cw = comps[c]
        bw, bh, off = int(cw[J.COMP_BW]), int(cw[J.COMP_BH]), int(cw[J.COMP_BLK_OFF])
        blk = idct_blocks(coef[off:off + bw * bh], quant[c])
        plane = blk.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(-1)
        po = int(cw[J.COMP_PLANE_OFF])
        planes[po:po + plane.size] = plane
    return planes


# ---- upsampling (jdsample.c) and colour conversion (jdcolor.c) --------------------------------------------------------------------
def _plane(buf, planes, c):
    cw = _comps(buf)[c]
    po, pw, bh = int(cw[J.COMP_PLANE_OFF]), int(cw[J.COMP_PLANE_W]), int(cw[J.COMP_BH])
    return planes[po:po + pw * bh * 8].reshape(bh * 8, pw).astype(np.int64)


def upsample(buf, planes, c, H, W):
    """Chroma plane c -> int [H, W] as libjpeg's upsampler: fancy h1v2, fancy h2v1 / h2v2 where the downsampled width is > 2, else
    replication.  Neighbour rows and columns past the downsampled extent repeat its edge."""
    h = _hdr(buf)
    hmax, vmax = int(h[J.HDR_HMAX]), int(h[J.HDR_VMAX])
    cw = _comps(buf)[c]
    dw, dh = int(cw[J.COMP_DW]), int(cw[J.COMP_DH])
    p = _plane(buf, planes, c)
    y, x = np.arange(H), np.arange(W)
    if hmax == 1 and vmax == 1:
        return p[:H, :W]
    fancy = dw > 2 or hmax == 1                          # (h1v2 is fancy at any width)
    j, i = (y >> 1) if vmax == 2 else y, (x >> 1) if hmax == 2 else x
    if not fancy:
        return p[j][:, i]
    if vmax == 1:                                        # h2v1
        c0, left, right = p[j][:, i], p[j][:, np.maximum(i - 1, 0)], p[j][:, np.minimum(i + 1, dw - 1)]
        even = np.where(i == 0, c0, (3 * c0 + left + 1) >> 2)
        odd = np.where(i == dw - 1, c0, (3 * c0 + right + 2) >> 2)
        return np.where((x & 1) == 0, even, odd)
    nb = np.where((y & 1) == 0, np.maximum(j - 1, 0), np.minimum(j + 1, dh - 1))
    if hmax == 1:                                        # h1v2
        bias = np.where((y & 1) == 0, 1, 2)[:, None]
        return (3 * p[j][:, i] + p[nb][:, i] + bias) >> 2
    cs = 3 * p[j] + p[nb]                                # h2v2: column sums
    this, prev, nxt = cs[:, i], cs[:, np.maximum(i - 1, 0)], cs[:, np.minimum(i + 1, dw - 1)]
    even = np.where(i == 0, (this * 4 + 8) >> 4, (3 * this + prev + 8) >> 4)
    odd = np.where(i == dw - 1, (this * 4 + 7) >> 4, (3 * this + nxt + 7) >> 4)
    return np.where((x & 1) == 0, even, odd)


def color(buf, planes):
    h = _hdr(buf)
    H, W, nf = int(h[J.HDR_H]), int(h[J.HDR_W]), int(h[J.HDR_NCOMP])
    Y = _plane(buf, planes, 0)[:H, :W]
    if nf == 1:
        return np.repeat(Y.astype(np.uint8)[:, :, None], 3, axis=2)
    cb = upsample(buf, planes, 1, H, W) - 128
    cr = upsample(buf, planes, 2, H, W) - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(buf):
    coef, err = huff(buf)
    if err:
        raise ValueError(f'jpeg_ref: error bits {err}')
    return color(buf, idct(buf, coef))
