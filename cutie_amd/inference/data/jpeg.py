"""Host side of the GPU JPEG decode (ingest='device-decode'): parse the markers of a baseline Huffman JPEG and pack what the three
decode stages of RESIZE (include/cutie_hip.h, ABI 6: flags 8 / 16 / 32; kernels in cutie_amd/csrc/jpeg.hip) read into ONE uint8
packet that is uploaded as it is.

Supported: SOF0 / SOF1 with 8-bit samples, one scan holding every component, 1 component (PIL mode 'L', replicated to RGB as
``.convert('RGB')`` does) or 3 YCbCr components interleaved with luma sampling 1x1, 2x1, 1x2 or 2x2 and chroma 1x1, optional restart
intervals.  Everything else -- progressive, arithmetic, lossless, 12-bit, CMYK / YCCK, Adobe transform 0 (RGB), multiple scans, other
sampling factors, files that are not JPEG -- makes ``parse`` return (None, reason); the caller then decodes on the host.

Packet layout (int32 words unless stated; offsets in the header):
  header [64]   HDR_* below
  segments      [nseg][4]: byte offset of the destuffed entropy data in the packet, its byte length, first chunk, chunk count
  chunk->seg    [nchunks]
  components    [3][16]: COMP_* below
  MCU blocks    [10][4]: component, horizontal and vertical block offset inside the MCU, 0
  quant         [ncomp][64]: natural order
  huffman       [ntab][TABW]: FAST (2^FASTBITS entries len << 8 | symbol, 0 = longer code), MAXCODE[18], VALOFF[18], HUFFVAL[256]
  data          the segments' destuffed bytes, each padded with 0xff to a multiple of 4 bytes plus 8 more
A segment is the entropy-coded data between two restart markers; it is cut into chunks of ``chunk_bits`` bits, one GPU thread each."""
import threading
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np

MAGIC = 0x3147504A                    # 'JPG1'
HDR_WORDS = 64
(HDR_MAGIC, HDR_H, HDR_W, HDR_NCOMP, HDR_BPM, HDR_MCUS_X, HDR_NMCU, HDR_RI, HDR_NSEG, HDR_NCHUNK, HDR_CHUNK_BITS, HDR_NBLOCK,
 HDR_HMAX, HDR_VMAX, HDR_PLANE_BYTES, HDR_OFF_SEG, HDR_OFF_C2S, HDR_OFF_COMP, HDR_OFF_MB, HDR_OFF_Q, HDR_OFF_HUFF, HDR_OFF_DATA,
 HDR_BYTES, HDR_NTAB) = range(24)
COMP_WORDS = 16
(COMP_H, COMP_V, COMP_BW, COMP_BH, COMP_BLK_OFF, COMP_PLANE_OFF, COMP_PLANE_W, COMP_DW, COMP_DH, COMP_DC, COMP_AC) = range(11)
MAX_BPM = 10
FASTBITS = 9
TAB_FAST, TAB_MAXCODE, TAB_VALOFF, TAB_VAL = 0, 1 << FASTBITS, (1 << FASTBITS) + 18, (1 << FASTBITS) + 36
TABW = TAB_VAL + 256
CHUNK_BITS = 1024

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63], dtype=np.int32)          # zigzag index -> natural index

HUFF_CACHE_SIZE = 256                 # tables kept (least recently used out): files with optimised tables bring their own per frame
_huff_cache: 'OrderedDict[bytes, np.ndarray]' = OrderedDict()
_huff_lock = threading.Lock()


def huff_table(counts: bytes, values: bytes, dc: bool = False) -> Optional[np.ndarray]:
    """DHT payload (16 code-length counts, the symbols) -> int32 [TABW] device table, cached by its bytes; None where libjpeg's
    jpeg_make_d_derived_tbl refuses the table (a code of all ones or beyond, a DC symbol above 15)."""
    key = (b'D' if dc else b'A') + bytes(counts) + bytes(values)
    with _huff_lock:
        t = _huff_cache.get(key)
        if t is not None:
            _huff_cache.move_to_end(key)
            return t
    if dc and any(v > 15 for v in values):
        return None
    t = np.zeros(TABW, dtype=np.int32)
    maxcode = np.full(18, -1, dtype=np.int64)
    maxcode[17] = 0x7FFFFFFF
    valoff = np.zeros(18, dtype=np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n:
            valoff[length] = k - code
            for _ in range(n):
                if length <= FASTBITS:
                    lo = code << (FASTBITS - length)
                    t[TAB_FAST + lo:TAB_FAST + lo + (1 << (FASTBITS - length))] = (length << 8) | values[k]
                code += 1
                k += 1
            maxcode[length] = code - 1
        if code >= (1 << length):
            return None
        code <<= 1
    t[TAB_MAXCODE:TAB_MAXCODE + 18] = maxcode
    t[TAB_VALOFF:TAB_VALOFF + 18] = valoff
    t[TAB_VAL:TAB_VAL + len(values)] = np.frombuffer(bytes(values), dtype=np.uint8)
    with _huff_lock:
        _huff_cache[key] = t
        while len(_huff_cache) > HUFF_CACHE_SIZE:
            _huff_cache.popitem(last=False)
    return t


class Packet:
    """A parsed frame: ``buf`` is the uint8 packet (module docstring), ``hdr`` its header words, ``source`` the file it came from
    ('' for bytes)."""
    __slots__ = ('buf', 'hdr', 'shape', 'source')

    def __init__(self, buf: np.ndarray, source: str = ''):
        self.buf = buf
        self.source = source
        self.hdr = buf[:HDR_WORDS * 4].view(np.int32)
        self.shape = (int(self.hdr[HDR_H]), int(self.hdr[HDR_W]))

    def words(self, off, n):
        return self.buf[off * 4:(off + n) * 4].view(np.int32)


def _u16(b, o):
    return (b[o] << 8) | b[o + 1]


def parse(data: bytes, chunk_bits: int = CHUNK_BITS) -> Tuple[Optional[Packet], str]:
    """JPEG file bytes -> (Packet, '') or (None, reason) for anything the GPU decoder does not take (module docstring)."""
    b = data
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        return None, 'not a JPEG'
    q, dc, ac = {}, {}, {}
    frame = None
    ri = 0
    jfif = False
    adobe = None
    o = 2
    while True:
        while o < n and b[o] != 0xFF:
            o += 1                                     # (garbage between markers: libjpeg skips it with a warning)
        while o < n and b[o] == 0xFF:
            o += 1
        if o >= n:
            return None, 'no scan'
        m = b[o]
        o += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            return None, 'no scan'
        if o + 2 > n:
            return None, 'truncated header'
        L = _u16(b, o)
        seg = b[o + 2:o + L]
        if L < 2 or len(seg) != L - 2:
            return None, 'truncated header'
        o += L
        if m == 0xDB:                                  # DQT
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or p + 1 + size > len(seg):
                    return None, 'bad DQT'
                raw = np.frombuffer(seg[p + 1:p + 1 + size], dtype='>u2' if pq else np.uint8).astype(np.int32)
                nat = np.zeros(64, dtype=np.int32)
                nat[ZIGZAG] = raw
                q[tq] = nat
                p += 1 + size
        elif m == 0xC4:                                # DHT
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    return None, 'bad DHT'
                tc, th = seg[p] >> 4, seg[p] & 15
                counts = seg[p + 1:p + 17]
                nv = sum(counts)
                if tc > 1 or th > 3 or nv > 256 or p + 17 + nv > len(seg):
                    return None, 'bad DHT'
                t = huff_table(counts, seg[p + 17:p + 17 + nv], dc=tc == 0)
                if t is None:
                    return None, 'bad DHT'
                (ac if tc else dc)[th] = t
                p += 17 + nv
        elif m in (0xC0, 0xC1):                        # SOF0 / SOF1
            if frame is not None:
                return None, 'multiple frames'
            if len(seg) < 6 or seg[0] != 8:
                return None, f'{seg[0] if seg else "?"}-bit samples'
            H, W, nf = _u16(seg, 1), _u16(seg, 3), seg[5]
            if len(seg) < 6 + 3 * nf:
                return None, 'bad SOF'
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(nf)]
            frame = (H, W, comps)
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None, {0xC2: 'progressive', 0xC3: 'lossless'}.get(m, 'arithmetic' if m >= 0xC9 else 'hierarchical')
        elif m == 0xCC:
            return None, 'arithmetic'
        elif m == 0xDD:                                # DRI
            if len(seg) < 2:
                return None, 'bad DRI'
            ri = _u16(seg, 0)
        elif m == 0xE0 and seg[:5] == b'JFIF\x00':
            jfif = True
        elif m == 0xEE and seg[:5] == b'Adobe' and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:                                # SOS: the scan runs to the next marker that is not RST / stuffing
            if frame is None:
                return None, 'no frame header'
            segs, end = _entropy_segments(b, o)
            i = end
            while i < n and b[i] == 0xFF:
                i += 1
            if i < n and b[i] != 0xD9:
                return None, 'multiple scans'
            return _pack(frame, seg, q, dc, ac, ri, jfif, adobe, segs, chunk_bits)
        elif m in (0xDC, 0xDE, 0xDF):
            return None, 'DNL / hierarchical'
        # APPn, COM, anything else with a length: skipped


def _entropy_segments(b, o):
    """The scan from byte o: -> (its segments between restart markers, destuffed, as uint8 arrays; the offset of the marker that
    ends it, or len(b)).  One vectorised pass over the 0xff bytes finds the end, the RST markers and the stuffed zeros."""
    a = np.frombuffer(b, dtype=np.uint8, offset=o)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nb = a[ff + 1]
    rst = (nb >= 0xD0) & (nb <= 0xD7)
    stop = np.flatnonzero((nb != 0) & ~rst)
    end = int(ff[stop[0]]) if len(stop) else len(a)
    keep = ff < end
    ff, nb, rst = ff[keep], nb[keep], rst[keep]
    cuts = ff[rst]
    stuffed = ff[nb == 0] + 1
    starts = np.concatenate(([0], cuts + 2))
    ends = np.concatenate((cuts, [end]))
    data = np.delete(a[:end], stuffed) if len(stuffed) else a[:end]
    # positions after destuffing: subtract the stuffed bytes in front
    s2 = starts - np.searchsorted(stuffed, starts)
    e2 = ends - np.searchsorted(stuffed, ends)
    return [data[s:e] for s, e in zip(s2.tolist(), e2.tolist())], o + end


def _pack(frame, sos, q, dc, ac, ri, jfif, adobe, segs, chunk_bits):
    H, W, comps = frame
    nf = len(comps)
    if H < 1 or W < 1:
        return None, 'empty frame'
    if nf == 4:
        return None, 'CMYK / YCCK'
    if nf not in (1, 3):
        return None, f'{nf} components'
    if nf == 3:
        if adobe == 0:
            return None, 'Adobe transform 0 (RGB)'
        if not jfif and adobe is None and tuple(c[0] for c in comps) == (82, 71, 66):
            return None, 'RGB component ids'
    if len(sos) < 1 or sos[0] != nf or len(sos) < 4 + 2 * nf:
        return None, 'multiple scans'
    ss, se, ahl = sos[1 + 2 * nf], sos[2 + 2 * nf], sos[3 + 2 * nf]
    if (ss, se, ahl) != (0, 63, 0):
        return None, 'not a sequential scan'
    tabsel = {}
    for k in range(nf):
        cid, t = sos[1 + 2 * k], sos[2 + 2 * k]
        tabsel[cid] = (t >> 4, t & 15)
    if set(tabsel) != {c[0] for c in comps}:
        return None, 'scan components'
    if nf == 1:
        samp = [(1, 1)]
    else:
        samp = [(c[1], c[2]) for c in comps]
        if samp[0] not in ((1, 1), (2, 1), (1, 2), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            return None, 'sampling ' + 'x'.join(f'{h}{v}' for h, v in samp)
    hmax, vmax = samp[0]
    tabs, tab_index = [], {}

    def tab(t):
        k = id(t)
        if k not in tab_index:
            tab_index[k] = len(tabs)
            tabs.append(t)
        return tab_index[k]

    comp_words = np.zeros((3, COMP_WORDS), dtype=np.int32)
    quant = []
    mb = np.zeros((MAX_BPM, 4), dtype=np.int32)
    if nf == 1:
        mcus_x, mcus_y = -(-W // 8), -(-H // 8)
    else:
        mcus_x, mcus_y = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    nmcu = mcus_x * mcus_y
    blk_off, plane_off, bpm = 0, 0, 0
    for k, (cid, _, _, tq) in enumerate(comps):
        hc, vc = samp[k]
        td, ta = tabsel[cid]
        if tq not in q or td not in dc or ta not in ac:
            return None, 'missing table'
        bw, bh = mcus_x * hc, mcus_y * vc
        cw = comp_words[k]
        cw[COMP_H], cw[COMP_V], cw[COMP_BW], cw[COMP_BH] = hc, vc, bw, bh
        cw[COMP_BLK_OFF], cw[COMP_PLANE_OFF], cw[COMP_PLANE_W] = blk_off, plane_off, bw * 8
        cw[COMP_DW], cw[COMP_DH] = -(-W * hc // hmax), -(-H * vc // vmax)
        cw[COMP_DC], cw[COMP_AC] = tab(dc[td]), tab(ac[ta])
        quant.append(q[tq])
        for v in range(vc):
            for h in range(hc):
                mb[bpm] = (k, h, v, 0)
                bpm += 1
        blk_off += bw * bh
        plane_off += bw * bh * 64
    mpr = nmcu if ri == 0 else ri
    nseg = -(-nmcu // mpr)
    if not ri and len(segs) > 1:
        return None, 'restart markers without an interval'
    if len(segs) > nseg and not any(len(s) for s in segs[nseg:]):
        segs = segs[:nseg]                               # (an RST right before EOI)
    if len(segs) != nseg:
        return None, f'{len(segs)} restart segments for {nseg}'

    seg_words = np.zeros((nseg, 4), dtype=np.int32)
    chunks = [max(1, -(-8 * len(s) // chunk_bits)) for s in segs]
    nchunk = sum(chunks)
    off_seg = HDR_WORDS
    off_c2s = off_seg + 4 * nseg
    off_comp = off_c2s + nchunk
    off_mb = off_comp + 3 * COMP_WORDS
    off_q = off_mb + 4 * MAX_BPM
    off_huff = off_q + 64 * nf
    off_data = 4 * (off_huff + TABW * len(tabs))
    padded = [(len(s) + 3) // 4 * 4 + 8 for s in segs]
    total = off_data + sum(padded)
    buf = np.empty(total, dtype=np.uint8)
    words = buf[:off_data].view(np.int32)
    words[:] = 0
    hdr = words[:HDR_WORDS]
    hdr[:24] = (MAGIC, H, W, nf, bpm, mcus_x, nmcu, mpr, nseg, nchunk, chunk_bits, blk_off, hmax, vmax, plane_off, off_seg, off_c2s,
                off_comp, off_mb, off_q, off_huff, off_data, total, len(tabs))
    c2s = words[off_c2s:off_c2s + nchunk]
    pos, first = off_data, 0
    for k, s in enumerate(segs):
        seg_words[k] = (pos, len(s), first, chunks[k])
        c2s[first:first + chunks[k]] = k
        buf[pos:pos + len(s)] = s
        buf[pos + len(s):pos + padded[k]] = 0xFF
        pos += padded[k]
        first += chunks[k]
    words[off_seg:off_c2s] = seg_words.reshape(-1)
    words[off_comp:off_mb] = comp_words.reshape(-1)
    words[off_mb:off_q] = mb.reshape(-1)
    words[off_q:off_huff] = np.concatenate(quant)
    if tabs:
        words[off_huff:off_huff + TABW * len(tabs)] = np.concatenate(tabs)
    return Packet(buf), ''


def parse_file(path: str, chunk_bits: int = CHUNK_BITS) -> Tuple[Optional[Packet], str]:
    with open(path, 'rb') as fh:
        pkt, why = parse(fh.read(), chunk_bits)
    if pkt is not None:
        pkt.source = path
    return pkt, why


def stage_sizes(pkt: Packet, rounds: int) -> Dict[str, int]:
    """Element counts of the decode buffers of a packet: ``coef`` int16, ``planes`` uint8, ``work`` int32 (the Huffman stage's
    chunk exits, block counts and DC sums with their scans, per-round flags), ``rgb`` uint8 [H, W, 3]."""
    h = pkt.hdr
    return {'coef': int(h[HDR_NBLOCK]) * 64, 'planes': int(h[HDR_PLANE_BYTES]),
            'work': work_words(int(h[HDR_NCHUNK]), int(h[HDR_NSEG]), rounds), 'rgb': int(h[HDR_H]) * int(h[HDR_W]) * 3}


def work_words(nchunk: int, nseg: int, rounds: int) -> int:
    return 10 * nchunk + (rounds + 1) * nseg
