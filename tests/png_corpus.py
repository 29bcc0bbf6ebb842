"""The files of the PNG decode tests (test_png_decode_cpu.py, test_gpu_png_decode.py), generated -- no binaries are committed for them.
One shape per thing that can go wrong in the inflate and unfilter stages (cutie_amd/csrc/png_dec.hip), each below 64 KB inflated unless it
says otherwise; the expected pixels are always PIL's, ``np.array(Image.open(file))``.

    accepted(golden)  -> [(name, file bytes)]               every one is an accepted format: the parser must take it (fallback count 0)
    declined()        -> [(name, file bytes, reason)]       formats the parser hands back to PIL
    corrupt()         -> [(name, file bytes, error bit)]    valid containers (right CRCs) around bad streams: the device reports the bit
"""
import glob
import io
import os
import struct
import zlib

import numpy as np
from PIL import Image

from cutie_amd.inference.utils import png as png_container

import png_dec_ref as R
import png_ref

SIG = b'\x89PNG\r\n\x1a\n'


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def png_file(W, H, depth, ctype, stream, split=None, interlace=0, extra=()):
    """A PNG around a finished zlib stream; split: the IDAT chunk size; extra: chunks between IHDR and PLTE."""
    parts = [SIG, chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, ctype, 0, 0, interlace))] + list(extra)
    if ctype == 3:
        parts.append(chunk(b'PLTE', bytes(range(48)) * 16))
    step = split or max(len(stream), 1)
    parts += [chunk(b'IDAT', stream[o:o + step]) for o in range(0, max(len(stream), 1), step)]
    return b''.join(parts + [chunk(b'IEND', b'')])


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=None, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush_every is None:
        return c.compress(data) + c.flush()
    out = b''
    for o in range(0, len(data), flush_every):
        out += c.compress(data[o:o + flush_every]) + c.flush(flush)
    return out + c.flush()


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(rows, bpp, schedule):
    """The hand-written encoder: rows uint8 [H, rowbytes] (packed bytes) -> the filtered bytes, row y with filter schedule[y % len]."""
    H, rb = rows.shape
    out = bytearray()
    prev = np.zeros(rb, dtype=np.int64)
    for y in range(H):
        cur = rows[y].astype(np.int64)
        ft = schedule[y % len(schedule)]
        zero = np.zeros(min(bpp, rb), dtype=np.int64)
        a, c = np.concatenate([zero, cur[:rb - len(zero)]]), np.concatenate([zero, prev[:rb - len(zero)]])
        if ft == 0:
            pred = np.zeros(rb, dtype=np.int64)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) >> 1
        else:
            pred = np.array([paeth(int(a[i]), int(prev[i]), int(c[i])) for i in range(rb)], dtype=np.int64)
        out.append(ft)
        out += bytes(((cur - pred) & 255).astype(np.uint8))
        prev = cur
    return bytes(out)


def pack(ids, depth):
    """uint8 [H, W] of values < 2^depth -> the packed rows [H, ceil(W depth / 8)], MSB first."""
    H, W = ids.shape
    rb = (W * depth + 7) // 8
    out = np.zeros((H, rb), dtype=np.uint8)
    for x in range(W):
        bit = x * depth
        out[:, bit >> 3] |= (ids[:, x] << (8 - depth - (bit & 7))).astype(np.uint8)
    return out


def mask(H, W, seed, objects=3):
    """A mask-like plane: a few rectangles of ids over background."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), dtype=np.uint8)
    for k in range(1, objects + 1):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = k
    return m


def raw8(ids):
    """Filter 0 in front of every row of an 8-bit plane [H, W] or [H, W, 3]."""
    H = ids.shape[0]
    return filter_rows(ids.reshape(H, -1), 1, [0])


class FixedBits:
    """A DEFLATE bit writer with the fixed codes (RFC 1951 3.2.6), for the streams zlib will not write."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, k):
        self.v |= v << self.n
        self.n += k

    def code(self, v, k):                      # Huffman codes go MSB first
        self.put(int(format(v, f'0{k}b')[::-1], 2), k)

    def lit(self, s):                          # literal / length symbol
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, ln, dist):
        k = max(i for i in range(29) if R.LBASE[i] <= ln)
        self.lit(257 + k)
        self.put(ln - R.LBASE[k], R.LEXT[k])
        d = max(i for i in range(30) if R.DBASE[i] <= dist)
        self.code(d, 5)
        self.put(dist - R.DBASE[d], R.DEXT[d])

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, 'little')


def zwrap(body, data):
    return b'\x78\x9c' + body + struct.pack('>I', zlib.adler32(data) & 0xffffffff)


def far_window():
    """Stored block of 32768 bytes, then its copy as matches of distance 32768 (zlib's own deflate stops 262 short of that)."""
    rng = np.random.default_rng(7)
    rows = rng.integers(0, 256, (128, 256), dtype=np.uint8)
    rows[:, 0] = 0                                         # the filter bytes
    block = rows.tobytes()
    b = FixedBits()
    b.put(0, 3)                                            # not final, stored
    b.align()
    head = b.bytes() + struct.pack('<HH', 32768, 32767) + block
    b = FixedBits()
    b.put(3, 3)                                            # final, fixed
    for ln in [258] * 126 + [130, 130]:                    # 32768 bytes
        b.match(ln, 32768)
    b.lit(256)
    return png_file(255, 256, 8, 0, zwrap(head + b.bytes(), block + block))


def dynamic_block(data, dist_lens, use_matches, bad_distance=False):
    """A final dynamic block (RFC 1951 3.2.7) written by hand, for the code tables zlib never writes.  Literal/length code: symbols 0 .. 253
    at 8 bits, 254 .. 257 at 9 (complete); code-length code: symbols 0 .. 15 at 4 bits each, no repeat codes.  ``dist_lens``: the lengths of
    the HDIST distance codes -- [1] is ONE code of length 1 (an incomplete code, allowed), [0] none at all.  use_matches: every run of
    four equal bytes becomes literal + match(3, distance 1) with distance code '0'; bad_distance: the first match uses the bit pattern
    of the missing code instead."""
    lit_lens = [8] * 254 + [9] * 4
    codes, code = {}, 0
    for ln in (8, 9):
        code <<= 1 if ln == 9 else 0
        for sym, v in enumerate(lit_lens):
            if v == ln:
                codes[sym] = (code, ln)
                code += 1
    b = FixedBits()
    b.put(0b101, 3)                                       # final, dynamic
    b.put(len(lit_lens) - 257, 5); b.put(len(dist_lens) - 1, 5); b.put(19 - 4, 4)
    for sym in R.ORDER:
        b.put(4 if sym < 16 else 0, 3)
    for v in lit_lens + list(dist_lens):
        b.code(v, 4)                                      # the code-length code is the identity on 4 bits
    k, first = 0, True
    while k < len(data):
        b.code(*codes[data[k]])
        if use_matches and k + 3 < len(data) and data[k + 1] == data[k + 2] == data[k + 3] == data[k]:
            b.code(*codes[257])                           # length 3, no extra bits
            b.put(1 if (bad_distance and first) else 0, 1)
            first = False
            k += 4
        else:
            k += 1
    b.code(*codes[256])
    return zwrap(b.bytes(), bytes(data)) + (bytes(8) if bad_distance else b'')


def _table_rows():
    """4 rows of filter byte 0 + 7 pixels: runs of four equal bytes, so that dynamic_block can use matches of distance 1."""
    return bytes([0, 5, 5, 5, 5, 9, 9, 9, 0, 9, 7, 7, 7, 7, 1, 2, 0, 0, 0, 0, 3, 3, 3, 3, 0, 4, 6, 6, 6, 6, 8, 250])


def interlaced_file(ids):
    """A real Adam7 palette PNG of uint8 [H, W]: PIL reads it, the parser declines it."""
    H, W = ids.shape
    raw = b''
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        part = ids[y0::dy, x0::dx]
        if part.size:
            raw += raw8(np.ascontiguousarray(part))
    return png_file(W, H, 8, 3, deflate(raw), interlace=1)


def accepted(golden=None):
    rng = np.random.default_rng(2024)
    files = []

    def add(name, data):
        files.append((name, data))

    def pil(name, arr, mode, colours=256, **kw):
        im = Image.frombytes(mode, (arr.shape[1], arr.shape[0]), np.ascontiguousarray(arr).tobytes())
        if mode == 'P':
            im.putpalette((bytes(range(48)) * 16)[:3 * colours])
        f = io.BytesIO()
        im.save(f, format='PNG', **kw)
        add(name, f.getvalue())

    m = mask(50, 40, 1)
    noise = rng.integers(0, 256, (30, 20), dtype=np.uint8)
    # ---- deflate ----
    add('stored_small', png_file(20, 30, 8, 0, deflate(raw8(noise), 0)))
    big = rng.integers(0, 256, (300, 300), dtype=np.uint8)
    pil('stored_noise_300_two_idat', big, 'L', compress_level=0)                  # > 65535 bytes: several stored blocks (90 KB inflated)
    add('fixed', png_file(40, 50, 8, 3, deflate(raw8(m), 6, zlib.Z_FIXED)))
    add('dynamic_default', png_file(40, 50, 8, 3, deflate(raw8(m), 6)))
    add('dynamic_noise', png_file(20, 30, 8, 0, deflate(raw8(noise), 9)))
    add('huffman_only', png_file(20, 30, 8, 0, deflate(raw8(noise), 6, zlib.Z_HUFFMAN_ONLY)))
    add('filtered', png_file(40, 50, 8, 3, deflate(raw8(m), 6, zlib.Z_FILTERED)))
    for H, W in ((1, 600), (600, 1)):
        add(f'rle_constant_{H}x{W}', png_file(W, H, 8, 0, deflate(raw8(np.full((H, W), 7, dtype=np.uint8)), 6, zlib.Z_RLE)))
    runs = np.repeat(rng.integers(0, 256, 400, dtype=np.uint8), rng.integers(1, 40, 400))[:6000].reshape(60, 100)
    add('rle_runs_two_distance_codes', png_file(100, 60, 8, 0, deflate(raw8(runs), 6, zlib.Z_RLE)))
    add('one_symbol', png_file(64, 33, 8, 0, deflate(bytes(33 * 65), 6, zlib.Z_HUFFMAN_ONLY)))
    # code tables zlib's deflate never writes (it always sends two distance codes): ONE distance code of length 1, and none at all
    add('single_distance_code', png_file(7, 4, 8, 0, dynamic_block(_table_rows(), [1], True)))
    add('empty_distance_code', png_file(7, 4, 8, 0, dynamic_block(_table_rows(), [0], False)))
    for nm, fl in (('full', zlib.Z_FULL_FLUSH), ('sync', zlib.Z_SYNC_FLUSH)):
        for k in (1, 7):
            add(f'flush_{nm}_every_{k}_rows', png_file(40, 50, 8, 3, deflate(raw8(m), 6, flush_every=41 * k, flush=fl)))
    add('far_window_32768', far_window())
    blk = rng.integers(0, 256, (127, 256), dtype=np.uint8)
    blk[:, 0] = 0
    add('far_window_zlib', png_file(255, 254, 8, 0, deflate(blk.tobytes() * 2, 9)))
    small = rng.integers(0, 256, (4, 50), dtype=np.uint8)
    small[:, 0] = 0
    add('short_window_wbits9', png_file(49, 40, 8, 0, deflate(small.tobytes() * 10, 9, wbits=9)))
    stream = deflate(raw8(mask(70, 131, 3)), 6)
    for cut in (1, 2, 7, 8192):
        add(f'idat_split_{cut}', png_file(131, 70, 8, 3, stream, split=cut))
    # ---- unfilter ----
    for ch, ctype in ((1, 0), (3, 2)):
        for ft in range(5):
            for H, W in ((9, 131), (2, 65)):
                px = rng.integers(0, 256, (H, W * ch), dtype=np.uint8)
                add(f'filter{ft}_bpp{ch}_{H}x{W}', png_file(W, H, 8, ctype, deflate(filter_rows(px, ch, [ft]))))
        for H, W in ((1, 1), (70, 1), (2, 63), (70, 64), (1, 65), (70, 131)):
            px = np.repeat(rng.integers(0, 256, (H, -(-W * ch // 4)), dtype=np.uint8), 4, axis=1)[:, :W * ch]
            add(f'filter_mixed_bpp{ch}_{H}x{W}', png_file(W, H, 8, ctype, deflate(filter_rows(px, ch, [4, 1, 0, 3, 2, 2, 4, 1, 3]))))
    for depth in (1, 2, 4):
        for W in (1, 7, 9, 131):
            ids = rng.integers(0, 1 << depth, (5, W), dtype=np.uint8)
            add(f'packed_{depth}bit_w{W}', png_file(W, 5, depth, 3, deflate(filter_rows(pack(ids, depth), 1, [0, 1, 2, 3, 4]))))
            pil(f'pil_{depth}bit_w{W}', ids, 'P', bits=depth)
    pil('pil_default_3_colours', mask(70, 131, 5, objects=2), 'P', colours=3)                  # PIL packs it at 2 bits
    pil('pil_default_8bit', (mask(70, 131, 6, objects=3) * 40).astype(np.uint8), 'P')
    pil('pil_rgb', rng.integers(0, 256, (20, 33, 3), dtype=np.uint8), 'RGB')
    pil('pil_grey', mask(20, 33, 8) * 60, 'L')
    # ---- the project's own device-written stream (tests/png_ref.py = the bytes of csrc/png.hip) ----
    ids = mask(96, 136, 11)
    own, _ = png_ref.encode(ids)
    add('own_device_stream', png_container.assemble(bytes(own), 96, 136, bytes(range(48)) * 16))
    # ---- real files ----
    if golden is not None:
        pats = ('judo/*.png', 'bike/00000.png', 'io/video/Annotations*/v/*.png')
        for pat in pats:
            for f in sorted(glob.glob(os.path.join(golden, pat))):
                add('golden/' + os.path.relpath(f, golden), open(f, 'rb').read())
    return files


def declined():
    rng = np.random.default_rng(5)
    out = []

    def pil(arr, mode):
        f = io.BytesIO()
        Image.frombytes(mode, (arr.shape[1], arr.shape[0]), np.ascontiguousarray(arr).tobytes()).save(f, format='PNG')
        return f.getvalue()

    good = png_file(40, 50, 8, 3, deflate(raw8(mask(50, 40, 1))))
    out.append(('interlaced', png_file(40, 50, 8, 3, deflate(raw8(mask(50, 40, 1))), interlace=1), 'interlaced'))
    out.append(('16bit', pil(rng.integers(0, 65536, (8, 9)).astype(np.uint16), 'I;16'), '16 bits'))
    out.append(('rgba', pil(rng.integers(0, 256, (8, 9, 4), dtype=np.uint8), 'RGBA'), 'alpha'))
    out.append(('la', pil(rng.integers(0, 256, (8, 9, 2), dtype=np.uint8), 'LA'), 'alpha'))
    out.append(('grey4', png_file(9, 8, 4, 0, deflate(bytes(8 * 6))), 'grey below 8 bits'))
    bad = bytearray(good)
    bad[good.index(b'IDAT') + 6] ^= 0x10
    out.append(('bad_crc', bytes(bad), 'bad CRC'))
    out.append(('no_idat', b''.join([SIG, chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 4, 8, 0, 0, 0, 0)), chunk(b'IEND', b'')]), 'no IDAT'))
    out.append(('zlib_cm', png_file(4, 4, 8, 0, b'\x79\x9c' + deflate(bytes(20))[2:]), 'bad zlib header'))
    out.append(('zlib_fdict', png_file(4, 4, 8, 0, b'\x78\xbb' + deflate(bytes(20))[2:]), 'bad zlib header'))
    out.append(('zlib_fcheck', png_file(4, 4, 8, 0, b'\x78\x9d' + deflate(bytes(20))[2:]), 'bad zlib header'))
    return out


def corrupt():
    ids = mask(50, 40, 1)
    raw = raw8(ids)
    good = deflate(raw, 6)
    out = []

    def add(name, stream, bit, H=50):
        out.append((name, png_file(40, H, 8, 3, stream), bit))

    add('cut_quarter', good[:len(good) // 4], R.E_EOF)
    add('cut_half', good[:len(good) // 2], R.E_EOF)
    add('cut_last_byte', good[:-1], R.E_EOF)
    flipped = bytearray(good)
    flipped[-2] ^= 1
    add('adler_flipped', bytes(flipped), R.E_ADLER)
    add('block_type_3', b'\x78\x9c' + bytes([0b111]) + bytes(8), R.E_BTYPE)
    b = FixedBits()
    b.put(0b101, 3)                                       # final, dynamic
    b.put(0, 5); b.put(0, 5); b.put(15, 4)                # 257 lengths, 1 distance, 19 code-length codes
    for _ in range(19):
        b.put(1, 3)                                       # nineteen codes of length 1
    add('oversubscribed', b'\x78\x9c' + b.bytes() + bytes(8), R.E_LENGTHS)
    b = FixedBits()
    b.put(3, 3)
    b.lit(0)
    b.match(3, 2)                                         # distance 2 after one byte
    b.lit(256)
    add('distance_before_start', b'\x78\x9c' + b.bytes() + bytes(4), R.E_DIST)
    out.append(('missing_distance_code', png_file(7, 4, 8, 0, dynamic_block(_table_rows(), [1], True, bad_distance=True)), R.E_SYMBOL))
    out.append(('distance_with_empty_code', png_file(7, 4, 8, 0, dynamic_block(_table_rows(), [0], True) + bytes(8)), R.E_SYMBOL))
    add('one_row_too_few', deflate(raw[:-41], 6), R.E_SIZE)
    add('one_row_too_many', deflate(raw + raw[-41:], 6), R.E_SIZE)
    bad = bytearray(raw)
    bad[41 * 20] = 5
    add('filter_byte_5', deflate(bytes(bad), 6), R.E_FILTER)
    st = bytearray(deflate(raw, 0))
    st[5] ^= 0x40                                         # NLEN of the first stored block (header 2, block header 1, LEN 2)
    add('stored_len_nlen', bytes(st), R.E_STORED)
    return out
