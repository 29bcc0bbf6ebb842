"""Bit-level numpy model of the device PNG encoder (cutie_amd/csrc/png.hip): the same token rule, the same fixed Huffman codes and the same
bit order, so the GPU test can demand equal BYTES, and the CPU test can check the rule itself against zlib's inflater.

Filter 0 on every row (L = W + 1 filtered bytes), one final DEFLATE block with the fixed codes.  At byte i of a row:
    u = bytes from i on that equal the byte one row up (distance L; 0 in the first row)
    r = bytes from i on that equal their left neighbour in the row (distance 1; 0 at i = 0)
    n = max(u, r); n < 3 -> literal; else a match of take(n) bytes at distance L (u >= r) or 1, take(n) = n (n <= 258) | n - 3 (259, 260) | 258.
"""
import zlib

import numpy as np

ADLER = 65521


def filtered(ids: np.ndarray) -> np.ndarray:
    """uint8 [H, W] -> uint8 [H, W + 1]: the PNG scanlines with filter type 0."""
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    return np.concatenate([np.zeros((ids.shape[0], 1), np.uint8), ids], axis=1)


def capacity(H: int, W: int) -> int:
    """The bound of OpList.png_capacity, derived again: <= 9 bits per filtered byte, 3 + 7 bits of block header and end of block,
    2 + 4 bytes of zlib header and trailer; a multiple of 4."""
    body = ((W + 1) * H * 9 + 10 + 7) // 8
    return (body + 6 + 3) // 4 * 4


def adler_row_partials(row: np.ndarray):
    """(S, T) of one filtered row: S = sum of the bytes, T = sum of (L - j) * byte_j, both mod 65521."""
    L = len(row)
    r = row.astype(np.int64)
    return int(r.sum() % ADLER), int(((L - np.arange(L)) * r).sum() % ADLER)


def adler_combine(partials, L: int) -> int:
    """Adler-32 of H rows of L bytes from their partials: a = 1 + sum S_r, b = H L + sum ((H - 1 - r) L S_r + T_r)  (mod 65521)."""
    H = len(partials)
    a, b = 1, H * L
    for r, (S, T) in enumerate(partials):
        a += S
        b += (H - 1 - r) * L * S + T
    return ((b % ADLER) << 16) | (a % ADLER)


def _rev(code: int, n: int) -> int:
    return int(format(code, f'0{n}b')[::-1], 2)


def _literal(v: int):
    return (_rev(0x30 + v, 8), 8) if v < 144 else (_rev(0x190 + v - 144, 9), 9)


def _length(n: int):
    if n == 258:
        sym, eb, extra = 285, 0, 0
    elif n - 3 < 8:
        sym, eb, extra = 257 + n - 3, 0, 0
    else:
        l = n - 3
        eb = l.bit_length() - 1 - 2
        sym, extra = 261 + 4 * eb + ((l >> eb) & 3), l & ((1 << eb) - 1)
    code, cn = (_rev(sym - 256, 7), 7) if sym < 280 else (_rev(0xC0 + sym - 280, 8), 8)
    return code | (extra << cn), cn + eb


def _distance(dist: int):
    d = dist - 1
    if d < 4:
        code, eb, extra = d, 0, 0
    else:
        eb = d.bit_length() - 1 - 1
        code, extra = 2 * eb + 2 + ((d >> eb) & 1), d & ((1 << eb) - 1)
    return _rev(code, 5) | (extra << 5), 5 + eb


def _runs(flag: np.ndarray) -> np.ndarray:
    """run[i] = number of consecutive True from i on."""
    n = len(flag)
    stop = np.where(~flag, np.arange(n), n)
    nxt = np.minimum.accumulate(stop[::-1])[::-1]              # first False at or behind i
    return nxt - np.arange(n)


def take(n: int) -> int:
    return n if n <= 258 else (n - 3 if n - 258 < 3 else 258)


def row_tokens(cur: np.ndarray, up):
    """Tokens of one filtered row: ('lit', value) | ('match', length, distance).  ``up``: the filtered row above, or None."""
    L = len(cur)
    ru = _runs(cur == up) if up is not None else np.zeros(L, np.int64)
    eq = np.zeros(L, bool)
    eq[1:] = cur[1:] == cur[:-1]
    re = _runs(eq)
    out, i = [], 0
    while i < L:
        u, e = int(ru[i]), int(re[i]) if i > 0 else 0
        n = max(u, e)
        if n < 3:
            out.append(('lit', int(cur[i])))
            i += 1
        else:
            t = take(n)
            out.append(('match', t, L if u >= e else 1))
            i += t
    return out


def tokens(ids: np.ndarray):
    f = filtered(ids)
    return [row_tokens(f[r], f[r - 1] if r > 0 else None) for r in range(f.shape[0])]


def encode(ids: np.ndarray):
    """-> (zlib stream bytes, Adler-32) exactly as the device writes them."""
    f = filtered(ids)
    H, L = f.shape
    vals, lens = [3], [3]                                        # BFINAL = 1, BTYPE = 01
    dist_bits = {1: _distance(1), L: _distance(L)}
    for row in tokens(ids):
        for t in row:
            if t[0] == 'lit':
                v, n = _literal(t[1])
                vals.append(v), lens.append(n)
            else:
                v, n = _length(t[1])
                vals.append(v), lens.append(n)
                v, n = dist_bits[t[2]]
                vals.append(v), lens.append(n)
    vals.append(0), lens.append(7)                               # end of block
    vals, lens = np.array(vals, np.uint64), np.array(lens, np.int64)
    bits = ((vals[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    keep = np.arange(32)[None, :] < lens[:, None]
    body = np.packbits(bits[keep], bitorder='little').tobytes()
    adler = adler_combine([adler_row_partials(f[r]) for r in range(H)], L)
    return b'\x78\x01' + body + adler.to_bytes(4, 'big'), adler


def token_bytes(row) -> int:
    return sum(1 if t[0] == 'lit' else t[1] for t in row)


def corpus(golden_dir=None):
    """name -> uint8 [H, W]: the planes both the model and the device encoder are checked on."""
    out = {}
    if golden_dir is not None:
        import os
        from PIL import Image
        for root, _, files in sorted(os.walk(golden_dir)):
            for fn in sorted(files):
                if fn.endswith('.png'):
                    im = Image.open(os.path.join(root, fn))
                    if im.mode == 'P':
                        out['golden/' + os.path.relpath(os.path.join(root, fn), golden_dir)] = np.array(im, dtype=np.uint8)
    out['zeros'] = np.zeros((48, 70), np.uint8)
    yy, xx = np.mgrid[0:40, 0:66]
    out['checker'] = ((yy + xx) & 1).astype(np.uint8)
    out['checker_hi'] = (((yy + xx) & 1) * 111 + 144).astype(np.uint8)       # 9-bit literals only: the capacity bound itself
    out['w1'] = (np.arange(37) % 3).astype(np.uint8).reshape(37, 1)
    out['h1'] = (np.arange(300) // 50).astype(np.uint8).reshape(1, 300)
    out['one_pixel'] = np.array([[7]], np.uint8)
    for n in (257, 258, 259, 260, 261, 516, 517):                            # the filtered row: byte 0, then a run of n - 1 ... n + 1
        for idv in (0, 5):
            out[f'row{n}_id{idv}'] = np.full((3, n), idv, np.uint8)
        m = np.full((2, n + 2), 9, np.uint8)                                 # one other pixel, a literal 9, a run of exactly n
        m[:, 0] = 4
        m[1, 0] = 3
        out[f'run{n}'] = m
    for idv in (143, 144, 255):
        m = np.zeros((12, 33), np.uint8)
        m[3:9, 5:20] = idv
        m[5, 7], m[6, 30] = idv, idv
        out[f'id{idv}'] = m
        out[f'id{idv}_lits'] = np.where(((yy + xx) & 1) == 1, idv, 0).astype(np.uint8)
    rng = np.random.default_rng(20240607)
    out['noise4'] = rng.integers(0, 4, (33, 129), dtype=np.uint8)
    out['noise256'] = rng.integers(0, 256, (31, 67), dtype=np.uint8)
    blk = rng.integers(0, 4, (9, 13), dtype=np.uint8)
    out['blocks'] = np.kron(blk, np.ones((7, 23), np.uint8))[:, :290]
    return out


def check_stream(stream: bytes, ids: np.ndarray):
    """zlib inflates it to the filtered plane and the trailer is zlib's Adler-32."""
    f = filtered(ids).tobytes()
    assert zlib.decompress(stream) == f
    assert int.from_bytes(stream[-4:], 'big') == (zlib.adler32(f) & 0xffffffff)
