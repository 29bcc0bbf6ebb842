"""Model of the GPU PNG decode (cutie_amd/csrc/png_dec.hip, png_inflate_core.h): an independent inflate (RFC 1950 / 1951) and PNG unfilter in
plain Python / numpy -- zlib is not called for the decode.  It produces the status block the kernel writes: error bits, bytes produced,
blocks, tokens; the first error ends the decode, the tokens before it count.

    decode(packet)       -> (array | None, status [4])        the whole decode of a png_packet.Packet (or of its uint8 buffer)
    inflate(stream, n)   -> (bytes produced as bytearray, status [4])
"""
import numpy as np

E_BTYPE, E_LENGTHS, E_SYMBOL, E_DIST, E_EOF, E_SIZE, E_STORED, E_ADLER, E_FILTER, E_HEADER = (1 << k for k in range(10))
HDR_BYTES = 32
MAGIC = 0x44474E50
MAX_ROWBYTES = 16384

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


incomplete = []           # (symbols, longest code) of every incomplete code `build` has accepted: the tests look for the single and the empty code


class Fail(Exception):
    def __init__(self, bit):
        self.bit = bit


class Bits:
    """LSB-first reader over the stream; the position is a bit index."""

    def __init__(self, data):
        self.d = bytes(data)
        self.n = 8 * len(self.d)
        self.p = 0

    def peek(self, k):
        """k <= 32 bits from the position on (zeros behind the end)."""
        i = self.p >> 3
        return (int.from_bytes(self.d[i:i + 8], 'little') >> (self.p & 7)) & ((1 << k) - 1)

    def get(self, k):
        if self.p + k > self.n:
            raise Fail(E_EOF)
        r = self.peek(k)
        self.p += k
        return r

    def left(self):
        return self.n - self.p


def build(lens, strict):
    """-> (count[16], symbols in code order) or None: over-subscribed, or incomplete (allowed: empty, or one code of length 1 -- unless
    strict)."""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    left, maxlen = 1, 0
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            return None
        if count[l]:
            maxlen = l
    if left > 0 and (strict or maxlen > 1):
        return None
    if left > 0:
        incomplete.append((len(lens), maxlen))
    symbols = [s for l in range(1, 16) for s, v in enumerate(lens) if v == l]
    return count, symbols


def symbol(b, table):
    count, symbols = table
    avail = min(15, b.left())
    code = first = index = 0
    window = b.peek(15)
    for l in range(1, avail + 1):
        code |= (window >> (l - 1)) & 1
        c = count[l]
        if code - c < first:
            b.p += l
            return symbols[index + (code - first)]
        index += c
        first = (first + c) << 1
        code <<= 1
    raise Fail(E_EOF if avail < 15 else E_SYMBOL)


def dynamic(b):
    v = b.get(14)
    nlen, ndist, ncode = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
    if nlen > 286 or ndist > 30:
        raise Fail(E_LENGTHS)
    cl = [0] * 19
    for k in range(ncode):
        cl[ORDER[k]] = b.get(3)
    ct = build(cl, True)
    if ct is None:
        raise Fail(E_LENGTHS)
    lens = []
    while len(lens) < nlen + ndist:
        s = symbol(b, ct)
        if s < 16:
            lens.append(s)
            continue
        val = 0
        if s == 16:
            if not lens:
                raise Fail(E_LENGTHS)
            val, rep = lens[-1], 3 + b.get(2)
        elif s == 17:
            rep = 3 + b.get(3)
        else:
            rep = 11 + b.get(7)
        if len(lens) + rep > nlen + ndist:
            raise Fail(E_LENGTHS)
        lens += [val] * rep
    if lens[256] == 0:
        raise Fail(E_LENGTHS)
    dt = build(lens[nlen:], False)
    lt = build(lens[:nlen], False)
    if dt is None or lt is None:
        raise Fail(E_LENGTHS)
    return lt, dt


FIXED = (build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), build([5] * 32, False))


def inflate(stream, out_len):
    """-> (bytearray of the bytes produced, [error bits, bytes produced, blocks, tokens])."""
    out = bytearray()
    st = {'blocks': 0, 'tokens': 0}
    err = 0
    try:
        b = Bits(stream)
        cmf, flg = b.get(8), b.get(8)
        if (cmf & 15) != 8 or (cmf >> 4) > 7 or (flg & 32) or ((cmf << 8) | flg) % 31:
            raise Fail(E_HEADER)
        final = 0
        while not final:
            v = b.get(3)
            final, kind = v & 1, v >> 1
            st['blocks'] += 1
            if kind == 3:
                raise Fail(E_BTYPE)
            if kind == 0:
                b.get((-b.p) % 8)
                ln, nln = b.get(16), b.get(16)
                if ln ^ nln != 0xffff:
                    raise Fail(E_STORED)
                if ln == 0:
                    continue
                if 8 * ln > b.left():
                    raise Fail(E_EOF)
                if ln > out_len - len(out):
                    raise Fail(E_SIZE)
                o = b.p // 8
                out += bytes(stream[o:o + ln])
                b.p += 8 * ln
                st['tokens'] += 1
                continue
            lt, dt = FIXED if kind == 1 else dynamic(b)
            while True:
                s = symbol(b, lt)
                if s < 256:
                    if len(out) >= out_len:
                        raise Fail(E_SIZE)
                    out.append(s)
                    st['tokens'] += 1
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise Fail(E_SYMBOL)
                ln = LBASE[s - 257] + b.get(LEXT[s - 257])
                d = symbol(b, dt)
                if d > 29:
                    raise Fail(E_SYMBOL)
                dist = DBASE[d] + b.get(DEXT[d])
                if dist > len(out):
                    raise Fail(E_DIST)
                if ln > out_len - len(out):
                    raise Fail(E_SIZE)
                p = len(out)
                if dist >= ln:
                    out += out[p - dist:p - dist + ln]
                else:
                    seg = bytes(out[p - dist:p])
                    out += (seg * (ln // dist + 1))[:ln]
                st['tokens'] += 1
        b.get((-b.p) % 8)
        adler = 0
        for _ in range(4):
            adler = adler << 8 | b.get(8)
        if len(out) != out_len:
            raise Fail(E_SIZE)
        arr = np.frombuffer(bytes(out), dtype=np.uint8).astype(np.int64)         # Adler-32, RFC 1950, written out (no zlib)
        n = len(arr)
        a = (1 + int(arr.sum())) % 65521
        s2 = (n + int((arr * (n - np.arange(n, dtype=np.int64))).sum())) % 65521      # 255 n^2 / 2 < 2^63 for n < 2.6e8
        if (s2 << 16 | a) != adler:
            raise Fail(E_ADLER)
    except Fail as f:
        err = f.bit
    return out, [err, len(out), st['blocks'], st['tokens']]


def header(buf):
    """The packet header -> (W, H, depth, channels, rowbytes, stream bytes, inflated bytes) or None (the checks of pd_header)."""
    buf = np.asarray(buf, dtype=np.uint8)
    if buf.nbytes < HDR_BYTES:
        return None
    h = [int(v) for v in buf[:HDR_BYTES].view('<i4')]
    magic, W, H, depth, ch, rb, ns, ni = h
    if magic != MAGIC or W < 1 or H < 1:
        return None
    if not (depth == 8 or (depth in (1, 2, 4) and ch == 1)) or ch not in (1, 3):
        return None
    if (W * ch * depth + 7) // 8 != rb or rb > MAX_ROWBYTES:
        return None
    if H * (rb + 1) >= 1 << 31 or ni != H * (rb + 1) or ns < 0 or ns > buf.nbytes - HDR_BYTES:
        return None
    return W, H, depth, ch, rb, ns, ni


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def unfilter(data, W, H, depth, ch, rb):
    """The filtered rows -> uint8 [H, W] | [H, W, 3], or None when a filter byte is above 4."""
    rows = np.frombuffer(bytes(data), dtype=np.uint8).reshape(H, rb + 1)
    bpp = ch
    prev = np.zeros(rb, dtype=np.int64)
    out = np.zeros((H, rb), dtype=np.uint8)
    for y in range(H):
        ft, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if ft > 4:
            return None
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        elif ft == 1:
            cur = x.copy()
            for c in range(bpp):
                cur[c::bpp] = np.cumsum(x[c::bpp]) & 255
        else:
            cur = np.zeros(rb, dtype=np.int64)
            for i in range(rb):
                a = int(cur[i - bpp]) if i >= bpp else 0
                b = int(prev[i])
                c = int(prev[i - bpp]) if i >= bpp else 0
                cur[i] = (int(x[i]) + ((a + b) >> 1 if ft == 3 else paeth(a, b, c))) & 255
        out[y] = cur
        prev = cur
    if depth == 8:
        return out.reshape(H, W) if ch == 1 else out.reshape(H, W, 3)
    px = np.arange(W) * depth
    return ((out[:, px >> 3] >> (8 - depth - (px & 7))) & ((1 << depth) - 1)).astype(np.uint8)


def decode(packet):
    """-> (decoded array or None, status [4])."""
    buf = np.asarray(getattr(packet, 'buf', packet), dtype=np.uint8)
    h = header(buf)
    if h is None:
        return None, [E_HEADER, 0, 0, 0]
    W, H, depth, ch, rb, ns, ni = h
    data, st = inflate(buf[HDR_BYTES:HDR_BYTES + ns].tobytes(), ni)
    if st[0]:
        return None, st
    arr = unfilter(data, W, H, depth, ch, rb)
    if arr is None:
        st[0] = E_FILTER
    return arr, st


class PngExecutor:
    """Wraps another executor (tests/mock_exec.py MockExecutor, or jf_ref.ScoreExecutor around it, on host memory) and runs RESIZE flags
    64 / 128 through this model: the host wiring of the consumers -- png_to_device, the scorer, score_masks -- without a GPU."""
    is_mock = True

    def __init__(self, inner):
        self.inner = inner
        self.images = 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def stream(self):
        return 0

    def _one(self, rec):
        from mock_exec import view, U8, I32
        i, p = [int(v) for v in rec['i']], [int(v) for v in rec['p']]
        flags, n, pb, ib, ob = int(rec['flags']), i[0], i[1], i[2], i[3]
        packets, table, infl, status = view(p[0], U8, (pb,)).numpy(), view(p[1], I32, (n, 4)).numpy(), view(p[2], U8, (ib,)).numpy(), view(p[4], I32, (n, 4)).numpy()
        out = view(p[3], U8, (ob,)).numpy() if flags & 128 else None
        for k in range(n):
            po, io, oo = (int(v) for v in table[k, :3])
            h = header(packets[po:]) if 0 <= po < pb and po % 16 == 0 else None
            if h is not None and (io < 0 or io % 16 or io + h[6] > ib):
                h = None
            if flags & 64:
                if h is None:
                    status[k] = [E_HEADER, 0, 0, 0]
                    continue
                data, st = inflate(packets[po + HDR_BYTES:po + HDR_BYTES + h[5]].tobytes(), h[6])
                infl[io:io + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
                status[k] = st
                self.images += 1
            if flags & 128 and status[k, 0] == 0:
                W, H, depth, ch, rb = h[:5] if h is not None else (0, 0, 0, 0, 0)
                if h is None or oo < 0 or oo + H * W * ch > ob:
                    status[k, 0] = E_HEADER
                    continue
                arr = unfilter(infl[io:io + h[6]].tobytes(), W, H, depth, ch, rb)
                if arr is None:
                    status[k, 0] = E_FILTER
                else:
                    out[oo:oo + arr.size] = arr.reshape(-1)

    def run(self, arr):
        for rec in arr:
            if int(rec['kind']) == 37 and int(rec['flags']) & 192:
                self._one(rec)
            else:
                self.inner.run(np.array([rec], dtype=arr.dtype))
