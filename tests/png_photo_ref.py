"""Bit-level numpy model of the device PNG encoder for photographs and smooth planes (cutie_amd/csrc/png_photo.hip, PROB_TO_ID flags ==
16384): scanline filters chosen per row, tokens on the filtered bytes, one DEFLATE block per band of R rows with dynamic Huffman codes (or
the fixed ones where they are no longer).  The rule is stated in include/cutie_hip.h; this file restates it operation by operation, so the
GPU test can demand equal BYTES and the CPU test can check the rule against zlib's inflater and PIL.

1. Filter.  B = bytes per pixel, L = W B + 1.  Raw byte j of a row has a = raw[j - B] (0 for j < B), b = the byte above (0 in the first row),
   c = the byte above a.  Residuals mod 256: 0 x | 1 x - a | 2 x - b | 3 x - ((a + b) >> 1) | 4 x - paeth(a, b, c).  The cost of a filter is
   the sum of |residual as int8| (so 128 for 0x80); the lowest cost wins, ties go to the lower number.  Filtered row = filter number, residuals.
2. Tokens, on the filtered bytes f of the row (filter byte included), never across a row.  At byte i:
       n1 = bytes from i on with f[k] == f[k - 1]   (0 at i = 0)          distance 1
       nB = bytes from i on with f[k] == f[k - B]   (0 for i < B; B > 1)  distance B
       nL = bytes from i on equal to the filtered row above (0 in row 0)  distance L
   each counted up to RUNCAP = 261 and no further.  n = max(n1, nB, nL); ties go to distance 1, then B, then L.  n < MINMATCH: a literal, one
   byte.  Else a match of take(n) bytes, take(n) = n (n <= 258) | n - 3 (259, 260) | 258 (261).
3. Blocks.  Rows r with r // R == k are DEFLATE block k; the last one carries BFINAL.
4. Codes, per block.  Counts of the literal/length symbols (end-of-block counted once) and of the distance symbols.  code_lengths(): the
   symbols with a count, sorted by (count, symbol) ascending; Huffman depths by the in-place two-queue merge (a tie between a leaf and an inner
   node takes the leaf); depths above the limit are folded into it and the Kraft sum is repaired by moving one code from the longest
   length that has one down a level until the sum is exact; then the lengths, shortest first, go to the symbols from the END of the sorted
   list (largest count first).  One symbol with a count gets length 1 (an incomplete code: inflate accepts it for the distances); none: all 0.
   Limits: 15, and 7 for the code-length code.  Codes are canonical.  HLIT, HDIST, HCLEN are the smallest legal.  The HLIT + HDIST lengths are
   one sequence; at position i with value v and r equal values from i on: v == 0 and r >= 11: symbol 18 for min(r, 138); v == 0 and r >= 3:
   symbol 17 for r; v != 0, i > 0, the value before is v and r >= 3: symbol 16 for min(r, 6); else v itself.
   The block is written with the fixed codes (BTYPE 01) when that takes no more bits than the dynamic form, header and end-of-block included.
5. zlib header 78 01, the blocks, Adler-32 of the filtered bytes, big endian.
"""
import zlib

import numpy as np

ADLER = 65521
MINMATCH = 12
R = 32
RUNCAP = 261
ROW_LIMIT = 16384           # L = W B + 1 <= ROW_LIMIT
FLAGS = 16384
BUILD_BIT = 256

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, np.int64)[:286]
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
MODE = {1: 'L', 2: 'LA', 3: 'RGB', 4: 'RGBA'}

# length 3 .. 258 -> (symbol - 257, extra bits, extra value)
_LEN_SYM = np.zeros(259, np.int64)
_LEN_EB = np.zeros(259, np.int64)
_LEN_EX = np.zeros(259, np.int64)
for _n in range(3, 259):
    _k = max(k for k in range(29) if LBASE[k] <= _n)
    if _n == 258:
        _k = 28
    _LEN_SYM[_n], _LEN_EB[_n], _LEN_EX[_n] = _k, LEXT[_k], _n - LBASE[_k]


def dist_code(dist: int):
    """distance -> (symbol, extra bits, extra value)  (RFC 1951 3.2.5)"""
    d = dist - 1
    if d < 4:
        return d, 0, 0
    eb = d.bit_length() - 2
    return 2 * eb + 2 + ((d >> eb) & 1), eb, d & ((1 << eb) - 1)


def take(n: int) -> int:
    return n if n <= 258 else (n - 3 if n - 258 < 3 else 258)


def raw_rows(src0: np.ndarray, src1=None):
    """uint8 [H, W] | [H, W, 3] and an optional uint8 [H, W] -> (raw uint8 [H, W B], B): the channels interleaved, the plane last."""
    src0 = np.asarray(src0, dtype=np.uint8)
    if src0.ndim == 2:
        src0 = src0[:, :, None]
    assert src0.ndim == 3 and src0.shape[2] in (1, 3) and src0.shape[0] >= 1 and src0.shape[1] >= 1
    parts = [src0]
    if src1 is not None:
        src1 = np.asarray(src1, dtype=np.uint8)
        assert src1.shape == src0.shape[:2]
        parts.append(src1[:, :, None])
    px = np.concatenate(parts, axis=2)
    H, W, B = px.shape
    assert W * B + 1 <= ROW_LIMIT, 'row limit'
    return np.ascontiguousarray(px.reshape(H, W * B)), B


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_image(raw: np.ndarray, B: int):
    """-> (filtered uint8 [H, L], filter numbers [H], costs int64 [H, 5])"""
    H, n = raw.shape
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, B:] = x[:, :-B] if n > B else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, B:] = b[:, :-B] if n > B else 0
    res = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)], axis=1) & 255           # [H, 5, n]
    cost = np.abs(res.astype(np.uint8).view(np.int8).astype(np.int64)).sum(axis=2)                     # [H, 5]
    pick = np.argmin(cost, axis=1)                                                                    # first minimum: ties to the lower number
    out = np.empty((H, n + 1), np.uint8)
    out[:, 0] = pick
    out[:, 1:] = res[np.arange(H), pick].astype(np.uint8)
    return out, pick, cost


def _runs(flag: np.ndarray) -> np.ndarray:
    n = len(flag)
    stop = np.where(~flag, np.arange(n), n)
    nxt = np.minimum.accumulate(stop[::-1])[::-1]
    return np.minimum(nxt - np.arange(n), RUNCAP)


def row_tokens(f: np.ndarray, up, B: int, minmatch: int = MINMATCH):
    """Tokens of one filtered row -> (starts, kinds, lengths): kind -1 literal (length 1) | 0 distance 1 | 1 distance B | 2 distance L."""
    L = len(f)
    e1 = np.zeros(L, bool)
    e1[1:] = f[1:] == f[:-1]
    eB = np.zeros(L, bool)
    if B > 1 and L > B:
        eB[B:] = f[B:] == f[:-B]
    eL = (f == up) if up is not None else np.zeros(L, bool)
    n1, nB, nL = _runs(e1), _runs(eB), _runs(eL)
    n = np.maximum(np.maximum(n1, nB), nL)
    kind = np.where((n1 >= nB) & (n1 >= nL), 0, np.where(nB >= nL, 1, 2))
    cand = np.flatnonzero(n >= minmatch)
    starts, kinds, lens = [], [], []
    pos = 0
    while pos < L:
        k = int(np.searchsorted(cand, pos))
        q = int(cand[k]) if k < len(cand) else L
        if q > pos:
            starts.append(np.arange(pos, q))
            kinds.append(np.full(q - pos, -1))
            lens.append(np.ones(q - pos, np.int64))
        if q >= L:
            break
        t = take(int(n[q]))
        starts.append(np.array([q]))
        kinds.append(np.array([int(kind[q])]))
        lens.append(np.array([t]))
        pos = q + t
    return np.concatenate(starts), np.concatenate(kinds), np.concatenate(lens)


def code_lengths(counts, limit: int) -> np.ndarray:
    """Code lengths of the symbols with a count (rule 4)."""
    counts = [int(v) for v in counts]
    out = np.zeros(len(counts), np.int64)
    act = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    n = len(act)
    if n == 0:
        return out
    if n == 1:
        out[act[0]] = 1
        return out
    A = [counts[s] for s in act]
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or A[root] < A[leaf]:
            A[nxt] = A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] = A[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] += A[leaf]
            leaf += 1
    A[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            used += 1
            root -= 1
        while avbl > used:
            A[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    num = [0] * (limit + 1)
    for l in A:
        num[min(l, limit)] += 1
    total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
    while total != 1 << limit:
        num[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    j = n
    for i in range(1, limit + 1):
        for _ in range(num[i]):
            j -= 1
            out[act[j]] = i
    return out


def canonical(lengths) -> np.ndarray:
    """Canonical codes (RFC 1951 3.2.2), already bit-reversed: the value to write LSB first."""
    lengths = [int(v) for v in lengths]
    mx = max(lengths) if len(lengths) else 0
    cnt = [0] * (mx + 2)
    for l in lengths:
        if l:
            cnt[l] += 1
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = np.zeros(len(lengths), np.int64)
    for s, l in enumerate(lengths):
        if l:
            out[s] = int(format(nxt[l], f'0{l}b')[::-1], 2)
            nxt[l] += 1
    return out


def rle_lengths(seq):
    """The code-length symbols of the sequence -> [(symbol, extra bits, extra value)]."""
    seq = [int(v) for v in seq]
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            t = min(r, 138)
            out.append((18, 7, t - 11))
        elif v == 0 and r >= 3:
            t = r
            out.append((17, 3, t - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            t = min(r, 6)
            out.append((16, 2, t - 3))
        else:
            t = 1
            out.append((v, 0, 0))
        i += t
    return out


def dynamic_header(ll_len, d_len, final: bool):
    """-> [(value, bits)] of a dynamic block's header, and the pieces (hlit, hdist, hclen, code-length code lengths)."""
    hlit = max(257, max(s for s in range(286) if ll_len[s]) + 1)
    nz = [s for s in range(30) if d_len[s]]
    hdist = max(1, nz[-1] + 1) if nz else 1
    syms = rle_lengths(list(ll_len[:hlit]) + list(d_len[:hdist]))
    cl_cnt = np.zeros(19, np.int64)
    for s, _, _ in syms:
        cl_cnt[s] += 1
    cl_len = code_lengths(cl_cnt, 7)
    cl_code = canonical(cl_len)
    hclen = max(4, max(k for k in range(19) if cl_len[ORDER[k]]) + 1)
    out = [((1 if final else 0) | 2 << 1, 3), (hlit - 257, 5), (hdist - 1, 5), (hclen - 4, 4)]
    out += [(int(cl_len[ORDER[k]]), 3) for k in range(hclen)]
    for s, eb, ex in syms:
        out.append((int(cl_code[s]), int(cl_len[s])))
        if eb:
            out.append((ex, eb))
    return out, (hlit, hdist, hclen, cl_len)


def capacity(H: int, L: int) -> int:
    """Bytes that hold the stream of ANY image of H rows of L filtered bytes: a block is never longer than its fixed form, where a byte costs
    at most 9 bits (a match of >= MINMATCH bytes at most 31); 3 + 7 bits of header and end-of-block per block; 2 + 4 bytes of zlib header and
    trailer; a multiple of 4."""
    nb = -(-H // R)
    return (-(-(9 * H * L + 10 * nb) // 8) + 6 + 3) // 4 * 4


def scratch_words(H: int, L: int) -> int:
    """int32 words of the stage's scratch (csrc/png_photo.hip pph_layout): per row 4 words, per band 1024 words (counts, codes, header),
    the filtered bytes [H, L] and the token records uint16 [H, L], each rounded up to 4 words."""
    nb = -(-H // R)
    up4 = lambda v: (v + 3) & ~3
    return 4 * H + 1024 * nb + up4(-(-H * L // 4)) + up4(-(-H * L // 2))


def _pack(vals, lens) -> bytes:
    vals, lens = np.asarray(vals, np.uint64), np.asarray(lens, np.int64)
    bits = ((vals[:, None] >> np.arange(48, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    keep = np.arange(48)[None, :] < lens[:, None]
    return np.packbits(bits[keep], bitorder='little').tobytes()


def _band_counts(filt, toks, dsyms, rows):
    """Counts of the literal/length symbols (end-of-block once) and of the distance symbols over the rows of one block."""
    ll = np.zeros(286, np.int64)
    dd = np.zeros(30, np.int64)
    for r in rows:
        st, kd, ln = toks[r]
        lit = kd < 0
        ll[:256] += np.bincount(filt[r][st[lit]], minlength=256)
        ll[257:] += np.bincount(_LEN_SYM[ln[~lit]], minlength=29)
        for k in range(3):
            dd[dsyms[k][0]] += int((kd == k).sum())
    ll[256] = 1
    return ll, dd


def band_counts(e, band: int = R):
    """[(ll, dd, final)] per block of an encode() result: the counts its codes were built from."""
    H, dsyms = e['H'], [dist_code(d) for d in (1, e['B'], e['L'])]
    return [_band_counts(e['filtered'], e['tokens'], dsyms, range(b0, min(b0 + band, H))) + (min(b0 + band, H) == H,) for b0 in range(0, H, band)]


def encode(src0, src1=None, *, minmatch: int = MINMATCH, band: int = R, want_bytes: bool = True):
    """-> dict: stream (bytes, exactly the device's), adler, filtered [H, L], filters [H], forms (per block: 'fixed' | 'dynamic'), bits (per
    block), tokens (per row).  ``minmatch`` / ``band`` other than the constants and want_bytes=False are for the size tables only."""
    raw, B = raw_rows(src0, src1)
    filt, pick, _ = filter_image(raw, B)
    H, L = filt.shape
    dsyms = [dist_code(d) for d in (1, B, L)]
    toks = [row_tokens(filt[r], filt[r - 1] if r else None, B, minmatch) for r in range(H)]
    vals, lens, forms, nbits = [np.array([0x0178], np.uint64)], [np.array([16])], [], []
    for b0 in range(0, H, band):
        rows = range(b0, min(b0 + band, H))
        final = rows[-1] == H - 1
        ll, dd = _band_counts(filt, toks, dsyms, rows)
        ll_len, d_len = code_lengths(ll, 15), code_lengths(dd, 15)
        hdr, _ = dynamic_header(ll_len, d_len, final)
        ll_ext = np.zeros(286, np.int64)
        ll_ext[257:] = LEXT
        d_ext =np.array([0, 0, 0, 0] + [(s - 2) // 2 for s in range(4, 30)], np.int64)
        dyn = sum(n for _, n in hdr) + int((ll * (ll_len + ll_ext)).sum() + (dd * (d_len + d_ext)).sum())
        fix = 3 + int((ll * (FIXED_LL + ll_ext)).sum() + (dd * (5 + d_ext)).sum())
        fixed = fix <= dyn
        forms.append('fixed' if fixed else 'dynamic')
        nbits.append(fix if fixed else dyn)
        if not want_bytes:
            continue
        if fixed:
            ll_len, d_len = FIXED_LL, np.full(30, 5, np.int64)
            hdr = [((1 if final else 0) | 1 << 1, 3)]
            ll_code = canonical(list(FIXED_LL) + [8, 8])[:286]
        else:
            ll_code = canonical(ll_len)
        d_code = canonical(d_len)
        vals.append(np.array([v for v, _ in hdr], np.uint64))
        lens.append(np.array([n for _, n in hdr]))
        for r in rows:
            st, kd, ln = toks[r]
            lit = kd < 0
            v = np.zeros(len(st), np.uint64)
            n = np.zeros(len(st), np.int64)
            by = filt[r][st[lit]].astype(np.int64)
            v[lit], n[lit] = ll_code[by].astype(np.uint64), ll_len[by]
            m = ~lit
            if m.any():
                ls = 257 + _LEN_SYM[ln[m]]
                mv = ll_code[ls].astype(np.uint64)
                mn = ll_len[ls].copy()
                mv |= _LEN_EX[ln[m]].astype(np.uint64) << mn.astype(np.uint64)
                mn += _LEN_EB[ln[m]]
                ds = np.array([dsyms[k][0] for k in kd[m]])
                mv |= d_code[ds].astype(np.uint64) << mn.astype(np.uint64)
                mn += d_len[ds]
                mv |= np.array([dsyms[k][2] for k in kd[m]], np.uint64) << mn.astype(np.uint64)
                mn += np.array([dsyms[k][1] for k in kd[m]])
                v[m], n[m] = mv, mn
            vals.append(v)
            lens.append(n)
        vals.append(np.array([ll_code[256]], np.uint64))
        lens.append(np.array([ll_len[256]]))
    adler = zlib.adler32(filt.tobytes()) & 0xffffffff
    out = dict(adler=adler, filtered=filt, filters=pick, forms=forms, bits=nbits, tokens=toks, B=B, H=H, L=L,
               size=(16 + sum(nbits) + 7) // 8 + 4)
    if want_bytes:
        out['stream'] = _pack(np.concatenate(vals), np.concatenate(lens)) + adler.to_bytes(4, 'big')
        assert len(out['stream']) == out['size']
    return out


def stage(src0, src1, cap: int):
    """What the launch leaves: (stream bytes or None when they do not fit ``cap`` rounded down to 4, status int32 [4])."""
    e = encode(src0, src1)
    n = len(e['stream'])
    fits = n <= (cap & ~3)
    a = e['adler']
    status = np.array([n, a - (1 << 32) if a >= 1 << 31 else a, 0 if fits else 1, 0], np.int32)
    return (e['stream'] if fits else None), status


def check_stream(stream: bytes, filtered: np.ndarray):
    f = filtered.tobytes()
    assert zlib.decompress(stream) == f
    assert int.from_bytes(stream[-4:], 'big') == (zlib.adler32(f) & 0xffffffff)
