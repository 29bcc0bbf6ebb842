"""The JPEG corpus of the decode tests, generated from seeds with Pillow (no binary fixtures besides the bike / judo frames).
TEST INFRASTRUCTURE ONLY.  Every entry is (name, file bytes)."""
import glob
import io
import os

import numpy as np
from PIL import Image, ImageFile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SUBSAMPLING = {'444': 0, '422': 1, '420': 2}


def encode(arr, **kw) -> bytes:
    """uint8 [H, W, 3] or [H, W] -> JPEG bytes (Pillow / libjpeg-turbo)."""
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, arr.size * 4 + (1 << 16))      # optimize=True writes the file in one block
    try:
        b = io.BytesIO()
        Image.fromarray(arr).save(b, format='JPEG', **kw)
        return b.getvalue()
    finally:
        ImageFile.MAXBLOCK = old


def pil_rgb(data: bytes) -> np.ndarray:
    """What VideoReader decodes: Image.open(...).convert('RGB')."""
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def image(kind, h, w, seed=0):
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'flat':
        return np.full((h, w, 3), (37, 120, 201), dtype=np.uint8)
    if kind == 'gradient':
        y, x = np.mgrid[:h, :w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 127) // max(h + w - 2, 1)], 2).astype(np.uint8)
    if kind == 'synthetic':
        from cutie_amd.utils.synth import SyntheticClip
        return (SyntheticClip(h, w, 2, 1, seed=seed).frame(0).permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
    raise ValueError(kind)


def h1v2(seed=0, w=27, h=77) -> bytes:
    """A 4:2:2 file whose frame header is rewritten to luma sampling 1x2 and size w x h (same MCU count): Pillow cannot write 1x2."""
    mx, my = -(-w // 8), -(-h // 16)
    src = image('noise', 8 * my, 16 * mx, seed)
    d = bytearray(encode(src, quality=90, subsampling=1))
    i = d.index(b'\xff\xc0')
    assert d[i + 9] == 3 and d[i + 11] == 0x21
    d[i + 5:i + 7] = h.to_bytes(2, 'big')
    d[i + 7:i + 9] = w.to_bytes(2, 'big')
    d[i + 11] = 0x12
    return bytes(d)


def golden(clip, n=None):
    paths = sorted(glob.glob(os.path.join(GOLDEN, clip, '*.jpg')))
    return [(f'{clip}/{os.path.basename(p)}', open(p, 'rb').read()) for p in paths[:n]]


def corpus(large=True):
    """The decode corpus: sizes 1x1 .. 1920x1080, quality 50..100, 4:4:4 / 4:2:2 / 4:2:0 / greyscale / 1x2, optimised Huffman
    tables, restart intervals, the bike / judo frames.  large=False leaves out 720p and 1080p (the numpy reference is slow there)."""
    out = golden('bike', 2) + golden('judo', 2)
    sizes = [(1, 1), (7, 13), (17, 9), (480, 854)] + ([(1280, 720), (1080, 1920)] if large else [])
    k = 0
    for (h, w) in sizes:
        for kind in ('noise', 'flat', 'gradient', 'synthetic'):
            if kind == 'synthetic' and min(h, w) < 16:
                continue
            for sub in ('444', '422', '420', 'L'):
                k += 1
                q = (50, 75, 90, 95, 100)[k % 5]
                if (h * w > 500000 or kind == 'flat') and (k % 2):
                    continue                                   # (thin out the large and the trivial ones)
                arr = image(kind, h, w, seed=k)
                data = encode(arr[:, :, 0], quality=q) if sub == 'L' else encode(arr, quality=q, subsampling=SUBSAMPLING[sub])
                out.append((f'{kind}_{h}x{w}_{sub}_q{q}', data))
    for q in (50, 75, 90, 95, 100):
        out.append((f'gradient_120x160_420_q{q}', encode(image('synthetic', 120, 160, q), quality=q, subsampling=2)))
    out.append(('optimize_480x854_444', encode(image('synthetic', 480, 854, 3), quality=90, subsampling=0, optimize=True)))
    out.append(('optimize_64x96_L', encode(image('noise', 64, 96, 4)[:, :, 0], quality=75, optimize=True)))
    out.append(('restart_blocks_480x854_420', encode(image('synthetic', 480, 854, 5), quality=90, subsampling=2, restart_marker_blocks=7)))
    out.append(('restart_rows_200x300_422', encode(image('noise', 200, 300, 6), quality=75, subsampling=1, restart_marker_rows=1)))
    out.append(('restart_rows_33x47_L', encode(image('noise', 33, 47, 7)[:, :, 0], quality=95, restart_marker_rows=2)))
    out.append(('h1v2_77x27', h1v2(8)))
    out.append(('h1v2_16x2', h1v2(9, w=2, h=16)))
    out.append(('extremes_16x16_L', extremes()))
    return out


def _canonical(counts, symbols):
    """JPEG canonical Huffman codes: symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def extremes() -> bytes:
    """A 16 x 16 greyscale baseline file written by hand, with what encoders never write but libjpeg decodes: DC differences of
    categories 12 and 13 and AC runs past index 63 (libjpeg stores them at 63).  The DC values stay within +-4095, where libjpeg's C
    IDCT and its SIMD ones (16-bit, saturating) agree; beyond that they differ from each other."""
    dc_counts = [0, 0, 0, 14, 2] + [0] * 11
    dc_syms = list(range(16))
    ac_counts = [0, 3, 1] + [0] * 13
    ac_syms = [0x00, 0xF5, 0x01, 0xF0]
    dc, ac = _canonical(dc_counts, dc_syms), _canonical(ac_counts, ac_syms)
    bits = []

    def put(v, n):
        bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def sym(tab, s):
        put(*tab[s])

    for diff, overflow in ((2500, False), (-2450, True), (-4100, False), (4150, True)):     # DC 2500, 50, -4050, 100
        cat = abs(diff).bit_length()
        sym(dc, cat)
        put(diff if diff > 0 else diff + (1 << cat) - 1, cat)
        if overflow:
            for v in (20, 25, 30, 27):              # k = 16, 32, 48, then 64 -> stored at 63, the block ends
                sym(ac, 0xF5)
                put(v, 5)
        else:
            sym(ac, 0x01)
            put(0, 1)
            sym(ac, 0xF0)
            sym(ac, 0x00)
    bits.extend([1] * (-len(bits) % 8))
    data = bytearray()
    for i in range(0, len(bits), 8):
        byte = int(''.join(map(str, bits[i:i + 8])), 2)
        data.append(byte)
        if byte == 0xFF:
            data.append(0)

    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload

    out = b'\xff\xd8'
    out += seg(0xDB, bytes([0]) + bytes([1] * 64))
    out += seg(0xC0, bytes([8, 0, 16, 0, 16, 1, 1, 0x11, 0]))
    out += seg(0xC4, bytes([0x00] + dc_counts + dc_syms))
    out += seg(0xC4, bytes([0x10] + ac_counts + ac_syms))
    out += seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0]))
    return out + bytes(data) + b'\xff\xd9'
