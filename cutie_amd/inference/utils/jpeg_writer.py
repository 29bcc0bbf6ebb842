"""The JPEG container around a device-made entropy-coded segment (PROB_TO_ID flags == 128, include/cutie_hip.h ABI 11; kernels in
csrc/jpeg_enc.hip) -- the counterpart of utils/png.py.  ``header`` + stream + EOI is the file PIL's ``Image.save(x.jpg)`` writes
(libjpeg-turbo: baseline, 4:2:0, the standard Huffman tables of ITU-T T.81 Annex K.3-K.6, no restart markers, JFIF 1.1 with density
1:1): 623 header bytes = SOI, APP0, two DQT, SOF0, four DHT, SOS.  Also here: libjpeg's quality -> quantisation-table scaling over
the two Annex K.1 / K.2 base tables, the derived Huffman code tables (the numpy model tests/jpeg_enc_ref.py reads them), and the
colour table of the overlay (``ResultSaver``'s rule: colors[id % len(colors)] for the ids of the frame's objects, zero for every
other id)."""
import struct

import numpy as np

QUALITY = 75                # what PIL's Image.save(x.jpg) uses, hence what the host overlay writes
HEADER_BYTES = 623

# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

# Annex K.1 (luminance) and K.2 (chrominance), natural order
BASE_LUM = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHR = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64)

# Annex K.3 - K.6: (table class << 4 | id as in the DHT segment, codes per length 1..16, symbols in code order)
_AC_TAIL = [r << 4 | s for r in range(16) for s in range(1, 11)]       # (not the order of the tables: only the alphabet of AC symbols)
HUFF_DC_LUM = (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
HUFF_DC_CHR = (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
HUFF_AC_LUM = (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113,
    20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
    130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
    56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
    90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
    196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
    227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
HUFF_AC_CHR = (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34,
    50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
    10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
    55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
    89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122,
    130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
    194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
    226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
HUFF_SPECS = (HUFF_DC_LUM, HUFF_AC_LUM, HUFF_DC_CHR, HUFF_AC_CHR)      # in the order of the DHT segments
assert sorted(HUFF_AC_LUM[2]) == sorted(_AC_TAIL + [0x00, 0xF0]) == sorted(HUFF_AC_CHR[2])


def huff_codes(spec):
    """(code, size) per symbol of a Huffman spec, as Annex C derives them: codes of one length count up, a longer length doubles."""
    _, bits, vals = spec
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_tables(quality: int = QUALITY) -> np.ndarray:
    """uint16 [2, 64], natural order: libjpeg's jpeg_set_quality -- scale = 5000 / q below 50, else 200 - 2 q; every entry
    (base * scale + 50) / 100 clamped to 1 .. 255 (baseline)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUM, BASE_CHR)]).astype(np.uint16)


def header(H: int, W: int, qtables: np.ndarray) -> bytes:
    """Everything in front of the entropy-coded segment; qtables = uint16 [2, 64] in natural order, values 1 .. 255."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f'a JPEG is 1 .. 65535 pixels wide and high, not {H} x {W}')
    qt = np.asarray(qtables)
    if qt.shape != (2, 64) or qt.min() < 1 or qt.max() > 255:
        raise ValueError('qtables: [2, 64], values 1 .. 255 (8-bit tables)')
    out = [b'\xff\xd8', b'\xff\xe0' + struct.pack('>H5sBBBHHBB', 16, b'JFIF\0', 1, 1, 0, 1, 1, 0, 0)]
    for k in range(2):
        out.append(b'\xff\xdb' + struct.pack('>HB', 67, k) + bytes(int(v) for v in qt[k][ZIGZAG]))
    # SOF0: 8 bits, three components -- Y 2x2 with table 0, Cb and Cr 1x1 with table 1
    out.append(b'\xff\xc0' + struct.pack('>HBHHB', 17, 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFF_SPECS:
        out.append(b'\xff\xc4' + struct.pack('>HB', 19 + len(vals), tc_th) + bytes(bits) + bytes(vals))
    out.append(b'\xff\xda' + struct.pack('>HB', 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return b''.join(out)


def wrap(stream: bytes, H: int, W: int, qtables: np.ndarray) -> bytes:
    """The file: header, the entropy-coded segment (byte-stuffed, padded with 1-bits -- what the device stage writes), EOI."""
    return header(H, W, qtables) + bytes(stream) + b'\xff\xd9'


def color_table(colors: np.ndarray, all_obj_ids) -> np.ndarray:
    """uint8 [256, 4]: entry id = colors[id % len(colors)] for the ids of ``all_obj_ids`` (1 .. 255), zero elsewhere -- the rgb mask
    of the host overlay (results_utils.py ``_write_overlay``), where a pixel whose id is not an object stays black and is still halved."""
    tab = np.zeros((256, 4), dtype=np.uint8)
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    for oid in all_obj_ids:
        if 0 < int(oid) < 256:
            tab[int(oid), :3] = colors[int(oid) % len(colors)]
    return tab
