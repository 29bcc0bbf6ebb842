"""Host side of the GPU PNG decode (RESIZE flags 64 / 128, include/cutie_hip.h ABI 11, forms added; kernels in csrc/png_dec.hip): the container parser,
the counterpart of inference/data/jpeg.py.  The host reads the signature and IHDR, checks the CRC of the critical chunks, skips every
ancillary chunk and joins the IDAT chunks into one zlib stream; the few KB of compressed bytes are uploaded and the GPU inflates and
unfilters them (inference/data/device_ingest.py png_to_device).

Accepted: non-interlaced files of colour type 3 at 1 / 2 / 4 / 8 bits (PIL mode P; the result is the palette index), colour type 0 at 8 bits
(mode L) and colour type 2 at 8 bits (mode RGB).  Everything else -- interlace, 16 bits, alpha, grey below 8 bits, a CRC mismatch, a
missing IDAT, a bad zlib header, a row above 16384 bytes -- is declined with a short reason and decoded by PIL as before (which raises its
own error for files that are truly bad); ``fallbacks`` counts the declined files by reason, as VideoReader.decode_fallbacks does.

Packet = uint8 buffer: 8 little-endian int32 words (magic 'PNGD', W, H, bit depth, channels, bytes per filtered row, stream bytes, inflated
bytes = H * (rowbytes + 1)), then the zlib stream (csrc/png_inflate_core.h PD_H_*)."""
import struct
import threading
import zlib
from collections import Counter
from typing import NamedTuple, Optional, Tuple

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
MAGIC = 0x44474E50
HDR_WORDS = 8
HDR_BYTES = 32
HDR_MAGIC, HDR_W, HDR_H, HDR_DEPTH, HDR_CHANNELS, HDR_ROWBYTES, HDR_STREAM, HDR_INFLATED = range(8)
MAX_ROWBYTES = 16384          # PD_MAX_ROWBYTES: the unfilter stage keeps two rows in LDS

fallbacks: Counter = Counter()          # declined files by reason, summed over the process (count_fallback)
_lock = threading.Lock()


class Packet(NamedTuple):
    buf: np.ndarray            # uint8 [HDR_BYTES + stream bytes]
    shape: Tuple[int, ...]     # of the decoded array: (H, W) or (H, W, 3)
    source: str

    @property
    def hdr(self):
        return self.buf[:HDR_BYTES].view('<i4')

    @property
    def inflated(self) -> int:
        return int(self.hdr[HDR_INFLATED])

    @property
    def nbytes_out(self) -> int:
        return int(np.prod(self.shape))


def count_fallback(reason: str) -> None:
    with _lock:
        fallbacks[reason] += 1


def make_packet(W, H, depth, channels, stream: bytes, source='') -> Packet:
    """The packet of a zlib stream and its geometry (no check of the stream itself beyond what `parse` does before it calls this)."""
    rowbytes = (W * channels * depth + 7) // 8
    buf = np.empty(HDR_BYTES + len(stream), dtype=np.uint8)
    buf[:HDR_BYTES].view('<i4')[:] = [MAGIC, W, H, depth, channels, rowbytes, len(stream), H * (rowbytes + 1)]
    buf[HDR_BYTES:] = np.frombuffer(stream, dtype=np.uint8)
    return Packet(buf, (H, W) if channels == 1 else (H, W, channels), source)


def parse(data: bytes, source: str = '') -> Tuple[Optional[Packet], str]:
    """-> (Packet, '') or (None, reason)."""
    if data[:8] != SIGNATURE:
        return None, 'not a PNG'
    pos, ihdr, idat, end = 8, None, [], False
    n = len(data)
    while pos + 12 <= n:
        length, = struct.unpack('>I', data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        if pos + 12 + length > n:
            return None, 'truncated chunk'
        critical = not (kind[0] & 32)
        if critical:
            body = data[pos + 8:pos + 8 + length]
            crc, = struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])
            if zlib.crc32(kind + body) & 0xffffffff != crc:
                return None, 'bad CRC'
            if kind == b'IHDR':
                if ihdr is not None or length != 13:
                    return None, 'bad IHDR'
                ihdr = struct.unpack('>IIBBBBB', body)
            elif kind == b'IDAT':
                idat.append(body)
            elif kind == b'IEND':
                end = True
                break
            elif kind != b'PLTE':
                return None, 'unknown critical chunk'
            if ihdr is None:
                return None, 'no IHDR first'
        pos += 12 + length
    if ihdr is None:
        return None, 'no IHDR first'
    if not end:
        return None, 'no IEND'
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if comp != 0 or filt != 0:
        return None, 'unknown compression or filter method'
    if interlace != 0:
        return None, 'interlaced'
    if depth == 16:
        return None, '16 bits'
    if ctype in (4, 6):
        return None, 'alpha'
    if ctype == 0 and depth != 8:
        return None, 'grey below 8 bits'
    if not ((ctype == 3 and depth in (1, 2, 4, 8)) or (ctype in (0, 2) and depth == 8)):
        return None, 'unknown colour type or depth'
    if W < 1 or H < 1:
        return None, 'empty image'
    channels = 3 if ctype == 2 else 1
    rowbytes = (W * channels * depth + 7) // 8
    if rowbytes > MAX_ROWBYTES:
        return None, 'row too wide'
    if H * (rowbytes + 1) >= 1 << 31:
        return None, 'image too large'
    if not idat:
        return None, 'no IDAT'
    stream = b''.join(idat)
    if len(stream) < 2 or (stream[0] & 15) != 8 or (stream[0] >> 4) > 7 or (stream[1] & 32) or ((stream[0] << 8) | stream[1]) % 31:
        return None, 'bad zlib header'
    return make_packet(W, H, depth, channels, stream, source), ''


def parse_file(path: str) -> Tuple[Optional[Packet], str]:
    with open(path, 'rb') as f:
        return parse(f.read(), path)
