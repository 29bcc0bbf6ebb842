"""PNG container around a finished zlib stream (``ResultSaver(egress='device')``): the device hands over the compressed,
filtered image (csrc/png.hip: filter byte 0 in front of every row of ids), the host adds signature, IHDR, PLTE, one IDAT and
IEND with their CRCs.  No PIL here; a few KB per frame go through ``zlib.crc32``.

The files differ from PIL's in bytes (other filter, fixed Huffman codes, always 8 bits per pixel where PIL packs palettes of
<= 16 colours into 1 / 2 / 4 bits) and are equal in content: ``Image.open`` gives the same mode, palette and pixels."""
import struct
import zlib
from typing import Optional, Sequence, Union

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def plte_bytes(palette: Union[bytes, Sequence[int]]) -> bytes:
    """The PLTE chunk data PIL writes for ``putpalette(palette)`` (PngImagePlugin._save): the RGB triples as given, at most
    256 and at least one of them, zero-padded to whole entries."""
    data = bytes(palette)
    colors = max(min(len(data) // 3, 256), 1)
    return data[:colors * 3].ljust(colors * 3, b'\0')


def assemble(stream: bytes, H: int, W: int, palette: Optional[Union[bytes, Sequence[int]]] = None) -> bytes:
    """File bytes of an 8-bit PNG of H x W pixels whose IDAT data is ``stream`` (a complete zlib stream of the filtered
    rows).  ``palette`` (flat RGB, what ``Image.putpalette`` takes): colour type 3 with that PLTE; None: greyscale."""
    if H < 1 or W < 1:
        raise ValueError('assemble: empty image')
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 3 if palette is not None else 0, 0, 0, 0)
    parts = [SIGNATURE, _chunk(b'IHDR', ihdr)]
    if palette is not None:
        parts.append(_chunk(b'PLTE', plte_bytes(palette)))
    parts += [_chunk(b'IDAT', bytes(stream)), _chunk(b'IEND', b'')]
    return b''.join(parts)


COLOR_TYPES = {1: 0, 2: 4, 3: 2, 4: 6}      # bytes per pixel -> PNG colour type at 8 bits: L, LA, RGB, RGBA


def assemble_image(stream: bytes, H: int, W: int, channels: int) -> bytes:
    """File bytes of an 8-bit PNG of H x W pixels of ``channels`` = 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) bytes whose IDAT data is
    ``stream``: the complete zlib stream of the filtered rows, any filter per row (csrc/png_photo.hip: filters chosen per row,
    dynamic Huffman codes).  ``Image.open`` gives the mode and the exact pixels."""
    if H < 1 or W < 1:
        raise ValueError('assemble_image: empty image')
    if channels not in COLOR_TYPES:
        raise ValueError(f'assemble_image: {channels} channels, one of {tuple(COLOR_TYPES)}')
    ihdr = struct.pack('>IIBBBBB', W, H, 8, COLOR_TYPES[channels], 0, 0, 0)
    return b''.join([SIGNATURE, _chunk(b'IHDR', ihdr), _chunk(b'IDAT', bytes(stream)), _chunk(b'IEND', b'')])
