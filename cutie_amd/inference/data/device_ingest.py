"""Device ingest: the decoded uint8 frame goes to the GPU as it is, and ONE RESIZE launch (include/cutie_hip.h, ABI 5: flags 4, or
6 with the antialiased resize) turns it into the f32 [3, h, w] frame that the host path builds with ToTensor + F.interpolate(bilinear,
antialias=True) -- a quarter of the bytes on the copy and no per-pixel float work on the decode threads.  JPEG decoding stays on the
host.  ``VideoReader(ingest='device')`` produces the records this module finishes; the default host path is unchanged."""
from contextlib import nullcontext
from typing import Dict, Tuple

import numpy as np
import torch

from ... import ops as O

F32 = torch.float32
_tables: Dict[Tuple, torch.Tensor] = {}


def _taps(H, W, OH, OW, device) -> torch.Tensor:
    """The RESIZE tap table of one geometry on `device` (ops.resize_aa_table), built once and kept."""
    key = (H, W, OH, OW, str(device))
    t = _tables.get(key)
    if t is None:
        t = torch.from_numpy(O.resize_aa_table(H, W, OH, OW)).to(device)
        _tables[key] = t
    return t


def frame_to_device(rgb_u8, device, size_hw=None, stream=None) -> torch.Tensor:
    """uint8 [H, W, C] (numpy array or CPU tensor; rows may be padded, pixels packed) -> f32 [C, h, w] contiguous on `device`,
    (h, w) = size_hw (default (H, W): ToTensor only).  One synchronous uint8 copy, one RESIZE launch on `stream` (default: the
    current stream)."""
    u8 = torch.from_numpy(rgb_u8) if isinstance(rgb_u8, np.ndarray) else rgb_u8
    if u8.dtype != torch.uint8 or u8.dim() != 3 or u8.stride(2) != 1 or u8.stride(1) != u8.shape[2]:
        raise ValueError(f'frame_to_device: expected packed uint8 [H, W, C], got {u8.dtype} {tuple(u8.shape)} strides {u8.stride()}')
    H, W, C = u8.shape
    h, w = (H, W) if size_hw is None else (int(size_hw[0]), int(size_hw[1]))
    ctx = torch.cuda.stream(stream) if (stream is not None and torch.device(device).type == 'cuda') else nullcontext()
    with ctx:
        src = u8.to(device)
        out = torch.empty((C, h, w), dtype=F32, device=device)
        ol = O.OpList(prio=False)
        if (h, w) == (H, W):
            ol.resize(src, out, C=C, H=H, W=W, OH=h, OW=w, plane=0, ldrow=src.stride(0), src_u8=True)
        else:
            scratch = torch.empty((C, H, w), dtype=F32, device=device)
            ol.resize(src, out, C=C, H=H, W=W, OH=h, OW=w, plane=0, ldrow=src.stride(0), src_u8=True, antialias=True,
                      taps=_taps(H, W, h, w, device), scratch=scratch)
        ol.finalize()
        ol.run()
    return out


def to_device(record: Dict, device, stream=None) -> Dict:
    """Finish a reader record on `device`: ``rgb_u8`` (VideoReader(ingest='device')) becomes ``rgb`` = f32 [3, h, w], h, w =
    ``info['rgb_shape']``, and both device-ingest keys are dropped, so the record equals the host-path one.  A host-path record
    (it holds ``rgb``) is moved as the drivers always did: ``rgb.to(device)``."""
    if 'rgb_u8' not in record:
        record['rgb'] = record['rgb'].to(device)
        return record
    u8 = record.pop('rgb_u8')
    record['rgb'] = frame_to_device(u8, device, record['info'].pop('rgb_shape'), stream)
    return record
