"""Device ingest: the decoded uint8 frame goes to the GPU as it is, and ONE RESIZE launch (include/cutie_hip.h, ABI 5: flags 4, or
6 with the antialiased resize) turns it into the f32 [3, h, w] frame that the host path builds with ToTensor + F.interpolate(bilinear,
antialias=True) -- a quarter of the bytes on the copy and no per-pixel float work on the decode threads.  JPEG decoding stays on the
host.  ``VideoReader(ingest='device')`` produces the records this module finishes; the default host path is unchanged.

``ingest='device-decode'`` goes one step further: the record carries the parsed JPEG (inference/data/jpeg.py Packet), only its
compressed bytes are uploaded, and the decode runs on the GPU as three more RESIZE stages (ABI 6, flags 8 / 16 / 32) in front of
the same resize.  The uint8 frame equals PIL's, so the record equals the other modes' records."""
import threading
from contextlib import nullcontext
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ... import ops as O
from . import jpeg as J

F32 = torch.float32
_tables: Dict[Tuple, torch.Tensor] = {}
decode_stats = {'frames': 0, 'serial_segments': 0, 'max_sync_rounds': 0}   # GPU-decoded frames (checked), summed over the process
_stats_lock = threading.Lock()


def _taps(H, W, OH, OW, device) -> torch.Tensor:
    """The RESIZE tap table of one geometry on `device` (ops.resize_aa_table), built once and kept."""
    key = (H, W, OH, OW, str(device))
    t = _tables.get(key)
    if t is None:
        t = torch.from_numpy(O.resize_aa_table(H, W, OH, OW)).to(device)
        _tables[key] = t
    return t


def _resize(ol, src, H, W, C, h, w, ldrow, device):
    """Append the RESIZE that turns the device uint8 frame `src` [H, W, C] into the f32 [C, h, w] result; -> the result."""
    out = torch.empty((C, h, w), dtype=F32, device=device)
    if (h, w) == (H, W):
        ol.resize(src, out, C=C, H=H, W=W, OH=h, OW=w, plane=0, ldrow=ldrow, src_u8=True)
    else:
        scratch = torch.empty((C, H, w), dtype=F32, device=device)
        ol.resize(src, out, C=C, H=H, W=W, OH=h, OW=w, plane=0, ldrow=ldrow, src_u8=True, antialias=True,
                  taps=_taps(H, W, h, w, device), scratch=scratch)
    return out


def jpeg_buffers(pkt: J.Packet, device, rounds: int = O.JPEG_SYNC_ROUNDS) -> Dict[str, torch.Tensor]:
    """Fresh decode buffers of a packet (jpeg.stage_sizes), from the caching allocator of the current stream: every decode owns its
    own, so decodes on several threads / streams (parallel.run_concurrent) never share one."""
    sz = J.stage_sizes(pkt, rounds)
    return {'pkt': torch.from_numpy(pkt.buf).to(device),
            'work': torch.empty(sz['work'], dtype=torch.int32, device=device),
            'coef': torch.empty(sz['coef'], dtype=torch.int16, device=device),
            'planes': torch.empty(sz['planes'], dtype=torch.uint8, device=device),
            'rgb': torch.empty(pkt.shape + (3,), dtype=torch.uint8, device=device),
            'status': torch.zeros(4, dtype=torch.int32, device=device)}


class DecodeCheck:
    """The error word of one GPU decode, copied to host memory behind the decode on its stream.  Calling it waits for that copy only
    (an event), then raises ValueError naming the frame if the data was bad; later calls do nothing."""
    __slots__ = ('status', 'event', 'name', 'done')

    def __init__(self, status_dev: torch.Tensor, name: str):
        self.name, self.done = name, False
        if status_dev.device.type == 'cuda':
            self.status = torch.empty(4, dtype=torch.int32, pin_memory=True)
            self.status.copy_(status_dev, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
        else:
            self.status, self.event = status_dev.clone(), None

    def __call__(self):
        if self.done:
            return
        if self.event is not None:
            self.event.synchronize()
        self.done = True
        err, rounds, serial = (int(v) for v in self.status[:3])
        if err:
            raise ValueError(f'{self.name or "frame"}: corrupt or truncated JPEG data (GPU decode error bits {err:#x})')
        with _stats_lock:
            decode_stats['frames'] += 1
            decode_stats['serial_segments'] += serial
            decode_stats['max_sync_rounds'] = max(decode_stats['max_sync_rounds'], rounds)


def jpeg_to_device(pkt: J.Packet, device, size_hw=None, stream=None, name: Optional[str] = None, check: bool = True, keep_u8: bool = False):
    """A parsed JPEG -> f32 [3, h, w] contiguous on `device`, equal to ToTensor(+ antialiased resize) of PIL's decode.  One upload of
    the packet, then the three decode stages and the resize on `stream` (default: the current stream), into buffers of this call.
    check=True: wait for the error word and raise ValueError naming the frame (`name`, default the packet's file) if the data was bad.
    check=False: -> (frame, DecodeCheck); the caller must call the check before it uses the frame's result -- until then the frame may
    hold garbage, after a passed check it is the decoded frame.
    keep_u8=True: the decoded uint8 [H, W, 3] frame on the device joins the result: -> (frame, u8) | (frame, DecodeCheck, u8)."""
    dev = torch.device(device)
    on_gpu = dev.type == 'cuda'
    H, W = pkt.shape
    h, w = (H, W) if size_hw is None else (int(size_hw[0]), int(size_hw[1]))
    ctx = torch.cuda.stream(stream) if (on_gpu and stream is not None) else nullcontext()
    with ctx:
        b = jpeg_buffers(pkt, dev)
        ol = O.OpList(prio=False)
        ref = (pkt, b['pkt'])
        ol.jpeg_huff(ref, work=b['work'], coef=b['coef'], status=b['status'])
        ol.jpeg_idct(ref, coef=b['coef'], planes=b['planes'])
        ol.jpeg_color(ref, planes=b['planes'], rgb=b['rgb'])
        out = _resize(ol, b['rgb'], H, W, 3, h, w, 3 * W, dev)
        ol.finalize()
        ol.run()
        chk = DecodeCheck(b['status'], pkt.source if name is None else name)
    if check:
        chk()
        return (out, b['rgb']) if keep_u8 else out
    return (out, chk, b['rgb']) if keep_u8 else (out, chk)


def frame_to_device(rgb_u8, device, size_hw=None, stream=None, keep_u8: bool = False):
    """uint8 [H, W, C] (numpy array or CPU tensor; rows may be padded, pixels packed) -> f32 [C, h, w] contiguous on `device`,
    (h, w) = size_hw (default (H, W): ToTensor only).  One synchronous uint8 copy, one RESIZE launch on `stream` (default: the
    current stream).  keep_u8=True: -> (frame, the uploaded uint8 [H, W, C] on the device)."""
    u8 = torch.from_numpy(rgb_u8) if isinstance(rgb_u8, np.ndarray) else rgb_u8
    if u8.dtype != torch.uint8 or u8.dim() != 3 or u8.stride(2) != 1 or u8.stride(1) != u8.shape[2]:
        raise ValueError(f'frame_to_device: expected packed uint8 [H, W, C], got {u8.dtype} {tuple(u8.shape)} strides {u8.stride()}')
    H, W, C = u8.shape
    h, w = (H, W) if size_hw is None else (int(size_hw[0]), int(size_hw[1]))
    ctx = torch.cuda.stream(stream) if (stream is not None and torch.device(device).type == 'cuda') else nullcontext()
    with ctx:
        src = u8.to(device)
        ol = O.OpList(prio=False)
        out = _resize(ol, src, H, W, C, h, w, src.stride(0), device)
        ol.finalize()
        ol.run()
    return (out, src) if keep_u8 else out


def to_device(record: Dict, device, stream=None, defer_check: bool = False, keep_u8: bool = False) -> Dict:
    """Move a reader record to `device`: ``rgb_u8`` (VideoReader(ingest='device')) becomes ``rgb`` = f32 [3, h, w], h, w =
    ``info['rgb_shape']``, and both device-ingest keys are dropped, so the record equals the host-path one.  A host-path record
    (it holds ``rgb``) is moved as the drivers always did: ``rgb.to(device)``.  A 'device-decode' record (it holds ``jpeg``, a parsed
    packet) is decoded on the GPU on the current stream (jpeg_to_device); a corrupt frame raises ValueError with its file name --
    here, or with defer_check=True in ``finish(record)``, which the caller must call before it uses the record's result (the record
    holds ``decode_check`` until then: the drivers queue several frames ahead and check each when it leaves the look-ahead window,
    so the host does not wait for every decode).
    keep_u8=True: the original-size uint8 [H, W, 3] frame that a 'device' record uploaded or a 'device-decode' record decoded stays on
    the device as ``record['info']['image_u8']`` (what ``ResultSaver(overlay='device')`` blends the masks over: no second decode, no
    upload; ``info`` is what the drivers hand to the saver).  A host-path record has no such frame and gets no key."""
    if 'jpeg' in record:
        pkt = record.pop('jpeg')
        rgb, chk, u8 = jpeg_to_device(pkt, device, record['info'].pop('rgb_shape'), stream, record['info'].get('path_to_image') or pkt.source,
                                      check=False, keep_u8=True)
        record['rgb'] = rgb
        if keep_u8:
            record['info']['image_u8'] = u8
        if defer_check:
            record['decode_check'] = chk
        else:
            chk()
        return record
    if 'rgb_u8' not in record:
        record['rgb'] = record['rgb'].to(device)
        return record
    u8 = record.pop('rgb_u8')
    record['rgb'], src = frame_to_device(u8, device, record['info'].pop('rgb_shape'), stream, keep_u8=True)
    if keep_u8 and src.shape[2] == 3:
        record['info']['image_u8'] = src
    return record


def finish(record: Dict) -> Dict:
    """The deferred error check of a record from to_device(defer_check=True) (nothing to do for the other records): raises ValueError
    naming the frame if its GPU decode found bad data; afterwards the record equals the other modes' records."""
    chk = record.pop('decode_check', None)
    if chk is not None:
        chk()
    return record
