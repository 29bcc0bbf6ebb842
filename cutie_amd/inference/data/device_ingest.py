"""Device ingest: the decoded uint8 frame goes to the GPU as it is, and ONE RESIZE launch (include/cutie_hip.h, ABI 5: flags 4, or
6 with the antialiased resize) turns it into the f32 [3, h, w] frame that the host path builds with ToTensor + F.interpolate(bilinear,
antialias=True) -- a quarter of the bytes on the copy and no per-pixel float work on the decode threads.  JPEG decoding stays on the
host.  ``VideoReader(ingest='device')`` produces the records this module finishes; the default host path is unchanged.

``ingest='device-decode'`` goes one step further: the record carries the parsed JPEG (inference/data/jpeg.py Packet), only its
compressed bytes are uploaded, and the decode runs on the GPU as three more RESIZE stages (ABI 6, flags 8 / 16 / 32) in front of
the same resize.  The uint8 frame equals PIL's, so the record equals the other modes' records.  ``jpegs_to_device`` / ``to_device_many``
decode several frames through ONE chain of launches (the batch forms, RESIZE flags 256; ``--decode-batch``): one upload, one launch per
pass over all frames.

``png_to_device`` does the same for mask PNGs (inference/data/png_packet.py; RESIZE flags 64 / 128, ABI 11, forms added): a batch of parsed files is
uploaded in one copy and inflated and unfiltered in one launch per stage, one wave per image -- what the scorer's ``gt_decode='device'``
and ``score_masks --decode device`` use.  The arrays equal ``np.array(Image.open(f))``."""
import threading
from contextlib import nullcontext
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import ops as O
from . import jpeg as J
from . import png_packet as P

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


png_stats = {'images': 0, 'tokens': 0, 'blocks': 0}     # GPU-decoded PNGs (checked), summed over the process


class PngCheck:
    """The status blocks of one PNG decode launch (int32 [N, 4]: error bits, bytes produced, blocks, tokens), copied to host memory behind
    the launch on its stream.  Calling it waits for that copy only, then raises ValueError naming the first file whose error word is
    nonzero; later calls do nothing.  ``status`` keeps the host copy."""
    __slots__ = ('status', 'event', 'names', 'done')

    def __init__(self, status_dev: torch.Tensor, names: Sequence[str]):
        self.names, self.done = list(names), False
        if status_dev.device.type == 'cuda':
            self.status = torch.empty(status_dev.shape, dtype=torch.int32, pin_memory=True)
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
        st = self.status.numpy()
        bad = np.flatnonzero(st[:, 0])
        if len(bad):
            k = int(bad[0])
            raise ValueError(f'{self.names[k] or "mask"}: corrupt or truncated PNG data (GPU decode error bits {int(st[k, 0]):#x})')
        with _stats_lock:
            png_stats['images'] += len(st)
            png_stats['blocks'] += int(st[:, 2].sum())
            png_stats['tokens'] += int(st[:, 3].sum())


class PngStaging:
    """A few pinned upload buffers taken in turn (as SequenceScorer._upload's): a slot is reused only once its own upload has run -- its
    event -- and the decode check that went with it is resolved then at the latest."""

    def __init__(self, slots: int = 4):
        self.slots, self.turn, self.ring = slots, 0, []
        self.pending = []                    # checks of decodes that used no slot (a device without pinned staging)

    def take(self, nbytes: int):
        """-> (pinned uint8 [>= nbytes], slot): record the upload with ``slot['event'].record()`` and leave the check in ``slot['check']``."""
        if len(self.ring) < self.slots:
            self.ring.append({'host': None, 'event': torch.cuda.Event(), 'check': None})
            slot = self.ring[-1]
        else:
            slot = self.ring[self.turn % self.slots]
            slot['event'].synchronize()
            chk, slot['check'] = slot['check'], None
            if chk is not None:
                chk()
        self.turn += 1
        if slot['host'] is None or slot['host'].numel() < nbytes:
            slot['host'] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        return slot['host'], slot

    def finish(self):
        """Resolve every check that is still open."""
        pending, self.pending = self.pending, []
        for chk in pending:
            chk()
        for slot in self.ring:
            chk, slot['check'] = slot['check'], None
            if chk is not None:
                chk()


def png_to_device(packets: Sequence[P.Packet], device, stream=None, names: Optional[Sequence[str]] = None, check: bool = True,
                  staging: Optional[PngStaging] = None, guard: int = 0):
    """Parsed mask PNGs -> a list of uint8 device tensors, [H, W] (palette index / grey value) or [H, W, 3] each, equal to
    ``np.array(Image.open(f))``.  ONE upload -- the offset table and the packets in one buffer, through pinned staging with a non-blocking
    copy -- then one inflate and one unfilter launch over all images on `stream` (default: the current stream), one wave per image.
    check=True: wait for the status blocks and raise ValueError naming the file (`names`, default the packets' files) if any was bad.
    check=False: -> (tensors, PngCheck); the caller must call the check before it uses the results -- until then a tensor may hold garbage.
    staging: a PngStaging whose buffers are used in turn (the check is then also left in the slot and resolved when the slot comes round
    again or by ``staging.finish()``).  guard: that many bytes (a multiple of 16) of 0xA5 in front of and behind every image (tests)."""
    from ... import _lib
    dev = torch.device(device)
    on_gpu = dev.type == 'cuda'
    if on_gpu and not _lib.has_png_decode():
        raise _lib.HipLibraryError(f'{_lib.LIB_PATH} is stale (no PNG decode stages); rebuild it.')
    n = len(packets)
    if n == 0:
        raise ValueError('png_to_device: no packet')
    if guard % 16:
        raise ValueError('png_to_device: guard is a multiple of 16')
    names = [pk.source for pk in packets] if names is None else list(names)
    table, pbytes, ibytes, obytes = O.OpList.png_layout(packets, guard)
    head = 16 * n
    total = head + pbytes
    ctx = torch.cuda.stream(stream) if (on_gpu and stream is not None) else nullcontext()
    with ctx:
        slot = None
        if on_gpu and staging is not None:
            host, slot = staging.take(total)
        elif on_gpu:
            host = torch.empty(total, dtype=torch.uint8).pin_memory()
        else:
            host = torch.empty(total, dtype=torch.uint8)
        hv = host.numpy()
        hv[:head] = table.reshape(-1).view(np.uint8)
        for k, pk in enumerate(packets):
            o = head + int(table[k, 0])
            hv[o:o + pk.buf.nbytes] = pk.buf
        blob = host[:total].to(dev, non_blocking=True)
        if slot is not None:
            slot['event'].record()
        infl = torch.empty(ibytes, dtype=torch.uint8, device=dev)
        out = torch.full((obytes + guard,), 0xA5, dtype=torch.uint8, device=dev) if guard else torch.empty(obytes, dtype=torch.uint8, device=dev)
        status = torch.empty((n, 4), dtype=torch.int32, device=dev)
        tab_dev = blob[:head].view(torch.int32)
        ol = O.OpList(prio=False)
        ol.png_inflate(blob[head:], tab_dev, infl, status, n=n, packet_bytes=pbytes)
        ol.png_unfilter(blob[head:], tab_dev, infl, out, status, n=n, packet_bytes=pbytes)
        ol.finalize()
        ol.run()
        chk = PngCheck(status, names)
        if slot is not None:
            slot['check'] = chk
        elif staging is not None:
            staging.pending.append(chk)
    res = [out[int(table[k, 2]):int(table[k, 2]) + pk.nbytes_out].view(pk.shape) for k, pk in enumerate(packets)]
    if check:
        chk()
        return res
    return res, chk


class JpegBatchCheck:
    """The status blocks of one batch JPEG decode (int32 [N, 4] per image: error bits, sync rounds, serial segments), copied to host memory
    behind the decode on its stream.  ``chk()`` waits for that copy only, then raises ValueError naming the first bad frame; ``chk(k)``
    does the same for frame k alone (the drivers check a frame when it leaves the look-ahead window: a bad frame further on raises when
    its own turn comes).  A frame that passed is counted in ``decode_stats`` once."""
    __slots__ = ('status', 'event', 'names', 'seen', 'lock')

    def __init__(self, status_dev: torch.Tensor, names: Sequence[str]):
        self.names, self.seen, self.lock = list(names), [False] * len(names), threading.Lock()
        if status_dev.device.type == 'cuda':
            self.status = torch.empty(status_dev.shape, dtype=torch.int32, pin_memory=True)
            self.status.copy_(status_dev, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
        else:
            self.status, self.event = status_dev.clone(), None

    def __call__(self, k: Optional[int] = None):
        with self.lock:
            todo = [j for j in (range(len(self.names)) if k is None else (k,)) if not self.seen[j]]
            if not todo:
                return
            if self.event is not None:
                self.event.synchronize()
                self.event = None
            st = self.status.numpy()
            for j in todo:
                self.seen[j] = True
                err, rounds, serial = (int(v) for v in st[j, :3])
                if err:
                    what = 'bad decode table or packet header' if err & 4 else 'corrupt or truncated JPEG data'
                    raise ValueError(f'{self.names[j] or "frame"}: {what} (GPU decode error bits {err:#x})')
                with _stats_lock:
                    decode_stats['frames'] += 1
                    decode_stats['serial_segments'] += serial
                    decode_stats['max_sync_rounds'] = max(decode_stats['max_sync_rounds'], rounds)

    def one(self, k: int):
        """The check of frame k as a callable of its own (what a record's ``decode_check`` holds)."""
        return lambda: self(k)


def jpegs_to_device(packets: Sequence[J.Packet], device, sizes_hw=None, stream=None, names: Optional[Sequence[str]] = None, check: bool = True,
                    keep_u8: bool = False, staging: Optional[PngStaging] = None, guard: int = 0):
    """Parsed JPEGs -> a list of f32 [3, h, w] contiguous frames on `device`, each equal to what ``jpeg_to_device`` returns for that packet
    ((h, w) = sizes_hw[k], default the frame's own size).  ONE upload -- the table and the packets in one buffer, through pinned staging
    with a non-blocking copy -- then ONE op list on `stream` (default: the current stream): the three decode stages in their batch forms
    (RESIZE flags 8 / 16 / 32 with 256: one launch per pass over all images) and the per-frame RESIZE of every image, into buffers of this
    call.  The uint8 frames have an allocation of their own, so a caller that keeps one of them does not pin work, coef and planes.
    check=True: wait for the status blocks and raise ValueError naming the first bad frame (`names`, default the packets' files).
    check=False: -> (frames, JpegBatchCheck); the caller calls the check (whole, or per frame) before it uses a frame's result.
    keep_u8=True: the decoded uint8 [H, W, 3] frames join the result: -> (frames, u8s) | (frames, check, u8s).
    staging: a PngStaging whose pinned buffers are used in turn (a slot is reused once its upload has run).  guard: that many bytes (a multiple of 16) of 0xA5 in front of and behind
    every image in coef, planes and rgb (tests)."""
    from ... import _lib
    dev = torch.device(device)
    on_gpu = dev.type == 'cuda'
    if on_gpu and not _lib.has_jpeg_batch():
        raise _lib.HipLibraryError(f'{_lib.LIB_PATH} is stale (no batch JPEG decode); rebuild it.')
    n = len(packets)
    if n == 0:
        raise ValueError('jpegs_to_device: no packet')
    names = [pk.source for pk in packets] if names is None else list(names)
    table, sz = O.OpList.jpeg_layout(packets, guard=guard)
    head = -(-32 * n // 16) * 16
    total = head + sz['packets']
    ctx = torch.cuda.stream(stream) if (on_gpu and stream is not None) else nullcontext()
    with ctx:
        slot = None
        if on_gpu and staging is not None:
            host, slot = staging.take(total)
        elif on_gpu:
            host = torch.empty(total, dtype=torch.uint8).pin_memory()
        else:
            host = torch.empty(total, dtype=torch.uint8)
        hv = host.numpy()
        hv[:32 * n] = table.reshape(-1).view(np.uint8)
        for k, pk in enumerate(packets):
            o = head + int(table[k, 0])
            hv[o:o + pk.buf.nbytes] = pk.buf
        blob = host[:total].to(dev, non_blocking=True)
        if slot is not None:
            slot['event'].record()

        def buf(name, dtype, fill):
            if guard:
                return torch.full((sz[name],), fill, dtype=dtype, device=dev)
            return torch.empty(sz[name], dtype=dtype, device=dev)
        work = torch.empty(sz['work'], dtype=torch.int32, device=dev)
        coef, planes, rgb = buf('coef', torch.int16, -0x5A5B), buf('planes', torch.uint8, 0xA5), buf('rgb', torch.uint8, 0xA5)
        status = torch.empty((n, 4), dtype=torch.int32, device=dev)
        tab_dev, pk_dev = blob[:32 * n].view(torch.int32), blob[head:]
        ol = O.OpList(prio=False)
        ol.jpeg_huff_batch(pk_dev, tab_dev, sz, status, n=n, work=work, coef=coef)
        ol.jpeg_idct_batch(pk_dev, tab_dev, sz, status, n=n, coef=coef, planes=planes)
        ol.jpeg_color_batch(pk_dev, tab_dev, sz, status, n=n, planes=planes, rgb=rgb)
        outs, u8s = [], []
        for k, pk in enumerate(packets):
            H, W = pk.shape
            h, w = (H, W) if (sizes_hw is None or sizes_hw[k] is None) else (int(sizes_hw[k][0]), int(sizes_hw[k][1]))
            o = int(table[k, 4])
            u8 = rgb[o:o + H * W * 3].view(H, W, 3)
            u8s.append(u8)
            outs.append(_resize(ol, u8, H, W, 3, h, w, 3 * W, dev))
        ol.finalize()
        ol.run()
        chk = JpegBatchCheck(status, names)          # (not left in the staging slot: a slot that comes round must not raise for a frame
    if check:                                        #  that is still queued -- the slot's event alone guards the pinned buffer)
        chk()
        return (outs, u8s) if keep_u8 else outs
    return (outs, chk, u8s) if keep_u8 else (outs, chk)


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


def to_device_many(records: Sequence[Dict], device, stream=None, defer_check: bool = True, keep_u8: bool = False,
                   staging: Optional[PngStaging] = None) -> List[Dict]:
    """``to_device`` for several records at once, in order: the 'device-decode' records among them (they hold ``jpeg``) go through ONE
    ``jpegs_to_device`` call -- one upload, one chain of launches -- and every other record (host-path, ``rgb_u8``, a frame the parser
    declined) through ``to_device`` as it is.  Every decoded record gets a ``decode_check`` that resolves its own frame of the shared
    check, so ``finish(record)`` works unchanged; defer_check=False checks them all here.  keep_u8: one bool, or one per record (the
    records of several feeds in one call)."""
    records = list(records)
    keep = [bool(keep_u8)] * len(records) if isinstance(keep_u8, (bool, int)) else [bool(v) for v in keep_u8]
    batch = [k for k, r in enumerate(records) if 'jpeg' in r]
    if batch:
        pkts = [records[k].pop('jpeg') for k in batch]
        infos = [records[k]['info'] for k in batch]
        frames, chk, u8s = jpegs_to_device(pkts, device, [i.pop('rgb_shape') for i in infos], stream,
                                           [i.get('path_to_image') or p.source for i, p in zip(infos, pkts)], check=False, keep_u8=True,
                                           staging=staging)
        for j, k in enumerate(batch):
            records[k]['rgb'] = frames[j]
            if keep[k]:
                infos[j]['image_u8'] = u8s[j]
            records[k]['decode_check'] = chk.one(j)
    done = set(batch)
    out = [r if k in done else to_device(r, device, stream, defer_check=defer_check, keep_u8=keep[k]) for k, r in enumerate(records)]
    if not defer_check:
        for r in out:
            finish(r)
    return out


def finish(record: Dict) -> Dict:
    """The deferred error check of a record from to_device(defer_check=True) (nothing to do for the other records): raises ValueError
    naming the frame if its GPU decode found bad data; afterwards the record equals the other modes' records."""
    chk = record.pop('decode_check', None)
    if chk is not None:
        chk()
    return record
