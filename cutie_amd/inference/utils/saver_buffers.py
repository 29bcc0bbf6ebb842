"""What a ``ResultSaver`` (results_utils.py) keeps per frame in flight and per geometry: the ``[status | stream]`` slab with its pinned
head and its reader, the five buffer sets, the pool that recycles them between the stepping thread and the writer thread, and the keyed
cache of the scratch tensors and the small device tables."""
from queue import Empty, Queue

import numpy as np
import torch

POLY_TABLE = 255 * 16       # polygons: bytes of the object table of up to 255 objects between the status block and the stream
RLE_TABLE = 16 + 255 * 16   # BURST: bytes of the status block and the table of up to 255 objects in front of the RLE strings


class _NoEvent:
    record = synchronize = lambda self: None


class WriterCopies:
    """Writer thread: device-to-host copies on a stream of the writer's own (made on first use), so that they do not queue behind the
    stepping thread's launches."""

    def __init__(self):
        self._stream = None

    def _on(self, device):
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=device)
        return self._stream

    def to_host(self, t: torch.Tensor) -> np.ndarray:
        """a device tensor as a numpy array"""
        if t.device.type != 'cuda':
            return t.numpy()
        with torch.cuda.stream(self._on(t.device)):
            out = t.to('cpu', non_blocking=False)
        return out.numpy()

    def rest(self, tail: torch.Tensor) -> bytes:
        """the part of a long stream behind the first slab"""
        if tail.device.type != 'cuda':
            return tail.numpy().tobytes()
        stream = self._on(tail.device)
        rest = torch.empty(tail.numel(), dtype=torch.uint8).pin_memory()
        with torch.cuda.stream(stream):
            rest.copy_(tail, non_blocking=True)
        stream.synchronize()
        return rest.numpy().tobytes()


class Slab:
    """``[status int32[4] | fixed bytes | stream]`` on the device, the pinned twin of its first ``head`` bytes, and the reader.
    ``status[0]`` is the stream's length and ``status[error_word]`` the stage's error bits.  ``fixed``: bytes between the status block and
    the stream that the reader always returns in front of it (the RLE stage's object table).  ``overflow``: what a set error word means --
    None: ``fetch`` raises (``what`` names the encoder); a callable: it is told (needed bytes, capacity) and ``fetch`` returns None (the
    caller has another way to the frame's bytes)."""

    def __init__(self, capacity, head, device, copies: WriterCopies, *, what='PNG', error_word=2, fixed=0, overflow=None):
        on_gpu = torch.device(device).type == 'cuda'
        total = 16 + fixed + capacity
        self.dev = torch.empty(total, dtype=torch.uint8, device=device)
        self.status, self.stream = self.dev[:16].view(torch.int32), self.dev[16 + fixed:]
        self.host = torch.empty(min(total, head), dtype=torch.uint8)
        if on_gpu:
            self.host = self.host.pin_memory()
        self.copies, self.what, self.error_word, self.fixed, self.overflow = copies, what, error_word, fixed, overflow

    def copy(self):
        """Stepping thread: the non-blocking copy of the head, behind the launches that wrote the slab.  The caller records the event."""
        self.host.copy_(self.dev[:self.host.numel()], non_blocking=True)

    def fetch(self, event):
        """Writer thread: ``fixed`` bytes + the stream once the copy has landed -- the tail of a stream longer than the pinned head is
        fetched here, on the writer's own stream -- or what ``overflow`` says."""
        event.synchronize()
        words = [int(v) for v in self.host[:16].view(torch.int32)]
        length, err = words[0], words[self.error_word]
        if err != 0:
            if self.overflow is None:
                raise RuntimeError(f'device {self.what} encoder: error bits {err} (stream of {length} bytes, capacity {self.stream.numel()})')
            self.overflow(length, self.stream.numel())
            return None
        end = 16 + self.fixed + length
        have = self.host.numel()
        head = self.host[16:min(end, have)].numpy().tobytes()
        if end <= have:
            return head
        return head + self.copies.rest(self.dev[have:end])                  # the rare long stream


class _Buffers:
    """A set of buffers one frame in flight owns, with the event recorded behind its copies.  ``pool`` and ``key`` are the pool's."""
    pool = key = None

    def __init__(self, device):
        self.on_gpu = torch.device(device).type == 'cuda'
        self.event = torch.cuda.Event() if self.on_gpu else _NoEvent()      # (a CPU device: the interpreter of the tests, everything is synchronous)

    def twin(self, t: torch.Tensor) -> torch.Tensor:
        """the (pinned) host tensor a device tensor is copied into"""
        host = torch.empty(t.shape, dtype=t.dtype)
        return host.pin_memory() if self.on_gpu else host


class EgressBuffers(_Buffers):
    """What one frame in flight owns (egress='device', overlay='device'): the id plane, the [status | stream] slabs of the PNG, of the
    BURST strings and of the overlay's JPEG, and the event recorded behind their copies.  ``slab(kind, H, W)``: the saver's maker of a
    'png' | 'jpeg' | 'rle' slab (its sizes, its writer stream, what an overflow means to it)."""

    def __init__(self, H, W, device, slab, *, rle=False, png=True, jpeg=False):
        super().__init__(device)
        self.H, self.W = H, W
        if rle:                                  # BURST: [status | table | strings]; the whole slab is copied
            self.rle = slab('rle', H, W)
            self.rle_table = self.rle.dev[16:RLE_TABLE].view(torch.int32).view(-1, 4)
        if png:
            self.ids = torch.empty((H, W), dtype=torch.uint8, device=device)
            self.png = slab('png', H, W)
        if jpeg:                                 # overlay='device': [status | entropy-coded segment]
            self.jpeg = slab('jpeg', H, W)


class MatteBuffers(_Buffers):
    """What one frame in flight owns of the vis_modes / soft_masks / alpha_matte outputs: per mode the composed frame and the slab of its
    JPEG segment, the quantised planes (K soft masks, then the matte) and per plane the slab of its zlib stream; one event behind all copies."""

    def __init__(self, H, W, K, modes, alpha, device, slab, *, cutout=None, dynamic=False, refine=False):
        """``cutout``: None | 'device' (the slab of the RGBA cut-out's zlib stream) | 'host' (the frame is beyond the device stage's row
        limit: the writer thread encodes it with PIL from the frame and the matte).  ``dynamic``: the planes' streams come from the
        filtered, dynamic-Huffman stage (ResultSaver png_codes='dynamic').  ``refine``: the planes pass the guided filter
        (ResultSaver matte_refine=) into ``refined`` -- the K soft masks, then the matte -- which the PNG stages read instead."""
        super().__init__(device)
        self.H, self.W, self.K, self.modes, self.alpha = H, W, K, tuple(modes), alpha
        self.cutout_mode, self.dynamic = cutout, bool(dynamic)
        # (one tensor per mode: the composite's dword stores need a 16-byte aligned frame, and H * W * 3 is rarely a multiple of 16)
        self.frames = [torch.empty((H, W, 3), dtype=torch.uint8, device=device) for _ in self.modes]
        self.jpeg = [slab('jpeg', H, W) for _ in self.modes]
        self.planes = torch.empty((K, H, W), dtype=torch.uint8, device=device)               # the soft masks
        self.matte = torch.empty((H, W), dtype=torch.uint8, device=device) if (alpha or cutout) else None   # (a tensor of its own: 16-byte aligned)
        self.png = [slab('png dynamic' if dynamic else 'png', H, W) for _ in range(K + (1 if alpha else 0))]
        self.cutout = slab('cutout', H, W) if cutout == 'device' else None
        n = K + (1 if self.matte is not None else 0)
        self.refined = torch.empty((n, H, W), dtype=torch.uint8, device=device) if (refine and n) else None

    def final_plane(self, k):
        """The plane the PNG stages encode: soft mask k < K, the matte at k == K; the refined one where the guided filter ran."""
        if self.refined is not None:
            return self.refined[k]
        return self.planes[k] if k < self.K else self.matte


class TrackBuffers(_Buffers):
    """What one frame in flight owns of the track report: the table of up to 255 objects on the device, its pinned twin and the event."""

    def __init__(self, device):
        from ... import ops as O
        super().__init__(device)
        self.dev = torch.empty(O.OpList.TRACK_MAX_OBJECTS * O.OpList.TRACK_WORDS, dtype=torch.int32, device=device)
        self.host = self.twin(self.dev)


class PolygonBuffers(_Buffers):
    """What one frame in flight owns of the polygon report: the [status | object table | rings and vertices] slab with its pinned head,
    and the event behind its copy."""

    def __init__(self, H, W, device, slab):
        super().__init__(device)
        self.H, self.W = H, W
        self.slab = slab('polygons', H, W)
        self.table = self.slab.dev[16:16 + POLY_TABLE].view(torch.int32)


class RegionBuffers(_Buffers):
    """What one frame in flight owns of the region filter: its four counts on the device, their pinned twin and the event."""

    def __init__(self, device):
        super().__init__(device)
        self.dev = torch.empty(4, dtype=torch.int32, device=device)
        self.host = self.twin(self.dev)


class BandBuffers(_Buffers):
    """What one frame in flight owns of the trimaps and dilated masks: the S band planes of the distance stage, per plane the slab of its
    zlib stream, and the event behind their copies."""

    def __init__(self, H, W, S, device, slab):
        super().__init__(device)
        self.H, self.W, self.S = H, W, S
        self.band = torch.empty((S, H, W), dtype=torch.uint8, device=device)
        self.png = [slab('png', H, W) for _ in range(S)]


class RedactBuffers(_Buffers):
    """What one frame in flight owns of the redacted frame (ResultSaver redact=): the weight plane (the dilated union of the targets, or
    their matte when no other output of the frame holds it), the plane the guided filter refines it into (``refine``), the redacted RGB
    frame, the slab of its JPEG segment and the event behind its copy."""

    def __init__(self, H, W, device, slab, *, refine=False):
        super().__init__(device)
        self.H, self.W = H, W
        self.weight = torch.empty((1, H, W), dtype=torch.uint8, device=device)
        self.refined = torch.empty((1, H, W), dtype=torch.uint8, device=device) if refine else None
        self.out = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        self.jpeg = slab('jpeg', H, W)


class Pool:
    """Buffer sets recycled between two threads: ``take(*key)`` gives a returned set of that key, a new ``make(*key)`` while fewer than
    ``limit`` sets are alive, else it blocks for the next set given back; a returned set of another key is dropped (and no longer counts).
    Only the stepping thread takes -- and counts --, only the writer thread puts."""

    def __init__(self, limit, make):
        self.limit, self.make = limit, make
        self.reset()

    def reset(self):
        self._free, self.alive = Queue(), 0

    def take(self, *key):
        while True:
            try:
                b = self._free.get_nowait()
            except Empty:
                if self.alive < self.limit:
                    self.alive += 1
                    b = self.make(*key)
                    b.pool, b.key = self, key
                    return b
                b = self._free.get()             # the next set the writer gives back
            if b.key == key:
                return b
            self.alive -= 1                      # another geometry: dropped

    def put(self, b):
        self._free.put(b)


class KeyedCache:
    """name -> {key: value}, values made on first use.  ``latest``: one key per name -- a new key drops the old value (scratch tensors,
    keyed by geometry); otherwise every key stays (the small device tables, keyed by the object tuple: objects come, go and come back)."""

    def __init__(self, latest):
        self.latest, self._slots = latest, {}

    def get(self, name, key, make):
        slot = self._slots.setdefault(name, {})
        value = slot.get(key)
        if value is None:
            if self.latest:
                slot.clear()
            value = slot[key] = make()
        return value

    def clear(self):
        self._slots.clear()
