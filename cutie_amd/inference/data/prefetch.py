"""Ordered read-ahead over an indexable frame source: decode (PIL JPEG/PNG, resize) runs on a small thread pool while the GPU
works on earlier frames.  This is what ``DataLoader(vid_reader, batch_size=None, num_workers=4)`` does in the reference's
eval loop (cutie/eval_vos.py:92) -- threads instead of worker processes: PIL and torch release the GIL while decoding /
resizing, nothing has to be pickled, and the items arrive in index order with at most ``depth`` decoded frames alive.
A model at several hundred frames/s is otherwise limited by single-threaded JPEG decode (3-5 ms per 480p frame).
``Window`` is the stage behind it in the drivers: the next few records already uploaded to the device."""
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterator, Optional


class ReadAhead:
    def __init__(self, source, *, workers: int = 4, depth: int = 8, length: Optional[int] = None,
                 getitem: Optional[Callable] = None):
        """source[i] for i in range(len(source)) (or ``getitem(i)`` / ``length``).  workers <= 0: read inline."""
        self.get = getitem or source.__getitem__
        self.n = len(source) if length is None else length
        self.workers, self.depth = workers, max(1, depth)

    def __len__(self):
        return self.n

    def __iter__(self) -> Iterator:
        if self.workers <= 0:
            for i in range(self.n):
                yield self.get(i)
            return
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='cutie-read')
        pending = deque()
        try:
            nxt = 0
            while nxt < self.n and len(pending) < self.depth:
                pending.append(pool.submit(self.get, nxt))
                nxt += 1
            while pending:
                item = pending.popleft().result()              # re-raises a reader error at the frame it belongs to
                if nxt < self.n:
                    pending.append(pool.submit(self.get, nxt))
                    nxt += 1
                yield item
        finally:
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True)


class Window:
    """The device look-ahead window of a driver: up to ``depth`` records of an iterator are queued, ``upload(record)`` runs when a
    record enters and ``check(queued record)`` when it leaves through ``pop`` (a deferred decode check: the host does not wait for
    every decode).  ``queued`` holds what is still waiting, in order; a caller builds its ``next_images`` hints from it -- the
    same objects arrive later through ``pop``, which is what the look-ahead of ``InferenceCore.step`` matches frames by."""

    def __init__(self, records, upload: Callable, check: Callable, depth: int, upload_many: Optional[Callable] = None, batch: int = 1,
                 tag=None, fill: bool = True):
        """batch = B > 1: the records enter B at a time through ONE ``upload_many(records, owners)`` call (owners[i] = the window that
        record i belongs to; ``tag`` is the caller's note on a window for that function) -- a refill happens when at least B places
        are free or the source ends, and the depth grows by B - 1, so ``queued`` is never shorter at a pop than with batch = 1.  The
        popped sequence is the same.  Several such windows fill in one call through ``pop_together``."""
        self.records, self.upload, self.check, self.depth = iter(records), upload, check, max(1, depth)
        self.upload_many, self.batch, self.tag = upload_many, max(1, int(batch)), tag
        if self.batch > 1:
            if upload_many is None:
                raise ValueError('Window: batch > 1 needs upload_many')
            self.depth += self.batch - 1
        self.queued = deque()
        self.dry = False                     # (batch > 1) the source has ended
        if fill:                             # (fill=False: the caller fills it with others, fill_together)
            self._fill()

    def _fill(self):
        if self.batch > 1:
            return fill_together([self])
        while len(self.queued) < self.depth:
            try:
                record = next(self.records)
            except StopIteration:
                return
            self.queued.append(self.upload(record))

    def pop(self):
        """The oldest queued record, checked; the window is filled up again behind it."""
        record = self.check(self.queued.popleft())
        self._fill()
        return record

    def _group(self):
        """(batch > 1) The records that are due to enter now: ``batch`` of them once that many places are free, fewer when the source
        ends there; [] while the window is full enough or dry."""
        group = []
        if not self.dry and self.depth - len(self.queued) >= self.batch:
            for _ in range(self.batch):
                try:
                    group.append(next(self.records))
                except StopIteration:
                    self.dry = True
                    break
        return group


def fill_together(windows):
    """Fill batched windows in ONE ``upload_many`` call per round: the groups that are due in each of them go up together (the feeds of a
    lock-step group, the scales of a multi-scale run: C x B frames per call).  A window that is full or dry takes no part; the call
    of the first window with records is used -- windows filled together share one uploader."""
    while True:
        groups = [(w, w._group()) for w in windows]
        owners = [w for w, g in groups for _ in g]
        if not owners:
            return
        uploaded = owners[0].upload_many([r for _, g in groups for r in g], owners)
        for w, record in zip(owners, uploaded):
            w.queued.append(record)


def pop_together(windows):
    """``pop`` of every window, in order -> their records.  Batched windows are filled again in one joint call after all have popped
    (fill_together); with batch = 1 this is ``[w.pop() for w in windows]``."""
    if all(w.batch == 1 for w in windows):
        return [w.pop() for w in windows]
    if any(w.batch == 1 for w in windows):
        raise ValueError('pop_together: the windows are all batched or none is')
    records = [w.check(w.queued.popleft()) for w in windows]
    fill_together(windows)
    return records
