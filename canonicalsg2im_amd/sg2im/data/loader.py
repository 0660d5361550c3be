"""What the folder datasets' batch builders share: the seeded epoch order, pinned staging, and the look-ahead that keeps
every HIP call on the consumer's thread."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_LOADER_THREADS = 16


def epoch_batches(n, per_rank, rank=0, world=1, seed=0, epoch=0, shuffle=True):
    """The sample indices of one rank's batches in one epoch over n samples: a permutation seeded by (seed, epoch), cut into
    global batches of per_rank * world samples of which rank r takes every world-th, starting at r.  Ranks are disjoint and
    take the same number of steps; the ragged tail (fewer samples than a global batch) is dropped."""
    order = np.random.default_rng([seed, epoch]).permutation(n) if shuffle else np.arange(n)
    step = per_rank * world
    return [[int(i) for i in order[s * step:(s + 1) * step][rank::world]] for s in range(n // step)]


class _Staging:
    """A pinned byte buffer that grows, and the event after which the device has read it."""

    def __init__(self):
        self.buf, self.read = None, None

    def take(self, nbytes):
        if self.read is not None:
            self.read.synchronize()
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes * 1.25) + 64, dtype=torch.uint8, pin_memory=True)
        return self.buf


class _Pending:
    """A batch whose host half is under way: the decode futures and what the device half needs."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def done(self):
        return all(f.done() for f in self.futures)


class BatchBuilder:
    """Batches of a folder dataset as the 8-tuple Trainer.step takes.

    A batch has a host half and a device half, which a subclass writes.  start(indices): `num_workers` threads open the
    files and decode them into a pinned buffer; what else the device half needs is laid out in a second one.
    finish(pending), on the current stream: ONE copy of each buffer to the device (`_upload`), then the dataset's kernels
    and collate.packed_batch.  build(indices) is the two in a row.

    batches(lists) runs the HOST half one batch ahead: the decode of batch k + 1 — the host-bound part of the loader — runs
    in the worker threads while step k is enqueued and executed, and the device half of a batch is issued at hand-over, by
    the consumer's thread on the consumer's stream.  The workers make no HIP call at all.  That is deliberate: Trainer.step
    captures HIP graphs (graphs.py, capture mode "global"), and a HIP call another thread makes while a capture is open —
    an allocation, an event or stream synchronisation, the read-back of canonical_triplets — fails or invalidates the
    capture; the hand-over lies between two steps, where no capture is open.  `waited` counts the batches whose decode was
    not finished at hand-over, `steps` all of them."""

    def __init__(self, dataset, args, trainer, device, num_workers=1):
        self.ds, self.args, self.trainer, self.dev = dataset, args, trainer, device
        self.num_workers = max(1, min(int(num_workers), MAX_LOADER_THREADS))       # never sized from the machine's CPUs
        self.pool = ThreadPoolExecutor(max_workers=self.num_workers)
        self.pixels = [_Staging(), _Staging()]
        self.meta = [_Staging(), _Staging()]
        self.turn = 0
        self.steps = self.waited = 0

    def close(self):
        self.pool.shutdown(wait=True)

    def _take_slot(self):
        """The pair of staging buffers of the batch being started: two pairs, taken in turn."""
        slot = self.turn
        self.turn ^= 1
        return slot

    def start(self, indices):
        """The host half -> a _Pending with at least futures, slot, stage (the packed bytes) and meta."""
        raise NotImplementedError

    def finish(self, pending):
        """The device half, enqueued on the current stream -> the batch."""
        raise NotImplementedError

    def _upload(self, p):
        """Wait for the decode, then one copy of each staging buffer -> (packed bytes, second buffer) on the device."""
        for f in p.futures:
            f.result()                                                    # a worker's exception is raised here
        src = p.stage.to(self.dev, non_blocking=True)
        meta_dev = p.meta.to(self.dev, non_blocking=True)
        read = torch.cuda.Event()
        read.record()
        self.pixels[p.slot].read = self.meta[p.slot].read = read          # the slot is taken again two batches on
        return src, meta_dev

    def build(self, indices):
        """One batch, enqueued on the current stream."""
        return self.finish(self.start(indices))

    def batches(self, index_lists):
        """Generator over build(indices) for every list, with the host half of the next batch started before a batch is
        handed over."""
        index_lists = iter(index_lists)
        nxt = next(index_lists, None)
        pending = self.start(nxt) if nxt is not None else None
        while pending is not None:
            self.steps += 1
            if not pending.done():
                self.waited += 1
            batch = self.finish(pending)
            nxt = next(index_lists, None)
            pending = self.start(nxt) if nxt is not None else None        # decoded while the consumer runs its step
            yield batch
