"""What the folder datasets' batch builders share: the seeded epoch order, pinned staging, the two halves of a batch and the
look-ahead that keeps every HIP call on the consumer's thread."""
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


def file_order_batches(n, batch_size):
    """The index lists of one pass over n samples in file order, not shuffled: the full batches of `epoch_batches` and then
    the remainder as a last, shorter one (validation and the split walk: every sample once)."""
    lists = epoch_batches(n, batch_size, shuffle=False)
    if n % batch_size:
        lists.append(list(range(n - n % batch_size, n)))
    return lists


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


class MetaLayout:
    """Named host arrays (int64, float64, float32, int32; any shape, empty ones included) side by side in one byte buffer,
    each starting on a 16-byte boundary, in the order given.  `host[name]` are the arrays as CPU tensors, `offsets[name]`
    their first bytes, `nbytes` the bytes needed.  The only place that knows where a field of the second staging buffer
    lies: the host half fills the buffer through it and the device half reads the uploaded copy through it.  The bytes
    between two fields are never written or read."""

    def __init__(self, fields):
        self.host = {name: torch.as_tensor(a).contiguous() for name, a in fields.items()}
        self.offsets, end = {}, 0
        for name, t in self.host.items():
            self.offsets[name] = (end + 15) & ~15
            end = self.offsets[name] + t.numel() * t.element_size()
        self.nbytes = end

    def views(self, buf):
        """{name: the field's view of `buf`}, a uint8 tensor of at least nbytes on any device (pinned or not): the dtypes and
        shapes of the arrays given."""
        return {name: buf[self.offsets[name]:self.offsets[name] + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
                for name, t in self.host.items()}

    def fill(self, buf):
        """Copy the arrays to their places in the host buffer `buf`."""
        for name, view in self.views(buf).items():
            view.copy_(self.host[name])


class HostBatch(list):
    """The trainer's 8-tuple with `objs_host`: the batch's object ids (B,O,A) as the host already holds them, in the rows
    of the device tensor batch[1] (its `__image__` row included).  For what names the objects without reading them back
    (split.generate_split(draw_labels=True))."""

    def __init__(self, batch, objs_host):
        super().__init__(batch)
        self.objs_host = objs_host


class _Pending:
    """A batch whose host half is under way: the decode futures and what the device half needs (slot, stage, meta, layout),
    and as attributes of their own names the host copies of the second buffer's fields (`desc` among them) and the
    dataset's host-only extras."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def done(self):
        return all(f.done() for f in self.futures)


def _decode(im, dst, mode):
    """A worker's whole job: the pixels of the opened picture, in `mode`, straight into its slice of the pinned buffer."""
    try:
        dst[:] = np.asarray(im if im.mode == mode else im.convert(mode)).reshape(-1)
    finally:
        im.close()


class BatchBuilder:
    """Batches of a folder dataset as the 8-tuple Trainer.step takes.

    A batch has a host half and a device half.  start(indices): `num_workers` threads open the files and decode them into
    a pinned buffer, back to back; the picture descriptor, the image ids and the dataset's own fields are laid out in a
    second one (MetaLayout).  finish(pending), on the current stream: ONE copy of each buffer to the device (`_upload`),
    the dataset's kernel, ops.preprocess_images and collate.packed_batch.  build(indices) is the two in a row.

    A dataset's builder supplies what is its own:
      keep_rgba    False: every picture is converted to RGB and described by three columns (byte offset, h, w), for
                   csg_preprocess.  True: a picture whose decoded mode is RGBA stays as 4-byte pixels, any other is RGB; the
                   descriptor has a fourth column, bytes per pixel, and every picture starts on a 4-byte boundary so that the
                   device reads 4-byte pixels as dwords (csg_preprocess_px).
      mean, std    T.Normalize's, where they are not ImageNet's.
      draw(indices)                   optional; runs first, before a slot is taken or a file opened, and what it returns is
                   handed to rows.  For what must happen in batch order whatever else does.
      rows(indices, sizes, drawn)     the host hook -> ({name: array}, {name: host-only extra}): the dataset's fields, padded
                   to the batch's O, which go into the second buffer, and what only the host needs.  `sizes`: int64 (B,2) =
                   (h, w) of the decoded pictures.  Both are kept, unmodified, as attributes of the pending batch.
      assemble(dev, pending)          the device hook -> (objs, boxes, rel, counts) for collate.packed_batch, from the device
                   views `dev[name]` of the fields and their host copies `pending.<name>`.  A fifth value, optional, is a
                   pair (masks or None, centres): the batch's mask slot and the object centres the graph is built from, in
                   place of None and the box centres (the COCO datasets with segmentations).
    All of them run on the consumer's thread.

    batches(lists) runs the HOST half one batch ahead: the decode of batch k + 1 — the host-bound part of the loader — runs
    in the worker threads while step k is enqueued and executed, and the device half of a batch is issued at hand-over, by
    the consumer's thread on the consumer's stream.  The workers make no HIP call at all (they touch numpy only).  That is
    deliberate: Trainer.step captures HIP graphs (graphs.py, capture mode "global"), and a HIP call another thread makes
    while a capture is open — an allocation, an event or stream synchronisation, the read-back of canonical_triplets —
    fails or invalidates the capture; the hand-over lies between two steps, where no capture is open.  `waited` counts the
    batches whose decode was not finished at hand-over, `steps` all of them."""

    keep_rgba = False
    takes_rng = False
    mean = std = None

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

    def draw(self, indices):
        return None

    def rows(self, indices, sizes, drawn):
        raise NotImplementedError

    def assemble(self, dev, pending):
        raise NotImplementedError

    def host_objs(self, pending):
        """The object ids int64 (B,O,A) of the rows `assemble` hands over, from the host copies of the fields."""
        return pending.objs.to(torch.int64)

    def start(self, indices):
        """The host half.  Called by the consumer's thread between two steps: the one HIP call it can make, the pinned
        allocation when a staging buffer has to grow, is made here and not by a worker."""
        drawn = self.draw(indices)
        slot = self._take_slot()
        opened = list(self.pool.map(self.ds.open, indices))              # headers: sizes and modes
        modes = ["RGBA" if self.keep_rgba and im.mode == "RGBA" else "RGB" for im in opened]
        desc = np.zeros((len(opened), 4), np.int64)                      # byte offset, h, w, bytes per pixel
        end = 0
        for b, (im, mode) in enumerate(zip(opened, modes)):
            desc[b] = (-(-end // 4) * 4 if self.keep_rgba else end, im.size[1], im.size[0], len(mode))
            end = int(desc[b, 0] + desc[b, 1] * desc[b, 2] * desc[b, 3])
        fields, extras = self.rows(indices, desc[:, 1:3], drawn)
        stage = self.pixels[slot].take(end)[:end]
        host = stage.numpy()                                              # the workers write through numpy: no torch call
        futures = [self.pool.submit(_decode, im, host[desc[b, 0]:desc[b, 0] + desc[b, 1] * desc[b, 2] * desc[b, 3]], mode)
                   for b, (im, mode) in enumerate(zip(opened, modes))]
        layout = MetaLayout({"desc": desc if self.keep_rgba else desc[:, :3],
                             "image_ids": np.asarray([self.ds.image_ids[i] for i in indices], np.int64), **fields})
        meta = self.meta[slot].take(layout.nbytes)[:layout.nbytes]
        layout.fill(meta)                                                 # one buffer, one copy
        return _Pending(futures=futures, slot=slot, stage=stage, meta=meta, layout=layout, **layout.host, **extras)

    def finish(self, p):
        """The device half, enqueued on the current stream -> the batch."""
        from ... import ops
        from .collate import packed_batch
        src, meta_dev = self._upload(p)
        dev = p.layout.views(meta_dev)
        objs, boxes, rel, counts, *more = self.assemble(dev, p)
        masks, centers = more[0] if more else (None, None)
        H, W = self.ds.image_size
        imgs = ops.preprocess_images(src, dev["desc"], H, W, normalize=self.ds.normalize_images, desc_host=p.desc,
                                     **({} if self.mean is None else {"mean": self.mean, "std": self.std}))
        raw = [imgs, objs, boxes, rel, None, None, masks, dev["image_ids"]]
        batch = packed_batch(self.args, self.trainer, raw, self.dev, counts=counts, centers=centers)
        ids = self.host_objs(p)                                           # packed_batch appends one row of 0 per sample
        return HostBatch(batch, torch.cat([ids, ids.new_zeros((ids.shape[0], 1, ids.shape[2]))], 1))

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
