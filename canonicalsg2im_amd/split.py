"""A dataset split -> pictures: per image id the real picture, the picture generated from the ground-truth layout and the
one generated from the predicted layout (the reference's scripts/generation_attspade.py, whose folders gt/,
generation/gt_box_gt_mask/ and generation/pred_box_pred_mask/ are what FID and the Inception score are computed from by
outside tools), and pictures from a table of layouts alone (its scripts/generation_dataframe.py and layout_to_img.py).

`generate_split(sampler, batches, out_dir, deprocess=...)` walks the trainer's 8-tuples (what `BatchBuilder.batches`
yields) through calls this package already has, in this order per batch and under `no_grad`:

    generation/gt_box_gt_mask     Sampler.generate(..., boxes_gt=boxes, masks_gt=masks)
    generation/pred_box_pred_mask Sampler.generate(...)            (not with --skip_graph_model 1); boxes_pred is this call's
    gt                            ops.deprocess_u8 of the batch's own images: the picture as the model saw it, resized and
                                  normalised, through the same deprocess (generation_attspade.py:47,71)
    layout/gt, layout/pred        with draw_boxes: `gt` under the ground-truth boxes, the predicted-layout picture under the
                                  predicted ones (ops.draw_boxes_u8, palette and thickness of generate_from_graphs); outlines
                                  never go into gt/ or generation/, which feed the metrics; with draw_labels the objects'
                                  names as well (ops.draw_labels_u8), from the ids the batch holds on the host
    ops.box_iou                   the per-object IoU and the running totals of Evaluator.check_model
    ops.relation_agreement        with relations=True only: whether the predicted layout obeys the batch's triplets, per image
                                  by triplet type and as running totals by type and predicate (`generalisation_report`
                                  makes the large-graph run's generalisation.json of them, on the host)
    rewrite=Rewrite(...)          opt-in, the robustness walk: every graph also rewritten on the device into an equivalent or
                                  a corrupted one (ops.select_location_rows, ops.rewrite_rows), laid out as well and compared
                                  (ops.layout_consistency; `robustness_report` makes robustness.json) — see generate_split

Nothing is read back inside the loop.  The uint8 pictures stay planar and leave, with the batch's ids, objects, boxes and
IoU, in non-blocking copies to one of two pinned host buffers on a side stream (`PictureWriter`); a buffer whose copy has
completed is handed to a pool of threads that join the planes (PIL.Image.merge) and encode the files (`FileWriter`) while
the next batch is generated.  The threads make no HIP call (graphs.py captures on the loop's thread).  An error a thread
meets — or the loop — ends the run: nothing is submitted after it, `close()` joins the threads and raises it.  A file's
error surfaces one or two batches after the batch it belongs to, since that batch's files are written while the next is
walked; no batch is walked after it has been seen.

`rows` is one dictionary per image in the order generated — image_id, objects (names, as authored.py reads them),
gt_boxes, predicted_boxes, iou, over the rows `box_iou` counts — and `layouts.json` holds them.  `generate_layouts` draws
pictures from such rows with the generator alone: the scene-graph encoder is not run, so a generator-only checkpoint works.
The rows carry boxes, not masks: a model that predicts masks draws its layouts from the boxes alone there.
"""
import dataclasses
import json
import math
import os
import queue
import threading

import torch

from . import authored

MAX_WRITER_THREADS = 16
FORMATS = {"png": {}, "jpg": {"quality": 95}}
SETS = ("gt", "generation/gt_box_gt_mask", "generation/pred_box_pred_mask", "layout/gt", "layout/pred")
_BOX_KEYS = {"pred": "predicted_boxes", "gt": "gt_boxes"}
REWRITTEN_SET = "generation/pred_box_pred_mask_rewritten"                   # generate_split(rewrite=...): the pictures of graph B
LOCATION_RELATIONS = ("__below__", "__above__", "__left of__", "__right of__", "__inside__", "__surrounding__")   # slots 0..5


@dataclasses.dataclass(frozen=True)
class Rewrite:
    """How generate_split rewrites every graph (ops.rewrite_rows): mode "one_sided" (an equivalent graph: a share of the
    pairs stated in one direction only) or "noise" (a share of the rows with a wrong predicate), share in [0, 1],
    direction "forward" | "backward" | "random" (one_sided), seed: of the rows' hash and of the converse draws."""
    mode: str
    share: float = 1.0
    direction: str = "random"
    seed: int = 0

    def check(self):
        from . import ops
        if self.mode not in ops.REWRITE_MODES:
            raise ValueError("rewrite: mode must be one of %s, got %r" % (" or ".join(repr(k) for k in ops.REWRITE_MODES), self.mode))
        if self.direction not in ops.REWRITE_DIRECTIONS:
            raise ValueError("rewrite: direction must be one of %s, got %r" % (
                " or ".join(repr(k) for k in ops.REWRITE_DIRECTIONS), self.direction))
        if isinstance(self.share, bool) or not isinstance(self.share, (int, float)) or not 0.0 <= self.share <= 1.0:
            raise ValueError("rewrite: share must be a number in [0, 1], got %r" % (self.share,))
        if isinstance(self.seed, bool) or not isinstance(self.seed, int) or not 0 <= self.seed < (1 << 32):
            raise ValueError("rewrite: seed must be an integer in [0, 2^32) (it seeds a numpy RandomState too), got %r" % (self.seed,))
        return self


def save_planar(array, path, **options):
    """uint8 (3,H,W) planes -> an RGB file; the planes are joined here, on the host (PIL.Image.merge)."""
    from PIL import Image                      # only here: importing the package never needs PIL
    Image.merge("RGB", [Image.fromarray(p) for p in array]).save(path, **options)


class FileWriter:
    """(array, path) jobs -> files, in `num_threads` threads (1 .. 16, never sized from the machine's CPUs) behind a bounded
    queue: `submit` blocks while the queue is full.  The first error a job raises is kept: jobs still queued are dropped,
    `submit` raises it from then on, and `close()` — which joins the threads — raises it.  Host only: no thread makes a
    device call.  `encode(array, path)` is the job, by default `save_planar` with the format's options."""

    def __init__(self, num_threads=8, image_format="png", queue_size=None, encode=None):
        if image_format not in FORMATS:
            raise ValueError("image_format must be one of %s, got %r" % (" or ".join(repr(k) for k in FORMATS), image_format))
        if int(num_threads) < 1:
            raise ValueError("num_writers must be at least 1, got %r" % (num_threads,))
        self.num_threads = min(int(num_threads), MAX_WRITER_THREADS)
        options = FORMATS[image_format]
        self.encode = encode if encode is not None else (lambda array, path: save_planar(array, path, **options))
        self.jobs = queue.Queue(maxsize=int(queue_size) if queue_size else 4 * self.num_threads)
        self.error = None
        self._lock = threading.Lock()
        self._closed = False
        self.threads = [threading.Thread(target=self._run, name="csg-file-writer-%d" % i, daemon=True)
                        for i in range(self.num_threads)]
        for t in self.threads:
            t.start()

    def _run(self):
        while True:
            job = self.jobs.get()
            try:
                if job is None:
                    return
                if self.error is None:
                    self.encode(*job)
            except BaseException as e:                  # kept for the loop's thread, which raises it
                with self._lock:
                    if self.error is None:
                        self.error = e
            finally:
                self.jobs.task_done()

    def check(self):
        if self.error is not None:
            raise self.error

    def submit(self, array, path, block=True):
        """Queue one job.  block=False raises queue.Full instead of waiting for room."""
        if self._closed:
            raise RuntimeError("FileWriter.submit after close()")
        self.check()
        self.jobs.put((array, path), block=block)

    def drain(self):
        """Wait until every job submitted so far has been written or dropped; raises the kept error."""
        self.jobs.join()
        self.check()

    def close(self, reraise=True):
        """Join the threads (after the jobs queued so far); with `reraise` raise the first error a job met."""
        if not self._closed:
            self._closed = True
            for _ in self.threads:
                self.jobs.put(None)
            for t in self.threads:
                t.join()
        if reraise:
            self.check()


class _Slot:
    def __init__(self):
        self.buf = self.event = self.views = self.refs = self.then = None


class PictureWriter:
    """Device tensors -> the host, beside the next batch.  `put({name: tensor}, then)` enqueues non-blocking copies of the
    tensors into one of two pinned buffers on a side stream (`streams.beside`), ordered after the work that produced them,
    and records an event behind them.  The batch put before it is handed over first: its event is waited for and
    `then({name: numpy view})` runs on the caller's thread — it submits the file jobs, which read the views in place.  A
    buffer is written again two puts later, after `files.drain()`.  `flush()` hands over what is still in flight."""

    def __init__(self, device, files=None):
        self.device = torch.device(device)
        self.files = files
        self.slots = [_Slot(), _Slot()]
        self.turn = 0
        self.inflight = []

    def _hand_over(self):
        slot = self.inflight.pop(0)
        slot.event.synchronize()
        then, views = slot.then, slot.views
        slot.refs = slot.then = slot.views = None
        then(views)

    def put(self, tensors, then):
        from . import streams
        slot = self.slots[self.turn]
        self.turn ^= 1
        if self.files is not None:
            self.files.drain()                          # the jobs that read this slot's buffer (two puts ago) are done
        while self.inflight:                            # the previous batch: its jobs encode while this one is copied out
            self._hand_over()
        offsets, end = {}, 0
        tensors = {k: t.contiguous() for k, t in tensors.items()}
        for k, t in tensors.items():
            offsets[k] = (end + 15) & ~15
            end = offsets[k] + t.numel() * t.element_size()
        if slot.buf is None or slot.buf.numel() < end:
            slot.buf = torch.empty(int(end * 1.25) + 64, dtype=torch.uint8, pin_memory=True)
        host = {k: slot.buf[offsets[k]:offsets[k] + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
                for k, t in tensors.items()}
        with streams.beside("split_copy", self.device):
            for k, t in tensors.items():
                if t.numel():
                    host[k].copy_(t, non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record()
        # the device tensors are held until the hand-over: their blocks cannot be given out again under the copies
        slot.refs, slot.then, slot.views = tensors, then, {k: v.numpy() for k, v in host.items()}
        self.inflight.append(slot)

    def flush(self):
        while self.inflight:
            self._hand_over()
        if self.files is not None:
            self.files.drain()


def _finite_box(box):
    return isinstance(box, (list, tuple)) and len(box) == 4 and all(
        isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in box)


def encode_layouts(rows, which, vocab):
    """The host checks of `generate_layouts`, before any launch: `rows` (the `images` of a layouts.json) ->
    [(image_id, object id rows [n][A], boxes [n][4])].  ValueError("layouts row <index>: ... <token>") for an unknown class
    or attribute name, a row without the chosen boxes, mismatched lengths, a box that is not four finite numbers, a missing
    or repeated image id."""
    if which not in _BOX_KEYS:
        raise ValueError("layouts: which must be 'pred' or 'gt', got %r" % (which,))
    if not isinstance(rows, list) or len(rows) == 0:
        raise ValueError("layouts: a non-empty list of rows is needed")
    key = _BOX_KEYS[which]
    out, seen = [], set()
    for index, row in enumerate(rows):
        bad = lambda what, index=index: ValueError("layouts row %d: %s" % (index, what))
        if not isinstance(row, dict) or not isinstance(row.get("objects"), list):
            raise bad("a row is {\"image_id\": ..., \"objects\": [...], %r: [...]}, got %r" % (key, row))
        image_id = row.get("image_id")
        if isinstance(image_id, bool) or not isinstance(image_id, (int, str)):
            raise bad("image_id %r is neither an integer nor a string" % (image_id,))
        if image_id in seen:
            raise bad("image_id %r a second time: it would overwrite a file" % (image_id,))
        seen.add(image_id)
        ids = authored.object_ids(row["objects"], vocab, bad)
        boxes = row.get(key)
        if not isinstance(boxes, list):
            raise bad("no %r" % key)
        if len(boxes) != len(ids):
            raise bad("%d objects but %d %s" % (len(ids), len(boxes), key))
        for k, box in enumerate(boxes):
            if not _finite_box(box):
                raise bad("%s[%d] = %r is not four finite numbers" % (key, k, box))
        out.append((image_id, ids, [[float(v) for v in box] for box in boxes]))
    return out


def layout_batch(samples, vocab):
    """[(image_id, id rows, boxes)] -> (objs int64 (B,O,A), boxes fp32 (B,O,4)) on the host as a dataset batch carries them:
    a sample's real objects, then its `__image__` row with box -1, then rows of 0 with box -1 up to O = the most objects of
    a sample + 1 (sg2im/data/collate.py)."""
    names = list(vocab["attributes"].keys())
    image_row = [vocab["attributes"][a]["__image__"] for a in names]
    B, O = len(samples), max(len(ids) for _, ids, _ in samples) + 1
    objs = torch.zeros((B, O, len(names)), dtype=torch.int64)
    boxes = torch.full((B, O, 4), -1.0, dtype=torch.float32)
    for b, (_, ids, bx) in enumerate(samples):
        n = len(ids)
        if n:
            objs[b, :n] = torch.tensor(ids, dtype=torch.int64)
            boxes[b, :n] = torch.tensor(bx, dtype=torch.float64).to(torch.float32)
        objs[b, n] = torch.tensor(image_row, dtype=torch.int64)
    return objs, boxes


class _Paths:
    """<out_dir>/<set>/<image_id>.<ext> (the reference's "{}/{}.jpg".format(path, image_ids[i])); a set's directory is
    made when its first picture is."""

    def __init__(self, out_dir, ext):
        self.out_dir, self.ext = out_dir, ext
        self.made = set()

    def of(self, name, image_id):
        d = os.path.join(self.out_dir, *name.split("/"))
        if d not in self.made:
            os.makedirs(d, exist_ok=True)
            self.made.add(d)
        return os.path.join(d, "%s.%s" % (image_id, self.ext))


class SplitRows:
    """The host half of the split walk, batch by batch: `take({name: numpy array})` — image_id (B,), objs (B,O,A), boxes
    (B,O,4), with a graph model boxes_pred, iou and counted, and the uint8 (B,3,H,W) pictures under their SETS names — adds
    one row per image to `rows` and submits the pictures' files.  An image id seen a second time raises before anything of
    that sample is written."""

    def __init__(self, vocab, files=None, paths=None):
        self.vocab, self.files, self.paths = vocab, files, paths
        self.image_id_obj = vocab["object_name_to_idx"]["__image__"]
        self.rows, self.seen = [], set()

    def take(self, host):
        objs, boxes = host["objs"], host["boxes"]
        counted = host["counted"].astype(bool) if "counted" in host else \
            (boxes != -1).any(-1) & (objs[..., 0] != self.image_id_obj)        # remove_dummies_and_padding's rule
        for i, image_id in enumerate(host["image_id"].tolist()):
            if image_id in self.seen:
                raise ValueError("image id %r a second time in one run: it would overwrite a file" % (image_id,))
            self.seen.add(image_id)
            keep = counted[i]
            row = {"image_id": image_id, "objects": authored.object_names(objs[i][keep].tolist(), self.vocab),
                   "gt_boxes": boxes[i][keep].tolist()}
            if "boxes_pred" in host:
                row["predicted_boxes"] = host["boxes_pred"][i][keep].tolist()
                row["iou"] = host["iou"][i][keep].tolist()
            if "relations" in host:                     # generate_split(relations=True): {agreeing, tested} by triplet type
                row["relation_agreement"] = {"agreeing": host["relations"][i, :, 0].tolist(),
                                             "tested": host["relations"][i, :, 1].tolist()}
            if "rw_boxes_pred" in host:                 # generate_split(rewrite=...): the layout of the rewritten graph
                pairs = host["rw_pairs"][i].tolist()
                row["rewritten"] = {
                    "boxes_pred": host["rw_boxes_pred"][i][keep].tolist(), "iou": host["rw_iou"][i][keep].tolist(),
                    "consistency_iou": host["rw_cons_iou"][i][keep].tolist(), "shift": host["rw_shift"][i][keep].tolist(),
                    "pair_relations": dict({name: {"in_a": pairs[3 * k], "in_b": pairs[3 * k + 1], "in_both": pairs[3 * k + 2]}
                                            for k, name in enumerate(LOCATION_RELATIONS)},
                                           same_pairs=pairs[18], pairs=pairs[19]),
                    "relation_agreement": {"agreeing": host["rw_relations"][i, :, 0].tolist(),
                                           "tested": host["rw_relations"][i, :, 1].tolist()}}
            self.rows.append(row)
            if self.paths is not None:
                for name in SETS + (REWRITTEN_SET,):
                    if name in host:
                        self.files.submit(host[name][i], self.paths.of(name, image_id))


def _cut(batch, n):
    return [x[:n] if torch.is_tensor(x) else (None if x is None else list(x)[:n]) for x in batch]


def _open_writers(sampler, out_dir, image_format, num_writers):
    if image_format not in FORMATS:
        raise ValueError("image_format must be one of %s, got %r" % (" or ".join(repr(k) for k in FORMATS), image_format))
    files = FileWriter(num_writers, image_format) if out_dir else None
    return files, PictureWriter(sampler.device, files), (_Paths(out_dir, image_format) if out_dir else None)


def _host_ids(batch):
    """The object ids a batch carries on the host (loader.HostBatch), for the labels: they are never read back here."""
    ids = getattr(batch, "objs_host", None)
    if ids is None or tuple(ids.shape) != tuple(batch[1].shape):
        raise ValueError("draw_labels needs batches that carry their object ids on the host as `objs_host`, in the shape of "
                         "their objects (sg2im.data.loader.HostBatch, what a BatchBuilder yields): the ids are not read back")
    return ids


_NOT_MINIMAL = ("generate_split(rewrite=...): the batch holds rows that are not ORIGINAL (transitive or converse edges): build "
                "its batches with learned_transitivity = learned_converse = 0 at the dataset, so that a drawn edge is never "
                "mistaken for a source row; the checkpoint's own settings are applied to both graphs here")


class _RewriteWalk:
    """The robustness half of generate_split: per batch graph A and graph B (`graphs`), then B's layout and the three
    comparisons (`compare`); the running totals stay on the device until `summary`."""

    def __init__(self, rewrite, sampler, vocab, dev):
        import numpy as np
        self.rewrite, self.sampler, self.vocab, self.dev = rewrite, sampler, vocab, dev
        opt = sampler.opt
        self.transitivity = bool(getattr(opt, "learned_transitivity", False))
        self.converse = bool(getattr(opt, "learned_converse", False))
        self.weights = None
        if self.converse:
            from .sg2im.model import get_conv_converse
            self.weights = get_conv_converse(sampler.model).detach().cpu().numpy()
        self.random = np.random.RandomState(rewrite.seed)           # the converse draws: never numpy's global stream
        P = len(vocab["pred_name_to_idx"])
        self.iou_totals = torch.zeros(4, device=dev, dtype=torch.float64)
        self.rel_totals = torch.zeros((4, P, 2), device=dev, dtype=torch.int64)
        self.cons_f = torch.zeros(4, device=dev, dtype=torch.float64)
        self.cons_i = torch.zeros(20, device=dev, dtype=torch.int64)

    def graphs(self, batch, image_ids):
        """-> (triplets A, triplet_type A, (triplets B, triplet_type B))"""
        from . import ops
        from .sg2im.data.base_dataset import canonical_triplets
        objs, triplets, triplet_type = batch[1], batch[3], batch[5]
        host_objs = getattr(batch, "objs_host", None)
        if host_objs is None or tuple(host_objs.shape) != tuple(objs.shape):
            raise ValueError("generate_split(rewrite=...) needs batches that carry their object ids on the host as `objs_host` "
                             "(sg2im.data.loader.HostBatch, what a BatchBuilder yields): the objects per sample are not read back")
        n_objs = (host_objs[..., 0] != 0).sum(1).to(torch.int64) + 1          # the real objects and the `__image__` row
        rows, counts = ops.select_location_rows(triplets, triplet_type, self.vocab, num_objs=objs.shape[1])
        rows_b = ops.rewrite_rows(rows, counts, image_ids, self.vocab, self.rewrite.mode, self.rewrite.share,
                                  self.rewrite.direction, self.rewrite.seed)
        both = torch.cat([counts, (triplet_type != 0).any().to(torch.int64).view(1)]).cpu()     # the batch's one read-back
        if int(both[-1]):
            raise ValueError(_NOT_MINIMAL)
        counts_h = both[:-1]
        # a graph draws at most one number per original row, the dummies counted; both graphs see the same numbers
        uniforms = self.random.random_sample(int(counts_h.clamp(min=0).sum()) + int(n_objs.sum())) if self.converse else None
        made = [canonical_triplets(objs, None, None, n_objs, self.vocab, learned_transitivity=self.transitivity,
                                   learned_converse=self.converse, converse_weights=self.weights, uniforms=uniforms,
                                   triplets=r, triplet_counts=counts_h) for r in (rows, rows_b)]
        return made[0][0], made[0][2], (made[1][0], made[1][2])

    def compare(self, out, graph_b, objs, boxes, boxes_a, counted, triplets_a, triplet_type_a, image_id_obj, rescale, deprocess):
        """B's layout against the ground truth, against the clean graph and against A's layout; -> B's pictures"""
        from . import ops
        u8, boxes_b, _ = self.sampler.generate(objs, graph_b[0], graph_b[1], rescale=rescale, deprocess=deprocess)
        boxes_b = boxes_b.detach().float()
        iou_b = ops.box_iou(boxes_b, boxes, objs, image_id_obj, self.iou_totals)[0]
        agreement = ops.relation_agreement(boxes_b, triplets_a, triplet_type_a, self.vocab, self.rel_totals)[2]
        cons_iou, shift, _, pairs = ops.layout_consistency(boxes_a.detach().float(), boxes_b, counted, self.cons_f, self.cons_i)
        out.update({"rw_boxes_pred": boxes_b, "rw_iou": iou_b, "rw_cons_iou": cons_iou, "rw_shift": shift, "rw_pairs": pairs,
                    "rw_relations": agreement})
        return u8

    def summary(self):
        """The totals, read here once: what metrics["rewritten"] holds."""
        t, f, i = self.iou_totals.cpu(), self.cons_f.cpu().tolist(), self.cons_i.cpu().tolist()
        pair_relations = {name: {"in_a": i[3 * k], "in_b": i[3 * k + 1], "in_both": i[3 * k + 2],
                                 "kept": (i[3 * k + 2] / i[3 * k]) if i[3 * k] else None}
                          for k, name in enumerate(LOCATION_RELATIONS)}
        pair_relations.update({"same_pairs": i[18], "pairs": i[19], "same_share": (i[18] / i[19]) if i[19] else None})
        return {"avg_iou": float(t[0] / t[3]), "total_iou_05": float(t[1] / t[3]), "total_iou_03": float(t[2] / t[3]),
                "num_boxes": float(t[3]),
                "consistency": {"avg_iou": f[0] / f[3] if f[3] else None, "share_above_05": f[1] / f[3] if f[3] else None,
                                "avg_shift": f[2] / f[3] if f[3] else None},
                "pair_relations": pair_relations,
                "relation_agreement": relation_summary(self.rel_totals.cpu().tolist(), self.vocab)}


def generate_split(sampler, batches, out_dir=None, *, deprocess, rescale=True, draw_boxes=False, thickness=2,
                   image_format="png", num_writers=8, max_pictures=0, split=None, draw_labels=False, relations=False,
                   rewrite=None):
    """Walk `batches` (see the module docstring) -> (metrics, rows).  metrics: avg_iou, total_iou_05, total_iou_03 (the
    totals / counted boxes, float64, as Evaluator.check_model forms them) and num_boxes; empty for a model without a graph
    part.  With `out_dir` the pictures and layouts.json are written; without it only metrics and rows are made.
    `max_pictures`: stop after that many images (a batch may be cut; 0: all).  `split`: the name layouts.json records.
    `draw_labels` (needs `draw_boxes`): the objects' names on layout/gt and layout/pred (ops.draw_labels_u8, names by
    authored.labels_from_objs from the ids the batch holds on the host).
    `relations` (opt-in; without it nothing below is made and every output is as before): whether the PREDICTED layout
    obeys the triplets it was made from (ops.relation_agreement on boxes_pred, box centres, in the loop and without a
    read-back): every row gets `relation_agreement` = {agreeing, tested} by triplet type, and metrics gets
    `relation_agreement` (`relation_summary`) from one int64 (4,P,2) buffer of totals read once at the end.
    `rewrite` (a `Rewrite`; opt-in; without it every output is as before, key for key): the robustness walk.  The batches
    must carry the plain minimal graph (the dataset's learned_transitivity and learned_converse off; a batch with a row
    that is not ORIGINAL is refused) and their object ids on the host (`objs_host`).  Per batch the graph's location rows
    are selected (ops.select_location_rows; the one read-back of the counts), graph A is built from them and graph B from
    the rewritten rows (ops.rewrite_rows), both by canonical_triplets(boxes=None, ...) with the checkpoint's
    learned_transitivity / learned_converse and the same converse draws, from a np.random.RandomState(seed).  Everything
    above — pictures, boxes_pred, IoU, relations — is then made of graph A; graph B gets its own Sampler.generate,
    ops.box_iou against the ground truth, ops.relation_agreement of its boxes against A's triplets (the clean graph) and
    ops.layout_consistency(A, B).  Every row gains `rewritten` = {boxes_pred, iou, consistency_iou, shift, pair_relations,
    relation_agreement}, metrics gains `rewritten` (its totals, read once at the end; `robustness_report` makes
    robustness.json of both), and with `out_dir` B's pictures go to generation/pred_box_pred_mask_rewritten/."""
    from . import ops
    from .sample import NO_CPU
    from .sg2im.data.loader import HostBatch
    if draw_labels and not draw_boxes:
        raise ValueError("generate_split(draw_labels=True) needs draw_boxes=True: the names go on the layout pictures")
    if sampler.device.type != "cuda":
        raise RuntimeError(NO_CPU)
    if deprocess not in ops.DEPROCESS:
        raise ValueError("generate_split: deprocess must be one of %s, got %r" % (
            " or ".join(repr(k) for k in ops.DEPROCESS), deprocess))
    model, vocab, dev = sampler.model, sampler.opt.vocab, sampler.device
    image_id_obj = vocab["object_name_to_idx"]["__image__"]
    files, pictures, paths = _open_writers(sampler, out_dir, image_format, num_writers)
    totals = torch.zeros(4, device=dev, dtype=torch.float64)
    relations = bool(relations) and model.has_graph
    rel_totals = torch.zeros((4, len(vocab["pred_name_to_idx"]), 2), device=dev, dtype=torch.int64) if relations else None
    palette = torch.tensor(authored.DEFAULT_PALETTE, dtype=torch.uint8).reshape(-1, 3).to(dev) if draw_boxes else None
    rw = None
    if rewrite is not None:
        if not model.has_graph:
            raise ValueError("generate_split(rewrite=...) needs a model with a graph part: it compares predicted layouts")
        rw = _RewriteWalk(rewrite.check(), sampler, vocab, dev)
    taker = SplitRows(vocab, files, paths)
    rows, done = taker.rows, 0
    raising = True
    try:
        with torch.no_grad():
            for batch in batches:
                if files is not None:
                    files.check()
                if max_pictures and done + int(batch[1].shape[0]) > max_pictures:
                    n = max_pictures - done
                    batch = HostBatch(_cut(batch, n), batch.objs_host[:n]) if hasattr(batch, "objs_host") else _cut(batch, n)
                imgs, objs, boxes, triplets, _, triplet_type, masks, image_ids = batch
                if not objs.is_cuda:
                    raise RuntimeError(NO_CPU)
                names = authored.labels_from_objs(_host_ids(batch), vocab) if draw_labels else None
                if rw is not None:                      # graph A takes the batch's place; graph B is kept for below
                    triplets, triplet_type, graph_b = rw.graphs(batch, torch.as_tensor(image_ids).to(dev).reshape(-1).to(torch.int64))
                out = {}
                u8 = sampler.generate(objs, triplets, triplet_type, boxes_gt=boxes, masks_gt=masks, rescale=rescale,
                                      deprocess=deprocess)[0]
                if u8 is not None:
                    out["generation/gt_box_gt_mask"] = u8
                boxes_pred = None
                if model.has_graph:
                    u8, boxes_pred, _ = sampler.generate(objs, triplets, triplet_type, rescale=rescale, deprocess=deprocess)
                    if u8 is not None:
                        out["generation/pred_box_pred_mask"] = u8
                if imgs is not None:
                    out["gt"] = ops.deprocess_u8(imgs.float().contiguous(memory_format=torch.channels_last), rescale, deprocess)
                if draw_boxes:
                    if "gt" in out:
                        out["layout/gt"] = ops.draw_boxes_u8(out["gt"], boxes.float(), objs, image_id_obj, palette, thickness)
                    if "generation/pred_box_pred_mask" in out:
                        out["layout/pred"] = ops.draw_boxes_u8(out["generation/pred_box_pred_mask"], boxes_pred.detach().float(),
                                                               objs, image_id_obj, palette, thickness)
                    for name, bx in (("layout/gt", boxes), ("layout/pred", boxes_pred)):
                        if draw_labels and name in out:
                            out[name] = ops.draw_labels_u8(out[name], bx.detach().float(), objs, image_id_obj, palette, names)
                if paths is None:
                    out = {}                            # nothing to write: the pictures stay where they are
                ids = image_ids if torch.is_tensor(image_ids) else torch.as_tensor(image_ids)
                out.update({"image_id": ids.to(dev, non_blocking=True).reshape(-1).to(torch.int64), "objs": objs,
                            "boxes": boxes.float()})
                if boxes_pred is not None:
                    iou, counted, _ = ops.box_iou(boxes_pred, boxes, objs, image_id_obj, totals)
                    out.update({"boxes_pred": boxes_pred.detach().float(), "iou": iou, "counted": counted})
                    if relations:
                        out["relations"] = ops.relation_agreement(boxes_pred.detach().float(), triplets, triplet_type, vocab,
                                                                  rel_totals)[2]
                    if rw is not None:
                        u8 = rw.compare(out, graph_b, objs, boxes, boxes_pred, counted, triplets, triplet_type, image_id_obj,
                                        rescale, deprocess)
                        if u8 is not None and paths is not None:
                            out[REWRITTEN_SET] = u8
                pictures.put(out, taker.take)
                done += int(objs.shape[0])
                if max_pictures and done >= max_pictures:
                    break
            pictures.flush()
            metrics = {}
            if model.has_graph and rows:
                t = totals.cpu()                        # the one read of the totals, at the end
                metrics = {"avg_iou": float(t[0] / t[3]), "total_iou_05": float(t[1] / t[3]), "total_iou_03": float(t[2] / t[3]),
                           "num_boxes": float(t[3])}
                if relations:
                    metrics["relation_agreement"] = relation_summary(rel_totals.cpu().tolist(), vocab)
                if rw is not None:
                    metrics["rewritten"] = rw.summary()
        raising = False
    finally:
        if files is not None:
            files.close(reraise=not raising)            # an error already on its way is not replaced by the writer's
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "layouts.json"), "w") as f:
            json.dump({"dataset": getattr(sampler.opt, "dataset", None), "split": split,
                       "image_size": [int(v) for v in sampler.opt.image_size], "deprocess": deprocess, "rescale": bool(rescale),
                       "metrics": metrics, "images": rows}, f)
    return metrics, rows


EDGE_TYPES = ("original", "transitive", "symmetric", "anti_symmetric")      # triplet types 0..3 (sg2im/data/base_dataset.py)


def _rate(agreeing, tested):
    return {"agreeing": int(agreeing), "tested": int(tested), "rate": (agreeing / tested) if tested else None}


def relation_summary(totals, vocab):
    """The (4,P,2) totals of ops.relation_agreement as nested lists -> {agreeing, tested, rate, by_type: {name: ...},
    by_predicate: {name: ...}} (the predicates that were tested at least once; `rate` is None where nothing was)."""
    names = vocab["pred_idx_to_name"]
    by_type = {EDGE_TYPES[k]: _rate(sum(c[0] for c in totals[k]), sum(c[1] for c in totals[k])) for k in range(4)}
    by_pred = {names[p]: _rate(sum(totals[k][p][0] for k in range(4)), sum(totals[k][p][1] for k in range(4)))
               for p in range(len(names))}
    return dict(_rate(sum(v["agreeing"] for v in by_type.values()), sum(v["tested"] for v in by_type.values())),
                by_type=by_type, by_predicate={k: v for k, v in by_pred.items() if v["tested"]})


def generalisation_report(metrics, rows, **run):
    """What the large-graph run reports (generalisation.json), on the host from `generate_split(relations=True)`'s two
    results: the overall figures, relation agreement by triplet type and by predicate, and both again by the number of
    objects in the graph — `by_num_objects`, the curve the experiment is about — summed from the per-image rows.  `run`:
    what identifies the run (seed or scenes file, checkpoint), recorded as given."""
    sizes = {}
    for row in rows:
        sizes.setdefault(len(row["objects"]), []).append(row)
    by_size = {}
    for n in sorted(sizes):
        ious = [v for row in sizes[n] for v in row.get("iou", [])]
        entry = {"images": len(sizes[n]), "num_boxes": len(ious)}
        if ious:
            entry.update({"avg_iou": sum(ious) / len(ious), "total_iou_05": sum(v > 0.5 for v in ious) / len(ious),
                          "total_iou_03": sum(v > 0.3 for v in ious) / len(ious)})
        if any("relation_agreement" in row for row in sizes[n]):
            per = [row["relation_agreement"] for row in sizes[n]]
            by_type = {EDGE_TYPES[k]: _rate(sum(r["agreeing"][k] for r in per), sum(r["tested"][k] for r in per))
                       for k in range(4)}
            entry["relation_agreement"] = dict(_rate(sum(v["agreeing"] for v in by_type.values()),
                                                     sum(v["tested"] for v in by_type.values())), by_type=by_type)
        by_size[str(n)] = entry
    out = dict(run)
    out.update({"images": len(rows), "metrics": {k: v for k, v in metrics.items() if k != "relation_agreement"},
                "relation_agreement": metrics.get("relation_agreement"), "by_num_objects": by_size})
    return out


def _iou_figures(ious):
    n = len(ious)
    if not n:
        return {"num_boxes": 0}
    return {"num_boxes": n, "avg_iou": sum(ious) / n, "total_iou_05": sum(v > 0.5 for v in ious) / n,
            "total_iou_03": sum(v > 0.3 for v in ious) / n}


def _pair_figures(per):
    """[a row's rewritten.pair_relations] -> their sums, with kept = in_both / in_a and same_share = same_pairs / pairs"""
    out = {}
    for name in LOCATION_RELATIONS:
        a, b, both = (sum(p[name][k] for p in per) for k in ("in_a", "in_b", "in_both"))
        out[name] = {"in_a": a, "in_b": b, "in_both": both, "kept": (both / a) if a else None}
    same, pairs = sum(p["same_pairs"] for p in per), sum(p["pairs"] for p in per)
    out.update({"same_pairs": same, "pairs": pairs, "same_share": (same / pairs) if pairs else None})
    return out


def robustness_report(metrics, rows, **run):
    """What the robustness run reports (robustness.json), on the host from `generate_split(rewrite=...)`'s two results.
    `run`: what identifies the run — mode, share, direction, seed of the rewrite, checkpoint, scenes — recorded as given.
    `clean` and `rewritten`: avg_iou, total_iou_05, total_iou_03 against the ground truth for the layout of graph A and of
    graph B; `consistency` = {avg_iou, share_above_05, avg_shift} of B's boxes against A's; `pair_relations` = per location
    predicate {in_a, in_b, in_both, kept = in_both / in_a} over the ordered pairs of objects, and same_pairs / pairs;
    `relation_agreement`: of the rewritten layout with the CLEAN graph.  `by_num_objects`: every figure again by the number
    of objects in the graph, summed from the per-image rows (the fp64 averages of a size are the host's sums of the rows'
    fp32 values; the overall ones are the device's totals)."""
    rewritten = metrics.get("rewritten")
    if rewritten is None or any("rewritten" not in row for row in rows):
        raise ValueError("robustness_report: metrics and rows of generate_split(rewrite=...) are needed")
    sizes = {}
    for row in rows:
        sizes.setdefault(len(row["objects"]), []).append(row)
    by_size = {}
    for n in sorted(sizes):
        group = [row["rewritten"] for row in sizes[n]]
        cons, shift = [v for r in group for v in r["consistency_iou"]], [v for r in group for v in r["shift"]]
        by_type = {EDGE_TYPES[k]: _rate(sum(r["relation_agreement"]["agreeing"][k] for r in group),
                                        sum(r["relation_agreement"]["tested"][k] for r in group)) for k in range(4)}
        by_size[str(n)] = {
            "images": len(group), "clean": _iou_figures([v for row in sizes[n] for v in row["iou"]]),
            "rewritten": _iou_figures([v for r in group for v in r["iou"]]),
            "consistency": {"avg_iou": sum(cons) / len(cons), "share_above_05": sum(v > 0.5 for v in cons) / len(cons),
                            "avg_shift": sum(shift) / len(shift)} if cons else None,
            "pair_relations": _pair_figures([r["pair_relations"] for r in group]),
            "relation_agreement": dict(_rate(sum(v["agreeing"] for v in by_type.values()),
                                             sum(v["tested"] for v in by_type.values())), by_type=by_type)}
    iou_keys = ("avg_iou", "total_iou_05", "total_iou_03", "num_boxes")
    out = dict(run)
    out.update({"images": len(rows), "clean": {k: metrics[k] for k in iou_keys}, "rewritten": {k: rewritten[k] for k in iou_keys},
                "consistency": rewritten["consistency"], "pair_relations": rewritten["pair_relations"],
                "relation_agreement": rewritten["relation_agreement"], "by_num_objects": by_size})
    return out


def generate_layouts(sampler, rows, which="pred", out_dir=None, *, deprocess, rescale=True, batch_size=None,
                     image_format="png", num_writers=8, draw_labels=False, thickness=2):
    """Pictures from layout rows with the generator alone (the reference's generation_dataframe.py --mode pred|gt): the
    rows' objects go through the sampler's vocabulary, `batch_size` rows (default --batch_size) at a time in file order, and
    `sampler.generate(objs, None, None, boxes_gt=boxes)` sees the tensors a dataset batch would give (`layout_batch`).
    With `out_dir` the pictures go to generation/<which>_box_<which>_mask/<image_id>.<ext> and the number written is
    returned; without it the pictures are returned, uint8 (N,3,H,W) on the host.  Every row is checked first
    (`encode_layouts`): nothing is launched for a file with a bad row.
    `draw_labels`: besides, every picture under the outlines and the names of its boxes (ops.draw_boxes_u8, then
    ops.draw_labels_u8; palette and thickness of generate_split; the names are the rows' own, authored.object_labels) in
    layout/<which>/<image_id>.<ext>, as generate_split's layout/gt and layout/pred; without `out_dir` the pair (pictures,
    labelled pictures) is returned."""
    from . import ops
    from .sample import NO_CPU
    if deprocess not in ops.DEPROCESS:
        raise ValueError("generate_layouts: deprocess must be one of %s, got %r" % (
            " or ".join(repr(k) for k in ops.DEPROCESS), deprocess))
    samples = encode_layouts(rows, which, sampler.opt.vocab)
    if sampler.device.type != "cuda":
        raise RuntimeError(NO_CPU)
    step = int(batch_size or sampler.opt.batch_size)
    if step < 1:
        raise ValueError("generate_layouts: batch_size must be positive")
    name = "generation/%s_box_%s_mask" % (which, which)
    files, pictures, paths = _open_writers(sampler, out_dir, image_format, num_writers)
    kept, kept_layouts = [], []
    vocab = sampler.opt.vocab
    palette = torch.tensor(authored.DEFAULT_PALETTE, dtype=torch.uint8).reshape(-1, 3).to(sampler.device) if draw_labels else None

    def on_host(host):
        for i, image_id in enumerate(host["ids"]):
            if paths is None:
                kept.append(torch.from_numpy(host["u8"][i]).clone())
                if "layout" in host:
                    kept_layouts.append(torch.from_numpy(host["layout"][i]).clone())
            else:
                files.submit(host["u8"][i], paths.of(name, image_id))
                if "layout" in host:
                    files.submit(host["layout"][i], paths.of("layout/%s" % which, image_id))

    raising = True
    try:
        for first in range(0, len(samples), step):
            if files is not None:
                files.check()
            chunk = samples[first:first + step]
            objs, boxes = layout_batch(chunk, vocab)
            objs, boxes = objs.to(sampler.device), boxes.to(sampler.device)
            u8 = sampler.generate(objs, None, None, boxes_gt=boxes, rescale=rescale, deprocess=deprocess)[0]
            if u8 is None:
                raise RuntimeError("generate_layouts needs a model that generates pictures (--skip_generation 0)")
            ids = [s[0] for s in chunk]
            out = {"u8": u8}
            if draw_labels:
                image_id_obj = vocab["object_name_to_idx"]["__image__"]
                out["layout"] = ops.draw_labels_u8(ops.draw_boxes_u8(u8, boxes, objs, image_id_obj, palette, thickness), boxes,
                                                   objs, image_id_obj, palette, authored.object_labels(rows[first:first + step]))
            pictures.put(out, lambda host, ids=ids: on_host(dict(host, ids=ids)))
        pictures.flush()
        raising = False
    finally:
        if files is not None:
            files.close(reraise=not raising)
    if paths is not None:
        return len(samples)
    return (torch.stack(kept), torch.stack(kept_layouts)) if draw_labels else torch.stack(kept)
