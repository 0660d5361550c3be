"""The device half of the packed datasets' collate: objects and boxes in, the trainer's batch with its canonical graph out."""
import torch


def packed_batch(args, trainer, batch, dev, counts=None, centers=None):
    """A packed batch (the tensors of synth.make_batch or of a dataset's batch builder, on the host or on `dev`) on `dev`,
    with the canonical graph built on the device: the __image__ row appended to every sample, then canonical_triplets in
    place of the triplets.  packed_vg hands the batch's annotated relationships over, unless --include_relationships 0
    (packed_vg.py:128-130).  `counts`: the real objects per sample as a HOST int64 tensor, from a builder that knows them
    (its objects live on the device: deriving the counts from them would be a read-back per batch); by default they are
    derived from the objects, as before.  The unpacked coco dataset hands over, in the triplet slot, the pairs its builder
    drew: (other, flip) on the device and their host copies (None with --include_relationships 0: the dummies alone,
    sg2im/data/coco.py:374-375); its graph is the sampled rows, not the all-pairs relations of the geometry.  The unpacked vg
    dataset hands over its annotated rows, on the device and on the host: they and the dummies are its whole graph
    (sg2im/data/vg.py:136-149), built by annotated_triplets.  The unpacked clevr dataset hands over the renderer's relation
    rows the same way, and the objects per sample on the device besides: clevr_triplets reduces them per predicate
    (sg2im/data/clevr_dialog.py:289-307; the dummies alone with --include_relationships 0), and the `__image__` row, which
    follows a sample's objects, has the box (0, 0, 1, 1) (clevr_dialog.py:176-179) where every other dataset's has -1.
    `centers`: fp32 (B,O,2) object centres of the rows handed over, from a builder that has better ones than the box centres
    (the COCO datasets' mask centroids, ops.coco_masks); they replace x0 + 0.5 * w for those rows — the appended `__image__`
    row keeps its value — and reach canonical_triplets and, for coco, ops.pair_relations.  The batch's masks, if any, come
    with their `__image__` row already in place."""
    from . import annotated_triplets, canonical_triplets, clevr_triplets
    rel = pairs = rows = None
    if args.dataset == "clevr":
        if counts is None:
            raise ValueError("packed_batch: a clevr batch comes from ClevrDialogBatchBuilder, with the objects per sample")
        batch = list(batch)
        (*rows, counts_dev), batch[3] = batch[3], None
        if not args.include_relationships:
            rows = tuple(t[:, :0] for t in rows)
        n = counts + 1
    if args.dataset == "vg":
        if counts is None:
            raise ValueError("packed_batch: a vg batch comes from VGAnnotatedBatchBuilder, with the objects per sample")
        batch = list(batch)
        rows, batch[3] = batch[3], None
        if not args.include_relationships:                 # vg.py:138-139
            rows = tuple(t[:, :0] for t in rows)
        n = counts + 1
    if args.dataset == "coco":
        if counts is None:
            raise ValueError("packed_batch: a coco batch comes from CocoPairsBatchBuilder, with the objects per sample")
        batch = list(batch)
        pairs, batch[3] = batch[3], None
        n = counts + 1
        if pairs is None:
            rel = torch.zeros((counts.shape[0], 0, 3), dtype=torch.int64)
    if args.dataset == "packed_vg":  # the annotated rows and the object counts are read on the host: hand over CPU tensors
        rel = batch[3] if args.include_relationships else torch.zeros((batch[3].shape[0], 0, 3), dtype=torch.int64)
        n = (batch[1][..., 0] != 0).sum(1) if counts is None else counts
        n = n + 1                                           # real objects + the __image__ row appended below
    batch = [None if x is None else x.to(dev) for x in batch]
    objs, boxes = batch[1], batch[2]
    if rel is None and pairs is None and rows is None:
        n = ((objs[..., 0] != 0).sum(1) if counts is None else counts.to(dev)) + 1
    O = objs.shape[1] + 1
    objs = torch.cat([objs, objs.new_zeros(objs.shape[0], 1, objs.shape[2])], 1)
    boxes = torch.cat([boxes, boxes.new_full((boxes.shape[0], 1, 4), -1.0)], 1)
    batch[1], batch[2] = objs, boxes
    if args.dataset == "clevr":                            # row counts[b] of sample b is its __image__ row; -1 boxes after it
        counts_dev = counts_dev.to(dev)
        image_row = (torch.arange(O, device=dev)[None] == counts_dev[:, None])[..., None]
        boxes[..., :2].masked_fill_(image_row, 0.0)
        boxes[..., 2:].masked_fill_(image_row, 1.0)
        batch[3], batch[4], batch[5] = clevr_triplets(objs, counts_dev + 1, args.vocab, rows[0].contiguous(),
                                                      rows_host=rows[1].contiguous(), n_objs_host=n,
                                                      use_transitivity=int(args.use_transitivity))
        assert batch[3].shape[1] > 0 and objs.shape[1] == O
        return batch
    if centers is None:
        centers = boxes[..., :2] + 0.5 * boxes[..., 2:]
    else:
        if args.dataset in ("clevr", "vg") or tuple(centers.shape) != (objs.shape[0], O - 1, 2):
            raise ValueError("packed_batch: centers must be (B, O, 2) for the %d x %d rows handed over, and the dataset one "
                             "whose graph has location relations" % (objs.shape[0], O - 1))
        centers = torch.cat([centers.to(dev), boxes[:, O - 1:, :2] + 0.5 * boxes[:, O - 1:, 2:]], 1)
    extra = {"triplets": rel}
    if args.dataset == "coco":
        if pairs is None:                                  # no geometry: the (empty) rows are the whole graph
            boxes = centers = None
        else:                                              # the __image__ row draws nothing
            extra = {"pairs": tuple(torch.nn.functional.pad(t.to(dev), (0, 1), value=v) for t, v in zip(pairs[:2], (-1, 0))),
                     "pairs_host": tuple(torch.nn.functional.pad(t, (0, 1), value=v) for t, v in zip(pairs[2:], (-1, 0))),
                     "use_converse": bool(args.use_converse)}
    conv_w = None
    if args.learned_converse:    # the data loader reads the model's converse weights back (scripts/train.py:274-276)
        from ..model import get_conv_converse
        conv_w = get_conv_converse(trainer.model).detach().cpu().numpy()
    if rows is not None:
        batch[3], batch[4], batch[5] = annotated_triplets(objs, n, args.vocab, rows[0].contiguous(),
                                                          rows_host=rows[1].contiguous(),
                                                          learned_transitivity=bool(args.learned_transitivity),
                                                          learned_converse=bool(args.learned_converse),
                                                          converse_weights=conv_w)
        assert batch[3].shape[1] > 0 and objs.shape[1] == O
        return batch
    batch[3], batch[4], batch[5] = canonical_triplets(objs, boxes, centers, n, args.vocab,
                                                      learned_transitivity=bool(args.learned_transitivity),
                                                      learned_converse=bool(args.learned_converse),
                                                      converse_weights=conv_w, **extra)
    assert batch[3].shape[1] > 0 and objs.shape[1] == O
    return batch
