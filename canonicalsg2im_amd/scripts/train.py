"""Command-line trainer for the HIP hot path, on a COCO, CLEVR or Visual Genome folder or on SYNTHETIC batches.

The reference's scripts/train.py owns data loading, logging, evaluation and checkpoint policy; of it only the
iteration (:353-393, :468-485) is on the hot path and lives in `canonicalsg2im_amd.train.Trainer`.  This entry point
drives that iteration with the reference's flags, one process per GPU:

    python -m canonicalsg2im_amd.scripts.train --dataset packed_clevr --image_size 256,256 --batch_size 48 \\
        --num_iterations 100 --no_vgg_loss --learned_transitivity 1
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m canonicalsg2im_amd.scripts.train ...

Data.  `--dataset packed_coco` trains on real pictures when the train image directory exists (`--coco_train_image_dir`, by
default <dataroot>/MSCoco/images/train2017 with the annotation files beside it, the reference's layout): the pictures are
decoded on the host in `--loader_num_workers` threads and resized, converted and normalised on the device, one batch ahead of
the step (sg2im/data/packed_coco.py of this package; `--mask_size` must be 0 there unless `--coco_segmentations 1` decodes
the annotations' segmentations on the device: masks in the batch, mask centroids as centres).  Every epoch is a permutation seeded by
the epoch number; with N ranks each takes every N-th sample of a global batch.  `--dataset packed_clevr` does the same when
its train image directory exists (`--clevr_train_image_dir`, by default <dataroot>/CLEVR/CLEVR_Dialog/images/train with
scenes/CLEVR_train_scenes.json beside `images`): the renders go up as decoded, RGBA included, and the boxes are computed on
the device from the scene geometry (sg2im/data/packed_clevr.py of this package; `--mask_size` must be 0 there too).
`--dataset packed_vg` does the same when its image directory and its split file exist (`--vg_image_dir`, `--train_h5`,
`--vocab_json` where they exist, else <dataroot>/vg/{images, train.h5 or train.npz, vocab.json}): the objects of a sample are
chosen on the host as the reference chooses them, their pixel boxes are divided by the decoded picture's size on the device,
and the annotated relationships join the canonical graph (sg2im/data/packed_vg.py of this package; `--mask_size` must be 0;
a .h5 split needs h5py, a .npz split does not: tools/vg_h5_to_npz.py).  `--dataset coco`, the default, reads the COCO folder
of `packed_coco` with the original sg2im graph: 3 to 8 objects, every object draws one partner on the host and the pair's
predicate and the graph are made on the device (sg2im/data/coco.py of this package; `--mask_size` must be 0 unless
`--coco_segmentations 1`, as for `packed_coco`; `--coco_val_ids`
names the val split's image ids).  `--dataset vg` reads the unpacked Visual Genome folder, <dataroot>/VisualGenome with the
pictures, train.h5 or train.npz and vocab.json in it (or `--vg_image_dir`, `--train_h5`, `--vocab_json` where they exist), with
`packed_vg`'s object choice and boxes and the reference's annotated-only graph: the annotated relationships and the dummies,
no location relation, at most 63 objects per picture (sg2im/data/vg.py of this package; `--mask_size` must be 0).
`--dataset clevr` reads the CLEVR folder of `packed_clevr` with the reference's CLEVR-Dialog graph: the scene file's own
relationships, every predicate's reduced to its minimal graph on the device, and the dummies; six predicates, at most 63
objects per scene (sg2im/data/clevr.py of this package; `--use_transitivity` is 0 or 1, the learned flags, `--use_converse` and
`--mask_size` above 0 are refused).  Without the directory, and for `--dataset synthetic`,
the batches are seeded synthetic ones of the chosen dataset's shape.  One line says which of the two it is.

For packed datasets the scene graphs are built on the device from the boxes (`sg2im.data.canonical_triplets`), as
the packed data loaders do on the host; `packed_vg` batches carry annotated relationships (the split file's, or synthetic
ones among the vocabulary's non-location predicates) that join the graph as in sg2im/data/packed_vg.py:127-142.

`--val_every N` (default 0: off) runs the reference's two validation passes (scripts/train.py:410-424, `GT VAL` and `VAL`)
every N iterations on the validation set of scripts/evaluate.py: the first `--num_val_samples` pictures of the val split
when its directory exists, seeded synthetic batches (seeds disjoint from the training seeds) otherwise.  With N > 1 ranks
every rank validates the SAME batches and rank 0 prints: the passes advance the discriminators' spectral-norm vectors and
BatchNorm statistics (evaluate.py), which must stay identical across ranks, and no collective is issued.

`--ema_decay D` (default 0: off; 0 < D <= 1) keeps an exponential moving average of the whole generator model's weights
(canonicalsg2im_amd/ema.py): one launch per iteration after the optimiser steps, `--ema_warmup 1` (default) with the decay
min(D, (1 + n) / (10 + n)) at update n.  Checkpoints then carry `model_ema_state` and `ema` besides today's keys, and a
restored run continues the average (a checkpoint without them starts it from the restored weights).  `--val_ema 1` (default
0; needs --ema_decay) runs the validation passes of --val_every on the averaged weights, swapped in for the passes and out
again; their lines read `EMA GT VAL` and `EMA VAL`.

`--d_augment POLICIES` (default empty: off) transforms everything the PatchGAN and the object-crop discriminator see during
training with DiffAugment (canonicalsg2im_amd/d_augment.py): a comma list out of color,translation,cutout, anything else is
refused.  `--d_augment_seed N` (default 0) keys the counter-based hash the transforms' parameters come from; there is no RNG
state.  Both flags are part of the run's argument namespace; checkpoints then carry `d_augment` = {seed, iteration, policies}
and a restored run continues the parameter stream.  Validation and sampling see raw inputs.

`--d_augment_p P`, `--d_augment_target T`, `--d_augment_interval K` (default 4), `--d_augment_kimg M` (default 500) gate the
policies per sample with probability p (StyleGAN2-ADA): T = 0 (default) keeps p = P (default 1); 0 < T < 1 (the paper uses
0.6) steers p, starting from P (default 0), so that r_t = E[sign(D(real))] — taken per PatchGAN output element, over all
scales — stays at T: every K iterations p moves by B K / (1000 M) towards it, B the pictures of one iteration over all ranks.  Any of the four without
--d_augment policies is refused.  The controller lives on the device and is read back here only: every --print_every a line
`d_augment: p %.4f r_t %.4f` follows the loss line.  Checkpoints carry its eight words and the four settings in `d_augment`.

`--d_augment` also takes `ada_blit` (x-flip, rot90, integer translation), `ada_geom` (isotropic scale, rotation, anisotropic
scale, rotation, fractional translation) and `ada_color` (brightness, contrast, luma flip, hue, saturation): StyleGAN2-ADA's
own pipeline, one more launch in front of the DiffAugment kernel.  Each transform is applied with probability p, so these names
are refused without `--d_augment_p` or a non-zero `--d_augment_target` (at p = 1 they leak into the generator).  Checkpoints
carry the names in `d_augment.policies`."""
import os
import sys
import time

import torch


def _vocab_kind(dataset):
    return {"vg": "vg", "packed_vg": "vg", "clevr": "clevr", "packed_clevr": "clevr", "packed_clevr_syn": "clevr"}.get(dataset, "coco")


def packed_batch(args, trainer, batch, dev):
    """sg2im.data.collate.packed_batch, its home since the folder dataset shares it (imported there on first use: this
    module parses command lines without the library)."""
    from ..sg2im.data.collate import packed_batch as impl
    return impl(args, trainer, batch, dev)


def folder_dataset(args, split):
    """The dataset of `split` when --dataset names a folder dataset whose image directory exists, None otherwise: the batches
    are then synthetic."""
    from ..sg2im.data import build_folder_dataset
    return build_folder_dataset(args, split)


def hold_to_vocab(ds, vocab, split):
    """Refuse, on the host, a folder dataset whose categories, attribute tables or predicates differ from `vocab`, the
    vocabulary the model was built with: its ids would index the model's embedding tables.  -> ds"""
    if ds is None or vocab is None:
        return ds
    if ds.vocab["attributes"] != vocab["attributes"] and ds.vocab["object_name_to_idx"] == vocab["object_name_to_idx"]:
        raise SystemExit("the %s split's attribute tables (%s rows) are not the model's (%s rows): train and validate on one "
                         "vocabulary" % (split, [len(t) for t in ds.vocab["attributes"].values()],
                                         [len(t) for t in vocab["attributes"].values()]))
    if "pred_idx_to_name" in vocab and list(ds.vocab["pred_idx_to_name"]) != list(vocab["pred_idx_to_name"]):
        raise SystemExit("the %s split's predicates (%d names) are not the model's (%d names): train and validate on one "
                         "vocabulary" % (split, len(ds.vocab["pred_idx_to_name"]), len(vocab["pred_idx_to_name"])))
    if ds.vocab["object_name_to_idx"] != vocab["object_name_to_idx"]:
        raise SystemExit("the %s split's categories (%d names, largest id %d) are not the model's (%d names, largest id %d): "
                         "train and validate on annotation files of one category set" % (
                             split, len(ds.vocab["object_name_to_idx"]), max(ds.vocab["object_name_to_idx"].values()),
                             len(vocab["object_name_to_idx"]), max(vocab["object_name_to_idx"].values())))
    return ds


def folder_builder(dataset, args, trainer, dev, rng=None):
    """The batch builder of a folder dataset, with --loader_num_workers threads.  `rng`: where a Visual Genome builder draws
    its object sampling (by default its own random.Random, seeded from the rank); the other datasets draw nothing."""
    cls = dataset.builder_class
    return cls(dataset, args, trainer, dev, num_workers=args.loader_num_workers, **({"rng": rng} if cls.takes_rng else {}))


def synth_config(args, batch_size):
    """The synth.BatchConfig of the seeded synthetic batches of --dataset's shape."""
    from ..synth import BatchConfig
    packed = args.dataset.startswith("packed")
    lo = args.min_objects or (16 if packed else 3)
    hi = args.max_objects or (40 if packed else 8)
    graph = ("annotated" if args.dataset == "packed_vg" else "packed") if packed else "random"
    return BatchConfig(batch_size, args.image_size[0], lo, hi, graph, mask_size=args.mask_size)


def validate_in_training(args, trainer, evaluator, dev, t, world=1, val_set=None):
    """The validation passes of --val_every.  With --val_ema 1 they run on the averaged weights: inside
    `trainer.ema.swapped()` (one swap launch and a cache invalidation on each side), with the evaluator's sampler — which
    adopted the trainer's model and keeps W / sigma and packed operands of its own — invalidated on both sides as well."""
    from . import evaluate as val_cli
    if not getattr(args, "val_ema", 0):
        return val_cli.validate(args, evaluator, dev, t, world, val_set)
    if trainer.ema is None:
        raise RuntimeError("--val_ema 1 needs a trainer with --ema_decay")
    with trainer.ema.swapped():
        evaluator.sampler.invalidate()
        try:
            return val_cli.validate(args, evaluator, dev, t, world, val_set, prefix="EMA ")
        finally:
            evaluator.sampler.invalidate()


def build_parser():
    from .args import build_parser as base_parser
    p = base_parser()
    p.add_argument('--val_every', default=0, type=int)
    p.add_argument('--val_ema', default=0, type=int, choices=[0, 1])
    return p


def argparse_copy(args, **changes):
    """A shallow copy of the namespace with some entries replaced."""
    import argparse
    out = argparse.Namespace(**vars(args))
    for k, v in changes.items():
        setattr(out, k, v)
    return out


def main(argv=None):
    from .. import dist as csg_dist, train as T
    from ..synth import make_batch, make_vocab
    from .args import init_args
    args = build_parser().parse_args(argv)
    if args.val_every < 0:
        raise SystemExit("--val_every must be >= 0 (0: no validation)")
    if args.val_ema and not args.ema_decay:
        raise SystemExit("--val_ema 1 needs --ema_decay D (0 < D <= 1): there are no averaged weights to validate")
    if args.dataset == "packed_clevr_syn":
        from ..sg2im.data.packed_clevr_syn import NO_TRAINING
        raise SystemExit(NO_TRAINING)
    rank, world, local = csg_dist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    from ..sg2im.data.loader import epoch_batches
    train_set = folder_dataset(args, "train")
    args.vocab = train_set.vocab if train_set is not None else make_vocab(_vocab_kind(args.dataset))
    if world > 1:
        args.gpu_ids = ",".join(str(i) for i in range(world))
    init_args(args)
    per_rank = args.batch_size // max(world, 1)
    torch.manual_seed(0)
    trainer = T.Trainer(args, dev)
    if trainer.d_augment is not None:
        # --batch_size is the GLOBAL batch here: the strength controller's step counts it once, not once per rank
        trainer.d_augment.set_pictures_per_iteration(per_rank * max(world, 1))
    t0 = epoch = 0
    if args.restore_checkpoint:
        # scripts/train.py:29-60: `--checkpoint_name` is the PATH of the checkpoint file; a failed restore raises
        if not args.checkpoint_name or not os.path.isfile(args.checkpoint_name):
            raise NotImplementedError("Could not restore weights for checkpoint %s because `no such file` (pass the path "
                                      "of a checkpoint, e.g. <output_dir>/itr_<t>.pt)" % args.checkpoint_name)
        t0, epoch = trainer.load_checkpoint(args.checkpoint_name)
    packed = args.dataset.startswith("packed")
    cfg = synth_config(args, per_rank)
    evaluator = None
    if args.val_every > 0:
        from ..evaluate import Evaluator
        from . import evaluate as val_cli
        evaluator = Evaluator(trainer)
        val_set = val_cli.folder_val_set(args, args.vocab)   # read once; refused if its vocabulary is not the model's
    builder = real = None
    if train_set is not None:
        steps_per_epoch = len(train_set) // (per_rank * max(world, 1))
        if steps_per_epoch < 1:
            raise SystemExit("the training set has %d images after filtering: fewer than one batch of %d" % (
                len(train_set), per_rank * max(world, 1)))
        builder = folder_builder(train_set, args, trainer, dev)

        def index_lists():               # iteration t is step (t - 1) % steps_per_epoch of epoch (t - 1) // steps_per_epoch
            for t in range(t0 + 1, args.num_iterations + 1):
                e, s = divmod(t - 1, steps_per_epoch)
                if s == 0 or t == t0 + 1:
                    lists = epoch_batches(len(train_set), per_rank, rank, max(world, 1), seed=0, epoch=e)
                yield lists[s]

        real = builder.batches(index_lists())
    if rank == 0:
        print("data: %s" % ("%d pictures of %s, %d loader threads" % (len(train_set), train_set.image_dir, builder.num_workers)
                            if train_set is not None else "seeded synthetic batches (%s shapes)" % args.dataset), flush=True)
        if trainer.d_augment is not None:
            print("d_augment: %s" % trainer.d_augment.meta(), flush=True)
    tic = time.time()
    for t in range(t0 + 1, args.num_iterations + 1):
        if real is not None:
            batch = next(real)
            epoch = (t - 1) // steps_per_epoch
        else:
            batch = make_batch(args.vocab, cfg, seed=t * max(world, 1) + rank)
            if packed:                   # canonical graph from the geometry (and annotations), on the device
                batch = packed_batch(args, trainer, batch, dev)
            else:
                batch = [None if x is None else x.to(dev) for x in batch]
        G, D = trainer.step(batch)
        if rank == 0 and (t % args.print_every == 0 or t == args.num_iterations):
            torch.cuda.synchronize()
            rate = args.print_every * args.batch_size / max(time.time() - tic, 1e-9)
            tic = time.time()
            terms = " ".join("%s %.4f" % (k, float(v.detach())) for k, v in list(G.items()) + list(D.items()) if v.numel() == 1)
            print("t = %d / %d  [%.1f img/s]  %s" % (t, args.num_iterations, rate, terms), flush=True)
            if trainer.d_augment is not None and trainer.d_augment.gated:
                c = trainer.d_augment.read()                 # the only read-back of the controller outside checkpoints
                print("d_augment: p %.4f r_t %.4f" % (c["p"], c["r_t"]), flush=True)
        if evaluator is not None and t % args.val_every == 0:
            import contextlib
            vargs = argparse_copy(args, batch_size=per_rank)
            with (contextlib.nullcontext() if rank == 0 else contextlib.redirect_stdout(open(os.devnull, "w"))):
                validate_in_training(vargs, trainer, evaluator, dev, t, world, val_set)
            tic = time.time()
        if args.output_dir and t % args.checkpoint_every == 0:
            os.makedirs(args.output_dir, exist_ok=True)
            trainer.save_checkpoint(os.path.join(args.output_dir, "itr_%s.pt" % t), t, epoch)      # scripts/train.py:427
    if builder is not None:
        if rank == 0:
            print("loader: %d of %d steps waited for their batch" % (builder.waited, builder.steps), flush=True)
        builder.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
