"""Command-line validation: a checkpoint and a validation set in, the reference's `GT VAL` / `VAL` lines
(scripts/train.py:410-424, :446-449) out.

The reference validates on its datasets' validation split.  With `--dataset packed_coco` and an existing val image directory
(`--coco_val_image_dir`, by default <dataroot>/MSCoco/images/val2017), or `--dataset packed_clevr` and an existing
`--clevr_val_image_dir` (by default <dataroot>/CLEVR/CLEVR_Dialog/images/val), or `--dataset packed_vg` and an existing image
directory and val split file (`--vg_image_dir`, `--val_h5`, by default <dataroot>/vg/images and val.h5 or val.npz; the objects
of a sample are drawn from a stream seeded anew for every pass, so every pass sees the same ones), so does this: the first `--num_val_samples` pictures in
file order, not shuffled, through the same device input stage as scripts/train.py of this package.  Otherwise the
validation set is seeded synthetic batches of the chosen dataset's shape.  The reference's flags describe the model; on top
of them:

    --checkpoint_name PATH   a checkpoint of `Trainer.save_checkpoint` or of the reference (required)
    --use_ema 0|1            1: validate the checkpoint's `model_ema_state`, the exponential moving average of the weights a run
                             with --ema_decay saves (canonicalsg2im_amd/ema.py); the lines then read `EMA GT VAL` / `EMA VAL`.
                             A checkpoint without the entry is refused (default 0: `model_state`)
    --output_dir DIR         where <pass>_<key>_%03d.png, metrics.json and table.json go (default: nothing is written)
    --num_val_samples N      images to validate (default 1024, the reference's), in batches of --batch_size
    --inception_weights FILE torchvision's inception_v3_google-*.pth: both passes also report `inception_mean` /
                             `inception_std` of the generated images (splits=5, scripts/train.py:198,262-268).  `random` is the
                             seeded stand-in (throughput only; the lines then carry inception_stand_in 1).  Loading the real
                             file and the numbers it gives are unchecked here.  Without the flag nothing changes.

    python -m canonicalsg2im_amd.scripts.evaluate --dataset packed_coco --image_size 256,256 --batch_size 16 \\
        --checkpoint_name out/itr_100000.pt --output_dir val --num_val_samples 1024

Seeds.  scripts.train draws batch t of rank r from seed t * world + r, t >= 1: a positive integer below
num_iterations * world + world, which `validation_batches` requires to stay below VAL_SEED_BASE = 2**40.  Validation batch i
is drawn from seed VAL_SEED_BASE + i: the two sets of seeds are disjoint, and the validation set does not depend on how
long or on how many ranks the model was trained.

Two passes, as the reference runs them at every checkpoint: ground-truth boxes and masks into the generator (`GT VAL`), then
the predicted ones (`VAL`; with --skip_graph_model 1 there is no prediction and the second pass uses the ground truth too,
:419).  The samples written are those of the second pass (:424).
"""
import json
import os
import sys

import torch

VAL_SEED_BASE = 2 ** 40
_NO_CHECKPOINT = "checkpoint"           # the reference's default of --checkpoint_name: no file was named


def build_parser():
    from .args import build_parser as train_parser
    p = train_parser()
    p.add_argument("--inception_weights", default=None)
    p.add_argument("--use_ema", default=0, type=int, choices=[0, 1])
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.checkpoint_name == _NO_CHECKPOINT:
        raise SystemExit("--checkpoint_name PATH is required: there is nothing to validate without trained weights")
    if not os.path.isfile(args.checkpoint_name):
        raise SystemExit("--checkpoint_name %s: no such file" % args.checkpoint_name)
    if args.num_val_samples is None or args.num_val_samples < 1 or args.batch_size < 1:
        raise SystemExit("--num_val_samples and --batch_size must be positive")
    return args


def validation_batches(args, trainer, dev, world=1, val_set=None):
    """Generator of the validation batches on `dev`, ceil(num_val_samples / batch_size) of them: the first pictures of
    `val_set` (a folder dataset, `folder_val_set`) in file order, or the seeded synthetic batches (see Seeds above)."""
    from ..synth import make_batch
    from .train import packed_batch, synth_config
    if val_set is not None:              # the first num_val_samples pictures in file order; every rank sees the same batches
        from ..sg2im.data.loader import file_order_batches
        import random
        from .train import folder_builder
        # a Visual Genome builder samples objects: a fresh stream per call, so every rank and every call sees the same ones
        builder = folder_builder(val_set, args, trainer, dev, rng=random.Random(0))
        try:
            yield from builder.batches(file_order_batches(len(val_set), args.batch_size))
        finally:
            builder.close()
        return
    if (args.num_iterations + 1) * max(world, 1) >= VAL_SEED_BASE:
        raise SystemExit("--num_iterations * ranks must stay below 2**40: the seeds above are the validation set's")
    packed = args.dataset.startswith("packed")
    cfg = synth_config(args, args.batch_size)
    for i in range(-(-args.num_val_samples // args.batch_size)):
        batch = make_batch(args.vocab, cfg, seed=VAL_SEED_BASE + i)
        yield packed_batch(args, trainer, batch, dev) if packed else [None if x is None else x.to(dev) for x in batch]


def folder_val_set(args, vocab=None):
    """The val split's folder dataset, or None (synthetic validation batches).  `vocab`: the vocabulary the model was built
    with; a val split whose categories, attribute tables or predicates differ from it is refused here, on the host — its
    ids would index the model's embedding tables."""
    from .train import folder_dataset, hold_to_vocab
    if args.dataset == "packed_clevr_syn":              # no pictures: check_model's losses have nothing to compare with
        from ..sg2im.data.packed_clevr_syn import NO_VALIDATION
        raise SystemExit(NO_VALIDATION)
    return hold_to_vocab(folder_dataset(args, "val"), vocab, "val")


def log_results(losses, t, prefix):
    """The reference's log_results (:446-449) and its G [name] lines, on one line per pass."""
    head = "Iter: %s, %s avg_iou: %.4f total_iou_03: %.4f total_iou_05: %.4f" % (
        t, prefix, float(losses.get("avg_iou", 0.0)), float(losses.get("total_iou_03", 0.0)), float(losses.get("total_iou_05", 0.0)))
    rest = " ".join("%s %.4f" % (k, float(v)) for k, v in losses.items() if k not in ("avg_iou", "total_iou_03", "total_iou_05"))
    print(head + ("  " + rest if rest else ""), flush=True)


def validate(args, evaluator, dev, t, world=1, val_set=None, inception=None, prefix=""):
    """The two passes of scripts/train.py:410-424 -> (gt_val_losses, val_losses, val_samples, val_table).  `prefix` goes in
    front of the passes' names on the printed lines ("EMA ": the averaged weights are being validated)."""
    tr = evaluator.trainer
    extra = {} if inception is None else {"inception": inception}
    gt_losses, _, _ = evaluator.check_model(validation_batches(args, tr, dev, world, val_set), use_gt=True, **extra)
    log_results(gt_losses, t, prefix + "GT VAL")
    use_gt = bool(args.skip_graph_model)                                          # :419
    losses, samples, table = evaluator.check_model(validation_batches(args, tr, dev, world, val_set), use_gt=use_gt, **extra)
    log_results(losses, t, prefix + "VAL")
    return gt_losses, losses, samples, table


def write_outputs(out_dir, gt_losses, losses, samples, table, tag="val"):
    from PIL import Image                      # only here: importing the package never needs PIL
    os.makedirs(out_dir, exist_ok=True)
    for key, imgs in samples.items():
        host = imgs.numpy()
        for i in range(host.shape[0]):
            Image.fromarray(host[i]).save(os.path.join(out_dir, "%s_%s_%03d.png" % (tag, key, i)))
    num = lambda d: {k: float(v) for k, v in d.items()}
    with open(os.path.join(out_dir, "metrics.json"), "w") as f:
        json.dump({"GT VAL": num(gt_losses), "VAL": num(losses)}, f, indent=1)
    with open(os.path.join(out_dir, "table.json"), "w") as f:
        json.dump({k: v.tolist() for k, v in table.items()}, f)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    from .. import train as T
    from ..evaluate import Evaluator
    from ..synth import make_vocab
    from .args import init_args
    from .train import _vocab_kind
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    val_set = folder_val_set(args)
    if val_set is not None and args.dataset in ("packed_vg", "vg"):   # vocab.json is a file of its own: hold it to the checkpoint's
        val_set = folder_val_set(args, torch.load(args.checkpoint_name, map_location="cpu").get("vocab"))
    args.vocab = val_set.vocab if val_set is not None else make_vocab(_vocab_kind(args.dataset))
    print("data: %s" % ("%d pictures of %s" % (len(val_set), val_set.image_dir) if val_set is not None
                        else "seeded synthetic batches (%s shapes)" % args.dataset), flush=True)
    init_args(args)
    torch.manual_seed(0)
    trainer = T.Trainer(args, dev)
    ckpt = torch.load(args.checkpoint_name, map_location=dev)
    t, _ = trainer.load_checkpoint(ckpt)
    use_ema = bool(getattr(args, "use_ema", 0))
    if use_ema:                          # the averaged weights over the raw ones, through the sampler's strict path
        from .. import ops
        from ..sample import model_state_of
        try:
            trainer.model.load_state_dict(model_state_of(ckpt, use_ema=True), strict=True)
        except KeyError as e:
            raise SystemExit("--use_ema 1: %s" % (e.args[0],))
        ops.invalidate_weight_caches()
    del ckpt
    net = None
    if getattr(args, "inception_weights", None):
        from ..inception import InceptionV3
        net = InceptionV3("torchvision", args.inception_weights).to(dev)
    gt_losses, losses, samples, table = validate(args, Evaluator(trainer), dev, t, val_set=val_set, inception=net,
                                                 prefix="EMA " if use_ema else "")
    if args.output_dir:
        write_outputs(args.output_dir, gt_losses, losses, samples, table)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main(sys.argv[1:])
