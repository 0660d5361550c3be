"""Command-line trainer for the HIP hot path on SYNTHETIC batches.

The reference's scripts/train.py owns data loading, logging, evaluation and checkpoint policy; of it only the
iteration (:353-393, :468-485) is on the hot path and lives in `canonicalsg2im_amd.train.Trainer`.  This entry point
drives that iteration with the reference's flags on seeded synthetic batches of the chosen dataset's shape (real
datasets are out of scope), one process per GPU:

    python -m canonicalsg2im_amd.scripts.train --dataset packed_clevr --image_size 256,256 --batch_size 48 \\
        --num_iterations 100 --no_vgg_loss --learned_transitivity 1
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m canonicalsg2im_amd.scripts.train ...

For packed datasets the scene graphs are built on the device from the boxes (`sg2im.data.canonical_triplets`), as
the packed data loaders do on the host; `packed_vg` batches carry annotated relationships (synthetic, among the
vocabulary's non-location predicates) that join the graph as in sg2im/data/packed_vg.py:127-142.

`--val_every N` (default 0: off) runs the reference's two validation passes (scripts/train.py:410-424, `GT VAL` and `VAL`)
every N iterations on the seeded synthetic validation set of scripts/evaluate.py (`--num_val_samples` images, seeds disjoint
from the training seeds).  With N > 1 ranks every rank validates the SAME batches and rank 0 prints: the passes advance the
discriminators' spectral-norm vectors and BatchNorm statistics (evaluate.py), which must stay identical across ranks, and
no collective is issued."""
import os
import sys
import time

import torch


def _vocab_kind(dataset):
    return {"vg": "vg", "packed_vg": "vg", "clevr": "clevr", "packed_clevr": "clevr"}.get(dataset, "coco")


def packed_batch(args, trainer, batch, dev):
    """A synthetic packed batch (CPU tensors from synth.make_batch) on `dev`, with the canonical graph built on the
    device: the __image__ row appended to every sample, then canonical_triplets in place of the triplets.  packed_vg
    hands the batch's annotated relationships over, unless --include_relationships 0 (packed_vg.py:128-130)."""
    from ..sg2im.data import canonical_triplets
    rel = None
    if args.dataset == "packed_vg":  # the annotated rows and the object counts are read on the host: hand over CPU tensors
        rel = batch[3] if args.include_relationships else torch.zeros((batch[3].shape[0], 0, 3), dtype=torch.int64)
        n = (batch[1][..., 0] != 0).sum(1) + 1              # real objects + the __image__ row appended below
    batch = [None if x is None else x.to(dev) for x in batch]
    objs, boxes = batch[1], batch[2]
    if rel is None:
        n = (objs[..., 0] != 0).sum(1) + 1
    O = objs.shape[1] + 1
    objs = torch.cat([objs, objs.new_zeros(objs.shape[0], 1, objs.shape[2])], 1)
    boxes = torch.cat([boxes, boxes.new_full((boxes.shape[0], 1, 4), -1.0)], 1)
    centers = boxes[..., :2] + 0.5 * boxes[..., 2:]
    batch[1], batch[2] = objs, boxes
    conv_w = None
    if args.learned_converse:    # the data loader reads the model's converse weights back (scripts/train.py:274-276)
        from ..sg2im.model import get_conv_converse
        conv_w = get_conv_converse(trainer.model).detach().cpu().numpy()
    batch[3], batch[4], batch[5] = canonical_triplets(objs, boxes, centers, n, args.vocab,
                                                      learned_transitivity=bool(args.learned_transitivity),
                                                      learned_converse=bool(args.learned_converse),
                                                      converse_weights=conv_w, triplets=rel)
    assert batch[3].shape[1] > 0 and objs.shape[1] == O
    return batch


def build_parser():
    from .args import build_parser as base_parser
    p = base_parser()
    p.add_argument('--val_every', default=0, type=int)
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
    from ..synth import BatchConfig, make_batch, make_vocab
    from .args import init_args
    args = build_parser().parse_args(argv)
    if args.val_every < 0:
        raise SystemExit("--val_every must be >= 0 (0: no validation)")
    rank, world, local = csg_dist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    args.vocab = make_vocab(_vocab_kind(args.dataset))
    if world > 1:
        args.gpu_ids = ",".join(str(i) for i in range(world))
    init_args(args)
    per_rank = args.batch_size // max(world, 1)
    torch.manual_seed(0)
    trainer = T.Trainer(args, dev)
    t0 = epoch = 0
    if args.restore_checkpoint:
        # scripts/train.py:29-60: `--checkpoint_name` is the PATH of the checkpoint file; a failed restore raises
        if not args.checkpoint_name or not os.path.isfile(args.checkpoint_name):
            raise NotImplementedError("Could not restore weights for checkpoint %s because `no such file` (pass the path "
                                      "of a checkpoint, e.g. <output_dir>/itr_<t>.pt)" % args.checkpoint_name)
        t0, epoch = trainer.load_checkpoint(args.checkpoint_name)
    packed = args.dataset.startswith("packed")
    lo = args.min_objects or (16 if packed else 3)
    hi = args.max_objects or (40 if packed else 8)
    graph = ("annotated" if args.dataset == "packed_vg" else "packed") if packed else "random"
    cfg = BatchConfig(per_rank, args.image_size[0], lo, hi, graph, mask_size=args.mask_size)
    evaluator = None
    if args.val_every > 0:
        from ..evaluate import Evaluator
        from . import evaluate as val_cli
        evaluator = Evaluator(trainer)
    tic = time.time()
    for t in range(t0 + 1, args.num_iterations + 1):
        batch = make_batch(args.vocab, cfg, seed=t * max(world, 1) + rank)
        if packed:                       # canonical graph from the geometry (and annotations), on the device
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
        if evaluator is not None and t % args.val_every == 0:
            import contextlib
            vargs = argparse_copy(args, batch_size=per_rank)
            with (contextlib.nullcontext() if rank == 0 else contextlib.redirect_stdout(open(os.devnull, "w"))):
                val_cli.validate(vargs, evaluator, dev, t, world)
            tic = time.time()
        if args.output_dir and t % args.checkpoint_every == 0:
            os.makedirs(args.output_dir, exist_ok=True)
            trainer.save_checkpoint(os.path.join(args.output_dir, "itr_%s.pt" % t), t, epoch)      # scripts/train.py:427
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
