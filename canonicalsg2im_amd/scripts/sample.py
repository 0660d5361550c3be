"""Command-line sampler: a checkpoint and seeded SYNTHETIC scene graphs in, PNG files out.

The reference's scripts/run_model.py and scripts/generation_attspade.py read scene graphs from its datasets.  This command
does not yet: scripts/train.py and scripts/evaluate.py of this package read a COCO folder (sg2im/data/packed_coco.py), the
sampler's graphs are still the seeded synthetic batches of the chosen dataset's shape — with a checkpoint trained on the
folder, whose vocabulary the checkpoint carries, pass graphs to `Sampler.generate` directly.  The reference's flags describe
the model; on top of them:

    --checkpoint_name PATH   a checkpoint of `Trainer.save_checkpoint` or of the reference (default: none — the freshly
                             initialised weights, which is only good for timing)
    --output_dir DIR         where img_%06d.png go (default: nothing is written)
    --num_samples N          pictures to generate (default 16), in batches of --batch_size

    python -m canonicalsg2im_amd.scripts.sample --dataset packed_coco --image_size 256,256 --batch_size 16 \\
        --checkpoint_name out/itr_100000.pt --output_dir samples --num_samples 64
"""
import os
import sys
import time

import torch

_NO_CHECKPOINT = "checkpoint"           # the reference's default of --checkpoint_name: no file was named


def build_parser():
    from .args import build_parser as train_parser
    p = train_parser()
    p.add_argument('--num_samples', default=16, type=int)
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.num_samples < 1 or args.batch_size < 1:
        raise SystemExit("--num_samples and --batch_size must be positive")
    if args.checkpoint_name != _NO_CHECKPOINT and not os.path.isfile(args.checkpoint_name):
        raise SystemExit("--checkpoint_name %s: no such file" % args.checkpoint_name)
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    from ..sample import Sampler
    from ..synth import BatchConfig, make_batch, make_vocab
    from .args import init_args
    from .train import _vocab_kind, packed_batch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    args.vocab = make_vocab(_vocab_kind(args.dataset))
    init_args(args)
    torch.manual_seed(0)
    sampler = Sampler(args, dev, None if args.checkpoint_name == _NO_CHECKPOINT else args.checkpoint_name)
    packed = args.dataset.startswith("packed")
    lo = args.min_objects or (16 if packed else 3)
    hi = args.max_objects or (40 if packed else 8)
    graph = ("annotated" if args.dataset == "packed_vg" else "packed") if packed else "random"
    cfg = BatchConfig(args.batch_size, args.image_size[0], lo, hi, graph, mask_size=args.mask_size)
    Image = None
    if args.output_dir:
        from PIL import Image                      # only here: importing the package never needs PIL
        os.makedirs(args.output_dir, exist_ok=True)
    done, t = 0, 0
    tic = time.time()
    while done < args.num_samples:
        t += 1
        batch = make_batch(args.vocab, cfg, seed=t)
        batch = packed_batch(args, sampler, batch, dev) if packed else [None if x is None else x.to(dev) for x in batch]
        _, objs, boxes, triplets, _, triplet_type, masks, _ = batch
        imgs = sampler.generate(objs, triplets, triplet_type, boxes_gt=boxes, masks_gt=masks)[0]
        n = min(imgs.shape[0], args.num_samples - done)
        if Image is not None:
            host = imgs[:n].permute(0, 2, 3, 1).contiguous().cpu().numpy()
            for i in range(n):
                Image.fromarray(host[i]).save(os.path.join(args.output_dir, "img_%06d.png" % (done + i)))
        done += n
    torch.cuda.synchronize()
    print("%d images in %.2f s  [%.1f img/s]  (%d replayed, %d eager calls)" % (
        done, time.time() - tic, done / max(time.time() - tic, 1e-9), sampler.replays, sampler.eager_calls), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
