"""Command-line sampler: a checkpoint and scene graphs in, PNG files out.

With --scene_graphs FILE.json the graphs are the ones a person wrote (canonicalsg2im_amd/authored.py: the form of the
reference's scripts/run_model.py, or a flat one), as that script draws them.  Without it they are seeded SYNTHETIC batches
of the chosen dataset's shape (the reference's scripts/generation_attspade.py reads its datasets; for a dataset folder,
pass a batch builder's batch to `Sampler.generate` directly).  The reference's flags describe the model; on top of them:

    --checkpoint_name PATH   a checkpoint of `Trainer.save_checkpoint` or of the reference (default: none — the freshly
                             initialised weights, which is only good for timing)
    --output_dir DIR         where img_%06d.png go (default: nothing is written)
    --num_samples N          pictures to generate (default 16), in batches of --batch_size
    --scene_graphs FILE      authored scene graphs (JSON), drawn in batches of --batch_size; the vocabulary is the one the
                             checkpoint carries, --num_samples is ignored.  Writes img_%06d_generated.png, with
                             --draw_boxes 1 (the default) img_%06d_layout.png — the picture with the outlines of the
                             predicted boxes, no text labels — and graphs.json, the encoded triplets with their
                             predicates' names (in place of the reference's GraphViz picture)

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
    p.add_argument('--scene_graphs', default=None, type=str)
    p.add_argument('--draw_boxes', default=1, type=int)
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.num_samples < 1 or args.batch_size < 1:
        raise SystemExit("--num_samples and --batch_size must be positive")
    if args.checkpoint_name != _NO_CHECKPOINT and not os.path.isfile(args.checkpoint_name):
        raise SystemExit("--checkpoint_name %s: no such file" % args.checkpoint_name)
    if args.scene_graphs is not None and not os.path.isfile(args.scene_graphs):
        raise SystemExit("--scene_graphs %s: no such file" % args.scene_graphs)
    return args


def sample_scene_graphs(args, dev):
    """--scene_graphs: the authored graphs of a JSON file through `Sampler.generate_from_graphs`."""
    import json

    from .. import authored
    from ..sample import Sampler
    from .args import init_args
    if args.checkpoint_name == _NO_CHECKPOINT:
        raise SystemExit("--scene_graphs needs --checkpoint_name: the graphs are read with the checkpoint's vocabulary")
    ckpt = torch.load(args.checkpoint_name, map_location="cpu")
    if not isinstance(ckpt, dict) or not isinstance(ckpt.get("vocab"), dict):
        raise SystemExit("--checkpoint_name %s carries no vocabulary (no 'vocab' entry): --scene_graphs cannot name its "
                         "objects and predicates" % args.checkpoint_name)
    args.vocab = ckpt["vocab"]
    init_args(args)
    try:
        graphs = authored.load_graphs(args.scene_graphs, args.vocab)
    except ValueError as e:
        raise SystemExit("--scene_graphs %s: %s" % (args.scene_graphs, e))
    torch.manual_seed(0)
    sampler = Sampler(args, dev, ckpt)
    Image = None
    if args.output_dir:
        from PIL import Image
        os.makedirs(args.output_dir, exist_ok=True)
    written = []
    tic = time.time()
    for first in range(0, len(graphs), args.batch_size):
        chunk = graphs[first:first + args.batch_size]
        imgs, _, overlays = sampler.generate_from_graphs(chunk, overlay=bool(args.draw_boxes))
        if Image is not None:
            kinds = [("generated", imgs)] + ([("layout", overlays)] if overlays is not None else [])
            for kind, t in kinds:
                host = t.permute(0, 2, 3, 1).contiguous().cpu().numpy()
                for i in range(len(chunk)):
                    Image.fromarray(host[i]).save(os.path.join(args.output_dir, "img_%06d_%s.png" % (first + i, kind)))
            rows = authored.triplet_names(authored.encode_graphs(chunk, args.vocab)[1], args.vocab)
            written.extend({"objects": g["objects"], "triplets": r} for g, r in zip(chunk, rows))
    torch.cuda.synchronize()
    if Image is not None:
        with open(os.path.join(args.output_dir, "graphs.json"), "w") as f:
            json.dump(written, f, indent=1)
    done = len(graphs)
    print("%d images in %.2f s  [%.1f img/s]  (%d replayed, %d eager calls)" % (
        done, time.time() - tic, done / max(time.time() - tic, 1e-9), sampler.replays, sampler.eager_calls), flush=True)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    from ..sample import Sampler
    from ..synth import make_batch, make_vocab
    from .args import init_args
    from .train import _vocab_kind, packed_batch, synth_config
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.scene_graphs is not None:
        return sample_scene_graphs(args, dev)
    args.vocab = make_vocab(_vocab_kind(args.dataset))
    init_args(args)
    torch.manual_seed(0)
    sampler = Sampler(args, dev, None if args.checkpoint_name == _NO_CHECKPOINT else args.checkpoint_name)
    packed = args.dataset.startswith("packed")
    cfg = synth_config(args, args.batch_size)
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
