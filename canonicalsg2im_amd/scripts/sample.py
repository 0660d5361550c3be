"""Command-line sampler: a checkpoint and scene graphs in, PNG files out.

With --scene_graphs FILE.json the graphs are the ones a person wrote (canonicalsg2im_amd/authored.py: the form of the
reference's scripts/run_model.py, or a flat one), as that script draws them.  With --split train|val they are the graphs of
a dataset folder, and every image id gets its real, ground-truth-layout and predicted-layout picture (the reference's
scripts/generation_attspade.py; canonicalsg2im_amd/split.py).  With --layouts FILE.json they are rows of object classes and
boxes, drawn by the generator alone (its scripts/generation_dataframe.py).  Without any of the three they are seeded
SYNTHETIC batches of the chosen dataset's shape.  The three flags exclude each other.  The reference's flags describe the
model; on top of them:

    --checkpoint_name PATH   a checkpoint of `Trainer.save_checkpoint` or of the reference (default: none — the freshly
                             initialised weights, which is only good for timing)
    --use_ema 0|1            1: draw from the checkpoint's `model_ema_state`, the exponential moving average of the weights a
                             run with --ema_decay saves (canonicalsg2im_amd/ema.py), in every mode below; needs
                             --checkpoint_name, and a checkpoint without the entry is refused (default 0: `model_state`)
    --output_dir DIR         where img_%06d.png go (default: nothing is written)
    --num_samples N          pictures to generate (default 16), in batches of --batch_size
    --scene_graphs FILE      authored scene graphs (JSON), drawn in batches of --batch_size; the vocabulary is the one the
                             checkpoint carries, --num_samples is ignored.  Writes img_%06d_generated.png, with
                             --draw_boxes 1 (the default) img_%06d_layout.png — the picture with the outlines of the
                             predicted boxes — and graphs.json, the encoded triplets with their predicates' names (the
                             graph as a picture: --draw_scene_graphs)
    --draw_labels 0|1        with --draw_boxes 1 (refused without): the objects' names on the layout pictures, a coloured
                             strip with the name across the top of each box as the reference's sg2im/vis.py draws it
                             (default 0).  --scene_graphs: on img_%06d_layout.png; --split: on layout/gt/ and
                             layout/pred/; --layouts: writes layout/<which>/<image id>.<ext> besides, the picture under
                             its boxes' outlines and names
    --draw_scene_graphs 0|1|2  with --scene_graphs (refused without; for --split and --layouts it is out of scope): the
                             picture of each graph itself as img_%06d_sg.png, at the graph's own size — objects and
                             predicates as nodes, two arrows per triplet (canonicalsg2im_amd/sgdraw.py; the reference's
                             flag, drawn there by GraphViz).  0 (default): none.  1: the host-encoded graph, what
                             graphs.json lists.  2: the canonical graph the model was given, with transitive and converse
                             edges in colours of their own; one read-back of the triplets per batch
    --split train|val        the split's folder (the paths of scripts/train.py; --num_train_samples / --num_val_samples cap
                             it, --coco_val_ids narrows coco's val) in file order, batches of --batch_size decoded in
                             --loader_num_workers threads.  Needs --checkpoint_name; the folder's vocabulary is held to the
                             checkpoint's.  A missing folder ends the run: there is no synthetic stand-in.  Writes
                             <output_dir>/gt/, generation/gt_box_gt_mask/, generation/pred_box_pred_mask/ (not with
                             --skip_graph_model 1), with --draw_boxes 1 layout/gt/ and layout/pred/ — <image id>.<ext> in
                             each — and layouts.json: the IoU figures and per image the counted objects' names, boxes,
                             predicted boxes and IoU.  The pictures go through --img_deprocess (decode_img, the default and
                             the inverse of CLEVR's and Visual Genome's normalisation, or imagenet, the COCO folders')
    --max_pictures N         with --split: stop after N images (0, the default: the whole split)
    --image_format png|jpg   with --split / --layouts: png (default, lossless) or jpg (Pillow, quality 95)
    --num_writers N          with --split / --layouts: threads that encode the files, 1 .. 16 (default 8)
    --layouts FILE           a layouts.json (its `images` rows, or a bare list of rows); needs --checkpoint_name and
                             --output_dir; the vocabulary is the checkpoint's.  Writes
                             generation/<which>_box_<which>_mask/<image id>.<ext>; the scene-graph encoder is not run
    --layout_boxes pred|gt   with --layouts: which boxes of the rows to draw (default pred)
    --dataset packed_clevr_syn   the large-graph generalisation run (the reference's scripts/generate_clevr.py): synthetic
                             CLEVR scenes of --min_objects .. --max_objects objects (15 .. 30), --max_samples of them
                             (1000), drawn from --seed (0) as the reference draws them, in batches of --batch_size (10
                             for this dataset).  --scenes FILE.json: the scenes are read from the file when it exists and
                             written to it otherwise, so that two checkpoints see the same scenes.  Needs
                             --checkpoint_name and --output_dir; excludes the three flags above.  Writes
                             generation/pred_box_pred_mask/ and generation/gt_box_gt_mask/ (<image id>.<ext>),
                             layouts.json and generalisation.json: the IoU figures, the share of the graph's location
                             triplets that the predicted layout obeys (ops.relation_agreement) by triplet type and by
                             predicate, and both by the number of objects in the graph.  --inception_weights FILE: the
                             Inception score of the predicted-layout pictures over 5 splits as well
    --rewrite one_sided|noise    with --dataset packed_clevr_syn (refused with any other): the robustness run.  Every scene's
                             minimal graph (A) is also rewritten on the device into graph B — one_sided: an EQUIVALENT
                             graph, a share of the pairs stated in one direction only; noise: a share of the rows with a
                             wrong location predicate — and both are laid out and drawn.  --rewrite_share S in [0, 1]
                             (default 1), --rewrite_direction forward|backward|random (one_sided; default random),
                             --rewrite_seed N (default 0).  The checkpoint's --learned_transitivity / --learned_converse
                             are applied to both graphs.  Writes, besides the files above,
                             generation/pred_box_pred_mask_rewritten/ and robustness.json: the IoU figures of both
                             layouts, B's boxes against A's (IoU, centre shift), the pair relations both layouts share,
                             B's agreement with the clean graph, and all of them by the number of objects

The two modes without --split / --layouts deprocess with imagenet_deprocess whatever --img_deprocess says.

    python -m canonicalsg2im_amd.scripts.sample --dataset packed_coco --image_size 256,256 --batch_size 16 \\
        --checkpoint_name out/itr_100000.pt --output_dir samples --num_samples 64
    python -m canonicalsg2im_amd.scripts.sample --dataset packed_clevr --image_size 256,256 --batch_size 16 \\
        --checkpoint_name out/itr_100000.pt --output_dir val_pictures --split val --loader_num_workers 16
"""
import os
import sys
import time

import torch

_NO_CHECKPOINT = "checkpoint"           # the reference's default of --checkpoint_name: no file was named
SYN = "packed_clevr_syn"


def build_parser():
    from .args import build_parser as train_parser
    p = train_parser()
    p.add_argument('--num_samples', default=16, type=int)
    p.add_argument('--use_ema', default=0, type=int, choices=[0, 1],
                   help="1: sample the checkpoint's model_ema_state (written by a run with --ema_decay), not model_state")
    p.add_argument('--scene_graphs', default=None, type=str)
    p.add_argument('--draw_boxes', default=1, type=int)
    p.add_argument('--draw_labels', default=0, type=int)
    p.add_argument('--draw_scene_graphs', default=0, type=int, choices=[0, 1, 2],
                   help="with --scene_graphs: img_%%06d_sg.png, the picture of each graph (1: as encoded on the host, 2: the "
                        "canonical graph with edge types coloured); not available with --split or --layouts")
    p.add_argument('--split', default=None, choices=["train", "val"])
    p.add_argument('--max_pictures', default=0, type=int)
    p.add_argument('--image_format', default="png", choices=["png", "jpg"])
    p.add_argument('--num_writers', default=8, type=int)
    p.add_argument('--layouts', default=None, type=str)
    p.add_argument('--layout_boxes', default="pred", choices=["pred", "gt"])
    p.add_argument('--max_samples', default=1000, type=int, help="--dataset packed_clevr_syn: the number of scenes")
    p.add_argument('--seed', default=0, type=int, help="--dataset packed_clevr_syn: the seed the scenes are drawn from")
    p.add_argument('--scenes', default=None, type=str,
                   help="--dataset packed_clevr_syn: a JSON file of scenes, read when it exists and written otherwise")
    p.add_argument('--inception_weights', default=None, type=str,
                   help="--dataset packed_clevr_syn: inception_v3_google-*.pth (or 'random', a stand-in)")
    p.add_argument('--rewrite', default=None, choices=["one_sided", "noise"],
                   help="--dataset packed_clevr_syn: the robustness run; every graph also rewritten into an equivalent "
                        "(one_sided) or a corrupted (noise) one; writes robustness.json")
    p.add_argument('--rewrite_share', default=1.0, type=float, help="--rewrite: the share of rows rewritten, in [0, 1]")
    p.add_argument('--rewrite_direction', default="random", choices=["forward", "backward", "random"],
                   help="--rewrite one_sided: the form a rewritten row takes")
    p.add_argument('--rewrite_seed', default=0, type=int, help="--rewrite: the seed of the rows' hash and the converse draws")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.dataset == SYN:                 # scripts/generate_clevr.py's defaults where this dataset has its own
        p.set_defaults(batch_size=10, min_objects=15, max_objects=30)
        args = p.parse_args(argv)
    if args.num_samples < 1 or args.batch_size < 1:
        raise SystemExit("--num_samples and --batch_size must be positive")
    if args.checkpoint_name != _NO_CHECKPOINT and not os.path.isfile(args.checkpoint_name):
        raise SystemExit("--checkpoint_name %s: no such file" % args.checkpoint_name)
    if args.use_ema and args.checkpoint_name == _NO_CHECKPOINT:
        raise SystemExit("--use_ema 1 needs --checkpoint_name: the averaged weights are read from a checkpoint written with "
                         "--ema_decay")
    if args.draw_labels and not args.draw_boxes:
        raise SystemExit("--draw_labels 1 needs --draw_boxes 1: the names go on the layout pictures, which --draw_boxes 0 "
                         "leaves out")
    if args.draw_scene_graphs and args.scene_graphs is None:
        raise SystemExit("--draw_scene_graphs %d needs --scene_graphs: only authored graphs get a picture of the graph "
                         "(--split and --layouts are out of its scope)" % args.draw_scene_graphs)
    if args.scene_graphs is not None and not os.path.isfile(args.scene_graphs):
        raise SystemExit("--scene_graphs %s: no such file" % args.scene_graphs)
    given = [flag for flag, v in (("--split", args.split), ("--layouts", args.layouts), ("--scene_graphs", args.scene_graphs))
             if v is not None]
    if len(given) > 1:
        raise SystemExit("%s exclude each other: a run draws a dataset split, a file of layouts or authored graphs" % (
            " and ".join(given)))
    if args.rewrite is not None:
        if args.dataset != SYN:
            raise SystemExit("--rewrite %s goes with --dataset %s alone (got --dataset %s): the robustness run rewrites graphs "
                             "whose every relation follows from the boxes; other datasets are out of its scope" % (
                                 args.rewrite, SYN, args.dataset))
        if not 0.0 <= args.rewrite_share <= 1.0:
            raise SystemExit("--rewrite_share %r: a share in [0, 1] is needed" % (args.rewrite_share,))
        if not 0 <= args.rewrite_seed < (1 << 32):
            raise SystemExit("--rewrite_seed %r: an integer in [0, 2^32) is needed" % (args.rewrite_seed,))
    if args.dataset == SYN:
        if given:
            raise SystemExit("--dataset %s is a run of its own: %s does not go with it" % (SYN, given[0]))
        if args.checkpoint_name == _NO_CHECKPOINT or not args.output_dir:
            raise SystemExit("--dataset %s needs --checkpoint_name and --output_dir: the run measures a trained model and "
                             "its files are its result" % SYN)
        if args.img_deprocess not in ("decode_img", "imagenet"):
            raise SystemExit("--img_deprocess %s: --dataset %s draws through decode_img or imagenet" % (args.img_deprocess, SYN))
        if args.max_pictures < 0 or not 1 <= args.num_writers <= 16:
            raise SystemExit("--max_pictures must be >= 0 and --num_writers within 1 .. 16")
        if args.inception_weights not in (None, "random") and not os.path.isfile(args.inception_weights):
            raise SystemExit("--inception_weights %s: no such file" % args.inception_weights)
    if args.split is not None or args.layouts is not None:
        flag = given[0]
        if args.checkpoint_name == _NO_CHECKPOINT:
            raise SystemExit("%s needs --checkpoint_name: %s" % (flag, "the pictures of untrained weights are of no use to a metric"
                                                                 if args.split else "the rows are read with the checkpoint's vocabulary"))
        if args.img_deprocess not in ("decode_img", "imagenet"):
            raise SystemExit("--img_deprocess %s: %s draws through decode_img or imagenet" % (args.img_deprocess, flag))
        if args.max_pictures < 0 or not 1 <= args.num_writers <= 16:
            raise SystemExit("--max_pictures must be >= 0 and --num_writers within 1 .. 16")
    if args.layouts is not None:
        if not os.path.isfile(args.layouts):
            raise SystemExit("--layouts %s: no such file" % args.layouts)
        if not args.output_dir:
            raise SystemExit("--layouts needs --output_dir: the pictures are its whole result")
    return args


def _rate_line(done, tic, sampler):
    print("%d images in %.2f s  [%.1f img/s]  (%d replayed, %d eager calls)" % (
        done, time.time() - tic, done / max(time.time() - tic, 1e-9), sampler.replays, sampler.eager_calls), flush=True)


def split_dataset(args):
    """--split: the folder dataset, or the end of the run — host only, before any device call."""
    from ..sg2im.data import looked_for
    from .train import folder_dataset
    dataset = folder_dataset(args, args.split)
    if dataset is None:
        raise SystemExit("--split %s: no dataset folder at %s (--dataset %s); there is no synthetic stand-in for a split" % (
            args.split, looked_for(args, args.split), args.dataset))
    return dataset


def sample_split(args, dev, dataset):
    """--split: every picture of the folder through `split.generate_split`."""
    import random

    from ..sample import Sampler
    from ..sg2im.data.loader import file_order_batches
    from ..split import generate_split
    from .args import init_args
    from .evaluate import log_results
    from .train import folder_builder, hold_to_vocab
    ckpt = torch.load(args.checkpoint_name, map_location="cpu")
    hold_to_vocab(dataset, ckpt.get("vocab") if isinstance(ckpt, dict) else None, args.split)
    args.vocab = dataset.vocab
    init_args(args)
    print("data: %d pictures of %s" % (len(dataset), dataset.image_dir), flush=True)
    torch.manual_seed(0)
    sampler = Sampler(args, dev, ckpt, use_ema=bool(args.use_ema))
    # a Visual Genome builder samples objects: a stream seeded anew, so every run sees the same ones (scripts/evaluate.py)
    builder = folder_builder(dataset, args, sampler, dev, rng=random.Random(0))
    tic = time.time()
    try:
        metrics, rows = generate_split(
            sampler, builder.batches(file_order_batches(len(dataset), args.batch_size)), args.output_dir,
            deprocess=args.img_deprocess, draw_boxes=bool(args.draw_boxes), draw_labels=bool(args.draw_labels),
            image_format=args.image_format,
            num_writers=args.num_writers, max_pictures=args.max_pictures, split=args.split)
    finally:
        builder.close()
    torch.cuda.synchronize()
    if metrics:
        log_results(metrics, ckpt.get("counters", {}).get("t", 0), "SPLIT %s" % args.split)
    _rate_line(len(rows), tic, sampler)


def syn_dataset(args):
    """--dataset packed_clevr_syn: the scenes, or the end of the run — host only, before any device call."""
    from ..sg2im.data import build_folder_dataset
    try:
        return build_folder_dataset(args, "val")
    except (ValueError, NotImplementedError) as e:
        raise SystemExit(str(e))


def sample_generalisation(args, dev, dataset):
    """--dataset packed_clevr_syn: the scenes through `split.generate_split(relations=True)`; generalisation.json."""
    import json

    from ..sample import Sampler
    from ..sg2im.data.loader import file_order_batches
    from ..split import generalisation_report, generate_split
    from .args import init_args
    from .train import folder_builder, hold_to_vocab
    ckpt = torch.load(args.checkpoint_name, map_location="cpu")
    hold_to_vocab(dataset, ckpt.get("vocab") if isinstance(ckpt, dict) else None, "synthetic")
    args.vocab = dataset.vocab
    init_args(args)
    print("data: %d scenes, %s" % (len(dataset), dataset.image_dir), flush=True)
    torch.manual_seed(0)
    sampler = Sampler(args, dev, ckpt, use_ema=bool(args.use_ema))
    rewrite, builder_args = None, args
    if args.rewrite is not None:
        # the robustness run: the batches carry the plain minimal graph, so that a drawn edge is never taken for a source
        # row; the checkpoint's learned_transitivity / learned_converse are applied to both graphs in generate_split
        import argparse

        from ..split import Rewrite, robustness_report
        rewrite = Rewrite(args.rewrite, float(args.rewrite_share), args.rewrite_direction, int(args.rewrite_seed))
        builder_args = argparse.Namespace(**dict(vars(args), learned_transitivity=0, learned_converse=0))
    builder = folder_builder(dataset, builder_args, sampler, dev)
    tic = time.time()
    try:
        metrics, rows = generate_split(
            sampler, builder.batches(file_order_batches(len(dataset), args.batch_size)), args.output_dir,
            deprocess=args.img_deprocess, image_format=args.image_format, num_writers=args.num_writers,
            max_pictures=args.max_pictures, split="synthetic", relations=True,
            **({} if rewrite is None else {"rewrite": rewrite}))
    finally:
        builder.close()
    torch.cuda.synchronize()
    run = dict(dataset=SYN, checkpoint=args.checkpoint_name, seed=None if dataset.loaded else dataset.seed, scenes=args.scenes,
               min_objects=min(len(s["objects"]) for s in dataset.scenes),
               max_objects=max(len(s["objects"]) for s in dataset.scenes))
    if rewrite is not None:
        robust = robustness_report(metrics, rows, rewrite={"mode": rewrite.mode, "share": rewrite.share,
                                                           "direction": rewrite.direction, "seed": rewrite.seed}, **run)
        with open(os.path.join(args.output_dir, "robustness.json"), "w") as f:
            json.dump(robust, f, indent=1)
        c, r = robust["consistency"], robust["pair_relations"]
        print("rewrite %s share %s: avg_iou %s -> %s; consistency avg_iou %s, avg_shift %s; same pairs %s of %s" % (
            rewrite.mode, rewrite.share, robust["clean"]["avg_iou"], robust["rewritten"]["avg_iou"], c["avg_iou"], c["avg_shift"],
            r["same_pairs"], r["pairs"]), flush=True)
        metrics = {k: v for k, v in metrics.items() if k != "rewritten"}
    report = generalisation_report(metrics, rows, **run)
    for k in ("avg_iou", "total_iou_05", "total_iou_03"):         # generate_clevr.py's three lines
        if k in metrics:
            print("%s: %s" % (k, metrics[k]), flush=True)
    agreement = metrics.get("relation_agreement")
    if agreement:
        print("relation_agreement: %s of %s tested triplets (%s)" % (agreement["agreeing"], agreement["tested"], agreement["rate"]))
    if args.inception_weights:
        from .. import quality
        from ..inception import InceptionV3
        from .quality import batches, list_files
        net = InceptionV3("torchvision", args.inception_weights).to(dev)
        scorer = quality.InceptionScore(net, channel_order="rgb")
        folder = os.path.join(args.output_dir, "generation", "pred_box_pred_mask")
        for pics in batches(list_files(folder), min(50, len(rows)), dev):
            scorer.update(pics)
        mean, std = scorer.compute(5)
        label = "  [stand-in weights: the number means nothing]" if net.stand_in else ""
        print("inception_mean: %s%s\ninception_std: %s%s" % (mean, label, std, label), flush=True)
        report["inception_score"] = {"mean": mean, "std": std, "splits": 5, "stand_in": bool(net.stand_in)}
    with open(os.path.join(args.output_dir, "generalisation.json"), "w") as f:
        json.dump(report, f, indent=1)
    _rate_line(len(rows), tic, sampler)


def sample_layouts(args, dev):
    """--layouts: the rows of a layouts.json through `split.generate_layouts`."""
    import json

    from ..sample import Sampler
    from ..split import encode_layouts, generate_layouts
    from .args import init_args
    ckpt = torch.load(args.checkpoint_name, map_location="cpu")
    if not isinstance(ckpt, dict) or not isinstance(ckpt.get("vocab"), dict):
        raise SystemExit("--checkpoint_name %s carries no vocabulary (no 'vocab' entry): --layouts cannot name its objects"
                         % args.checkpoint_name)
    args.vocab = ckpt["vocab"]
    init_args(args)
    with open(args.layouts, "r") as f:
        rows = json.load(f)
    rows = rows.get("images") if isinstance(rows, dict) else rows
    try:
        encode_layouts(rows, args.layout_boxes, args.vocab)
    except ValueError as e:
        raise SystemExit("--layouts %s: %s" % (args.layouts, e))
    torch.manual_seed(0)
    sampler = Sampler(args, dev, ckpt, use_ema=bool(args.use_ema))
    tic = time.time()
    done = generate_layouts(sampler, rows, args.layout_boxes, args.output_dir, deprocess=args.img_deprocess,
                            batch_size=args.batch_size, image_format=args.image_format, num_writers=args.num_writers,
                            draw_labels=bool(args.draw_labels))
    torch.cuda.synchronize()
    _rate_line(done, tic, sampler)


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
    sampler = Sampler(args, dev, ckpt, use_ema=bool(args.use_ema))
    Image = None
    if args.output_dir:
        from PIL import Image
        os.makedirs(args.output_dir, exist_ok=True)
    written = []
    tic = time.time()
    for first in range(0, len(graphs), args.batch_size):
        chunk = graphs[first:first + args.batch_size]
        drawn = sampler.generate_from_graphs(chunk, overlay=bool(args.draw_boxes), labels=bool(args.draw_labels),
                                             **({"return_graph": True} if args.draw_scene_graphs == 2 else {}))
        imgs, _, overlays = drawn[:3]
        if Image is not None and args.draw_scene_graphs:
            from .. import sgdraw
            canvas, sizes = sgdraw.draw_canvas(chunk, args.vocab, dev, *(drawn[3] if args.draw_scene_graphs == 2 else ()))
            host = canvas.permute(0, 2, 3, 1).contiguous().cpu().numpy()
            for i, (w, h) in enumerate(sizes):
                Image.fromarray(host[i, :h, :w]).save(os.path.join(args.output_dir, "img_%06d_sg.png" % (first + i)))
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
    dataset = split_dataset(args) if args.split is not None else (syn_dataset(args) if args.dataset == SYN else None)
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
    if args.split is not None:
        return sample_split(args, dev, dataset)
    if args.layouts is not None:
        return sample_layouts(args, dev)
    if args.dataset == SYN:
        return sample_generalisation(args, dev, dataset)
    args.vocab = make_vocab(_vocab_kind(args.dataset))
    init_args(args)
    torch.manual_seed(0)
    sampler = Sampler(args, dev, None if args.checkpoint_name == _NO_CHECKPOINT else args.checkpoint_name,
                      use_ema=bool(args.use_ema))
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
