"""Command-line FID (and Inception score) of folders of pictures, on the device: the reference's
evaluation/fid/fid_score.py with its behaviours kept.

    python -m canonicalsg2im_amd.scripts.quality A B --fid_weights FILE [--dims 2048] [--batch-size 50]
        [--inception_weights FILE --splits 5] [--channel_order bgr|rgb] [--output_dir DIR]
        [--kid [--kid_subsets 100 --kid_subset_size 1000 --kid_seed 0]]
        [--prdc [--prdc_k 5] [--prdc_real A|B]]
        [--object_crops LAYOUTS.json [--layout_boxes gt|pred] [--min_object_size 0.0] [--class_min_crops 1]]

A and B are folders of *.jpg / *.png, or .npz statistics with `mu` and `sigma` (fid_score.py:218-229).  Prints `FID:`; with
--inception_weights also the Inception score of A (a folder).  Writes DIR/quality.json and, for a folder, its statistics as
DIR/stats_A.npz / stats_B.npz.  PIL decodes on the host; everything after the decode runs on the device.

Opt-in, for two folders (an .npz holds no pictures: the flags are refused for it):
  --kid           `KID: mean +- std` over the pictures FID used (quality.KID; the remainder rule applies to them too)
  --prdc          `Precision:`, `Recall:`, `Density:`, `Coverage:` over the pictures FID used (quality.PRDC, k-nearest-neighbour
                  balls with --prdc_k neighbours; the remainder rule applies); --prdc_real names the folder taken as the real
                  pictures (default A: the ground-truth folder comes first)
  --object_crops  the layouts.json of `scripts.sample --split`: pictures are matched to its rows by file stem = image id;
                  prints `SceneFID:` (FID over the crops of every object's box, all of them: no remainder is dropped), the
                  crops per side and `class_mean_distance:` (per class |mu_B - mu_A|^2, averaged); with --kid also
                  `SceneKID:` and with --prdc `ScenePrecision:` ... `SceneCoverage:` over the crops' features.  Writes stats_A_objects.npz / stats_B_objects.npz and "objects" into quality.json.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

_HELP_EPILOG = """behaviours kept from the reference (evaluation/fid/fid_score.py):
  * the remainder of len(files) % batch_size pictures is DROPPED, with the reference's warning (:90-99);
  * the default --channel_order is bgr: the reference reads with cv2.imread and never converts (:111), so its network sees
    blue first.  rgb is what pytorch-fid does.  Numbers of the two orders are not comparable.
--fid_weights is pytorch-fid's pt_inception-2015-12-05-*.pth, --inception_weights torchvision's inception_v3_google-*.pth.
`random` in their place is a seeded stand-in for tests and throughput runs: its numbers mean nothing and every output says
"stand-in".  Loading the real files and the numbers they give are unchecked here."""


def build_parser():
    p = argparse.ArgumentParser(prog="python -m canonicalsg2im_amd.scripts.quality", epilog=_HELP_EPILOG,
                                formatter_class=argparse.RawDescriptionHelpFormatter,
                                description="FID of two sets of pictures (and the Inception score of the first) on the device")
    p.add_argument("A", help="a folder of *.jpg / *.png, or .npz statistics (mu, sigma)")
    p.add_argument("B", help="likewise")
    p.add_argument("--fid_weights", required=True, help="pt_inception-2015-12-05-*.pth, or 'random' (stand-in)")
    p.add_argument("--dims", type=int, default=2048, choices=[64, 192, 768, 2048])
    p.add_argument("--batch-size", type=int, default=50)
    p.add_argument("--inception_weights", default=None, help="inception_v3_google-*.pth, or 'random' (stand-in)")
    p.add_argument("--splits", type=int, default=5)
    p.add_argument("--channel_order", choices=["bgr", "rgb"], default="bgr")
    p.add_argument("--output_dir", default=".")
    p.add_argument("--kid", action="store_true", help="also KID over the pictures FID used")
    p.add_argument("--kid_subsets", type=int, default=100)
    p.add_argument("--kid_subset_size", type=int, default=1000)
    p.add_argument("--kid_seed", type=int, default=0)
    p.add_argument("--prdc", action="store_true", help="also precision / recall / density / coverage over the pictures FID used")
    p.add_argument("--prdc_k", type=int, default=5, help="neighbours of a ball (5: the prdc package; 3: the improved P&R paper)")
    p.add_argument("--prdc_real", choices=["A", "B"], default="A", help="the folder taken as the real pictures")
    p.add_argument("--object_crops", default=None, metavar="LAYOUTS.json",
                   help="SceneFID over the crops of the boxes of this layouts.json (scripts.sample --split)")
    p.add_argument("--layout_boxes", choices=["gt", "pred"], default="gt")
    p.add_argument("--min_object_size", type=float, default=0.0, help="leave out boxes with w * h below this")
    p.add_argument("--class_min_crops", type=int, default=1, help="crops a class needs on both sides to be averaged")
    return p


def refuse_statistics_files(args):
    """--kid, --object_crops and --prdc work on pictures: an .npz of (mu, sigma) holds none."""
    asked = [flag for flag, on in (("--kid", args.kid), ("--object_crops", args.object_crops is not None),
                                   ("--prdc", args.prdc)) if on]
    for path in (args.A, args.B):
        if asked and path.endswith(".npz"):
            raise SystemExit("%s need%s pictures: %s holds statistics (mu, sigma) only; give the folder"
                             % (" and ".join(asked), "s" if len(asked) == 1 else "", path))


def match_pictures(files, crops, folder):
    """Pictures to layout rows by file stem = image id, both ways: -> [(file, image id)] in file order."""
    by_stem = {str(image_id): image_id for image_id in crops}
    if len(by_stem) != len(crops):
        raise SystemExit("--object_crops: two image ids share one spelling")
    matched, seen = [], set()
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        if stem not in by_stem:
            raise SystemExit("--object_crops: picture %s has no row (image id %s) in the layouts" % (f, stem))
        if stem in seen:
            raise SystemExit("--object_crops: image id %s has two pictures in %s" % (stem, folder))
        seen.add(stem)
        matched.append((f, by_stem[stem]))
    for stem in by_stem:
        if stem not in seen:
            raise SystemExit("--object_crops: image id %s has a row and no picture in %s" % (stem, folder))
    return matched


def object_side(quality, net, args, matched, crops, classes, dev):
    """One folder's crops through quality.ObjectFID, `batch_size` pictures at a time (every picture, every crop)
    -> (the ObjectFID, its crops' features)."""
    from PIL import Image
    ofid = quality.ObjectFID(net, dims=args.dims, channel_order=args.channel_order, batch_size=args.batch_size, classes=classes)
    number = {key: k for k, key in enumerate(classes)}
    feats = []
    for i in range(0, len(matched), args.batch_size):
        part = matched[i:i + args.batch_size]
        pics = [np.asarray(Image.open(f).convert("RGB")) for f, _ in part]
        if any(p.shape != pics[0].shape for p in pics):
            raise SystemExit("pictures of one batch differ in size (%s)" % sorted({p.shape for p in pics}))
        boxes, index, ids = [], [], []
        for k, (_, image_id) in enumerate(part):
            boxes += crops[image_id][0]
            index += [k] * len(crops[image_id][0])
            ids += [number[key] for key in crops[image_id][1]]
        if boxes:
            feats.append(ofid.update(torch.from_numpy(np.stack(pics)).to(dev), boxes, index, ids))
    if ofid.n < 2:
        raise SystemExit("--object_crops: %d crops: a covariance needs two" % ofid.n)
    return ofid, torch.cat(feats)


def list_files(folder):
    """fid_score.py:225: every *.jpg, then every *.png (sorted here, so that a run can be repeated)."""
    return sorted(glob.glob(os.path.join(folder, "*.jpg"))) + sorted(glob.glob(os.path.join(folder, "*.png")))


def batches(files, batch_size, dev):
    """uint8 (B,H,W,3) device tensors of the reference's batches (:90-99): the remainder is dropped."""
    from PIL import Image
    if not files:
        raise SystemExit("no *.jpg / *.png pictures found")
    if len(files) % batch_size != 0:
        print("Warning: number of images is not a multiple of the batch size. Some samples are going to be ignored.")
    if batch_size > len(files):
        print("Warning: batch size is bigger than the data size. Setting batch size to data size")
        batch_size = len(files)
    for i in range(len(files) // batch_size):
        pics = [np.asarray(Image.open(f).convert("RGB")) for f in files[i * batch_size:(i + 1) * batch_size]]
        if any(p.shape != pics[0].shape for p in pics):
            raise SystemExit("pictures of one batch differ in size (%s): the reference stacks them into one array"
                             % sorted({p.shape for p in pics}))
        yield torch.from_numpy(np.stack(pics)).to(dev)


def print_prdc(out, real, label, prefix=""):
    for name in ("precision", "recall", "density", "coverage"):
        print("%s%s: %s%s" % (prefix, name.capitalize(), out[name], label))
    print("%sPRDC: k = %d, real = folder %s (%d rows), generated = the other (%d rows)%s" % (
        prefix, out["k"], real, out["n"][0], out["n"][1], label))


def prdc_of(quality, net, args, feats_a, feats_b):
    """--prdc over the two folders' feature rows, --prdc_real naming the real side -> the "prdc" of quality.json."""
    real, gen = (feats_a, feats_b) if args.prdc_real == "A" else (feats_b, feats_a)
    try:
        out = quality.prdc_from_features(real, gen, args.prdc_k)
    except ValueError as e:
        raise SystemExit("--prdc: %s" % e)
    out["real"] = args.prdc_real
    out["stand_in"] = bool(net.stand_in)
    return out


def objects(quality, net, args, plan, dev, label):
    """--object_crops: SceneFID, the per-class mean distance and, with --kid, SceneKID, with --prdc the four over the crops
    -> the "objects" of quality.json."""
    crops, classes, matched = plan
    sides = []
    for tag, files in zip("AB", matched):
        ofid, feats = object_side(quality, net, args, files, crops, classes, dev)
        stats = ofid.statistics()
        quality.save_statistics(os.path.join(args.output_dir, "stats_%s_objects.npz" % tag), *stats)
        sides.append((ofid, feats, stats))
    (a, feats_a, stats_a), (b, feats_b, stats_b) = sides
    scene_fid = quality.frechet_distance(stats_a[0], stats_a[1], stats_b[0], stats_b[1])
    per = quality.class_mean_distance(*a.class_means(), *b.class_means(), min_crops=args.class_min_crops)
    out = {"scene_fid": scene_fid, "crops": [a.n, b.n], "layout_boxes": args.layout_boxes,
           "min_object_size": args.min_object_size,
           "class_mean_distance": {"mean": per["mean"], "per_class": {classes[c]: d for c, d in per["per_class"].items()},
                                   "missing": [classes[c] for c in per["missing"]]},
           "stand_in": bool(net.stand_in)}
    print("SceneFID: %s  (crops: %d in A, %d in B)%s" % (scene_fid, a.n, b.n, label))
    print("class_mean_distance: %s over %d classes (%d on one side only)%s" % (
        per["mean"], len(per["per_class"]), len(per["missing"]), label))
    if args.kid:
        out["kid"] = quality.kid_from_features(feats_a, feats_b, args.kid_subsets, args.kid_subset_size, args.kid_seed)
        out["kid"]["stand_in"] = bool(net.stand_in)
        print("SceneKID: %s +- %s%s" % (out["kid"]["mean"], out["kid"]["std"], label))
    if args.prdc:
        out["prdc"] = prdc_of(quality, net, args, feats_a, feats_b)
        print_prdc(out["prdc"], args.prdc_real, label, prefix="Scene")
    return out


def read_object_crops(quality, args):
    """The host side of --object_crops, before anything is launched: the layouts' rows and both folders' pictures matched to
    them -> (crops by image id, class keys, [matched files of A, of B])."""
    if not os.path.isfile(args.object_crops):
        raise SystemExit("--object_crops %s: no such file" % args.object_crops)
    with open(args.object_crops, "r") as f:
        doc = json.load(f)
    try:
        crops = quality.crops_from_layouts(doc, args.layout_boxes, args.min_object_size)
    except ValueError as e:
        raise SystemExit("--object_crops %s: %s" % (args.object_crops, e))
    classes = sorted({key for _, keys in crops.values() for key in keys})
    if not classes:
        raise SystemExit("--object_crops %s: no box is left to crop" % args.object_crops)
    return crops, classes, [match_pictures(list_files(path), crops, path) for path in args.path]


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.path = [args.A, args.B]
    refuse_statistics_files(args)
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    from .. import quality
    from ..inception import InceptionV3
    dev = torch.device("cuda", 0)
    for p in args.path:
        if not os.path.exists(p):
            raise SystemExit("Invalid path: %s" % p)
    plan = read_object_crops(quality, args) if args.object_crops is not None else None
    os.makedirs(args.output_dir, exist_ok=True)
    net = InceptionV3("fid", args.fid_weights).to(dev)
    score_net = InceptionV3("torchvision", args.inception_weights).to(dev) if args.inception_weights else None
    stand_in = net.stand_in or bool(score_net is not None and score_net.stand_in)
    label = "  [stand-in weights: the number means nothing]" if stand_in else ""
    stats, counts, score = [], [], None
    kid = quality.KID(net, dims=args.dims, channel_order=args.channel_order, subsets=args.kid_subsets,
                      subset_size=args.kid_subset_size, seed=args.kid_seed) if args.kid else None
    kept = ([], []) if args.prdc else None          # --prdc: the features of both sides, fp32 on the device
    for side, (tag, path) in enumerate(zip("AB", args.path)):
        if path.endswith(".npz"):
            stats.append(quality.load_statistics(path))
            counts.append(None)
            continue
        fid = quality.FID(net, dims=args.dims, channel_order=args.channel_order)
        scorer = quality.InceptionScore(score_net, channel_order=args.channel_order) if (score_net is not None and tag == "A") else None
        for pics in batches(list_files(path), args.batch_size, dev):
            if kid is None and kept is None:
                fid.update(pics)
            else:                                   # the same features, kept
                feats = fid.features(pics)
                fid.update_features(feats)
                if kid is not None:
                    kid.update_features(feats, side)
                if kept is not None:
                    kept[side].append(feats.detach())
            if scorer is not None:
                scorer.update(pics)
        stats.append(fid.statistics())
        counts.append(fid.n)
        quality.save_statistics(os.path.join(args.output_dir, "stats_%s.npz" % tag), *stats[-1])
        if scorer is not None:
            score = scorer.compute(args.splits)
    value = quality.frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])
    print("FID: %s%s" % (value, label))
    result = {"fid": value, "dims": args.dims, "batch_size": args.batch_size, "channel_order": args.channel_order,
              "images": counts, "stand_in": stand_in}
    if score is not None:
        print("Inception score (A): %s +- %s%s" % (score[0], score[1], label))
        result["inception_score"] = {"mean": score[0], "std": score[1], "splits": args.splits}
    if kid is not None:
        result["kid"] = kid.compute()
        print("KID: %s +- %s%s" % (result["kid"]["mean"], result["kid"]["std"], label))
    if kept is not None:
        result["prdc"] = prdc_of(quality, net, args, torch.cat(kept[0]), torch.cat(kept[1]))
        print_prdc(result["prdc"], args.prdc_real, label)
    if plan is not None:
        result["objects"] = objects(quality, net, args, plan, dev, label)
    with open(os.path.join(args.output_dir, "quality.json"), "w") as f:
        json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
